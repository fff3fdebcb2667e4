// Device-side JSONL ingest for MI355X (gfx950): the raw session files -> session / aid / ts / type columns, sess_id and
// the CSR sess_off. C-ABI and SPEC-JSONL in include/otto_jsonl.h. Reference code this replaces:
// create_dataframe of src/utilities/dataset_writer_pickle.py:11-65; host restatement tests/jsonl_restatement.py.
//
// A line falls into pieces (leading ws, header, one per event) that are found from the bytes next to them alone
// (jsonl_parse.h:jsonl_piece_kind), so the indices every piece needs are three prefix counts: newlines (its line), header
// pieces (its session row) and event pieces (its event row).
//   k_jsonl_count  one wave per OTTO_JSONL_TILE bytes, 16-byte loads: the three counts of the tile
//   device_scan    (scan.h) over the per-tile counts only: the workspace is O(tiles)
//   k_jsonl_parse  one workgroup per tile: stages the tile + a MAX_PIECE halo in LDS, rebuilds the per-byte counts with a block scan, compacts the
//                  piece starts into an LDS list and hands the pieces to consecutive threads: the byte loops run dense
//                  and consecutive lanes write consecutive event rows. Every piece validates its own bytes up to the
//                  next piece; the smallest violating line is kept with a 64-bit atomicMin.
//   k_jsonl_expand session row of every event -> its session id
#include "common.h"
#include "scan.h"
#include "jsonl_parse.h"
#include "../../include/otto_jsonl.h"

namespace otto {

constexpr int JL_THREADS = 256;
constexpr int JL_PER = 16;                                  // bytes per thread: one 16-byte load
constexpr int JL_TILE = OTTO_JSONL_TILE;
constexpr int JL_HALO = OTTO_JSONL_MAX_PIECE;
static_assert(JL_TILE == JL_THREADS * JL_PER, "one 16-byte load per thread covers the tile");
static_assert(JL_HALO % JL_PER == 0 && JL_HALO / JL_PER <= JL_THREADS, "the halo is loaded by the first threads");
static_assert(JL_TILE <= (1 << 13), "13-bit fields of the piece list");
static_assert(JL_TILE % (WAVE * JL_PER) == 0, "k_jsonl_count: whole wave loads per tile");
constexpr int JL_LIST = 1024;                               // pieces the LDS list holds per round; a tile of the dataset has about 80

struct JsonlWs {
    unsigned long long* err;      // (line << 8 | reason) of the smallest violating line, ~0 without one
    uint64_t* cnt_a;              // [tiles]      newlines << 32 | header pieces of the tile
    uint64_t* cnt_b;              // [tiles]      event pieces of the tile
    uint64_t* scan_a;             // [tiles + 1]  exclusive scans of the two, totals last
    uint64_t* scan_b;
    uint64_t* partial;
};

static inline size_t jl_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int64_t jl_tiles(int64_t n_bytes) { return (n_bytes + JL_TILE - 1) / JL_TILE; }

static size_t jl_layout(int64_t n_bytes, char* base, JsonlWs* w) {
    const size_t nt = (size_t)jl_tiles(n_bytes);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += jl_align(bytes); return p; };
    JsonlWs t;
    t.err = (unsigned long long*)take(8);
    t.cnt_a = (uint64_t*)take(nt * 8);
    t.cnt_b = (uint64_t*)take(nt * 8);
    t.scan_a = (uint64_t*)take((nt + 1) * 8);
    t.scan_b = (uint64_t*)take((nt + 1) * 8);
    t.partial = (uint64_t*)take(scan_partial_bytes((int64_t)nt));
    if (w) *w = t;
    return o;
}

struct LoadU64 {
    const uint64_t* a;
    __device__ uint64_t operator()(int64_t i) const { return a[i]; }
};

// bytes[pos .. pos + 16), pos a multiple of 16, zero-filled at and past n: nothing at or past n is read
__device__ __forceinline__ uint4 jl_load16(const uint8_t* bytes, int64_t pos, int64_t n) {
    if (pos + JL_PER <= n) return *reinterpret_cast<const uint4*>(bytes + pos);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (int k = 0; k < JL_PER; ++k) {
        const uint32_t b = pos + k < n ? (uint32_t)bytes[pos + k] << (8 * (k & 3)) : 0u;
        if (k < 4) w0 |= b; else if (k < 8) w1 |= b; else if (k < 12) w2 |= b; else w3 |= b;
    }
    return make_uint4(w0, w1, w2, w3);
}

// The thread's 16 bytes: `kinds` holds the piece kind that starts at byte k in bits 2k, 2k + 1; `nl` bit k is set where
// byte k is '\n'. Only a '{' behind ws needs the look-back of jsonl_piece_kind; it goes to global memory, to bytes that the
// tile's loads have just brought in.
struct JlMarks { uint32_t kinds, nl; };
__device__ __forceinline__ JlMarks jl_classify(const uint8_t* bytes, uint4 v, int64_t pos, int64_t n) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    JlMarks m = {0u, 0u};
    int prev = pos > 0 && pos < n ? (int)bytes[pos - 1] : '\n';
#pragma unroll
    for (int k = 0; k < JL_PER; ++k) {
        const int b = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
        if (pos + k < n) {
            if (b == '\n') m.nl |= 1u << k;
            else m.kinds |= (uint32_t)jsonl_piece_kind_after(bytes, pos + k, n, prev, b) << (2 * k);
        }
        prev = b;
    }
    return m;
}
// newlines | header pieces << 16 | event pieces << 32 | pieces << 48 of the 16 bytes
__device__ __forceinline__ uint64_t jl_counts(JlMarks m) {
    const uint32_t lo = m.kinds & 0x55555555u, hi = (m.kinds >> 1) & 0x55555555u;
    return (uint64_t)__popc(m.nl) | (uint64_t)__popc(hi & ~lo) << 16 | (uint64_t)__popc(hi & lo) << 32 |
           (uint64_t)__popc(hi | lo) << 48;
}

// one wave per tile: four 16-byte loads per lane in flight (each wave instruction reads 1 KiB), the counts summed across
// the wave's lanes -- no LDS, no barrier
__global__ __launch_bounds__(JL_THREADS) void k_jsonl_count(const uint8_t* __restrict__ bytes, int64_t n, int64_t n_tiles,
                                                            uint64_t* __restrict__ cnt_a, uint64_t* __restrict__ cnt_b) {
    constexpr int WAVES = JL_THREADS / WAVE, STEPS = JL_TILE / (WAVE * JL_PER);
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                             // wave-uniform
    const int64_t pos0 = tile * JL_TILE + (int64_t)lane_id() * JL_PER;
    uint4 v[STEPS];
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int64_t pos = pos0 + (int64_t)k * WAVE * JL_PER;
        v[k] = pos < n ? jl_load16(bytes, pos, n) : make_uint4(0u, 0u, 0u, 0u);
    }
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int64_t pos = pos0 + (int64_t)k * WAVE * JL_PER;
        if (pos < n) c += jl_counts(jl_classify(bytes, v[k], pos, n));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane_id() == 0) {
        cnt_a[tile] = (c & 0xFFFFull) << 32 | ((c >> 16) & 0xFFFFull);
        cnt_b[tile] = (c >> 32) & 0xFFFFull;
    }
}

__global__ __launch_bounds__(JL_THREADS) void k_jsonl_parse(const uint8_t* __restrict__ bytes, int64_t n, int64_t line0,
                                                            const uint64_t* __restrict__ scan_a, const uint64_t* __restrict__ scan_b,
                                                            int64_t n_tiles, int64_t cap_sessions, int64_t cap_events,
                                                            uint32_t* __restrict__ session, uint32_t* __restrict__ aid,
                                                            int64_t* __restrict__ ts, uint8_t* __restrict__ type,
                                                            int64_t* __restrict__ sess_off, uint32_t* __restrict__ sess_id,
                                                            unsigned long long* err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[JL_TILE + JL_HALO];
    __shared__ uint64_t s_piece[JL_LIST];     // pos | kind << 13 | newlines before << 16 | headers before << 32 | events before << 48
    __shared__ uint64_t sm[JL_THREADS / 64 + 1];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * JL_TILE;
    const int64_t pos = base + (int64_t)tid * JL_PER;
    const uint4 v = jl_load16(bytes, pos, n);
    *reinterpret_cast<uint4*>(s_bytes + tid * JL_PER) = v;
    if (tid < JL_HALO / JL_PER)
        *reinterpret_cast<uint4*>(s_bytes + JL_TILE + tid * JL_PER) = jl_load16(bytes, base + JL_TILE + (int64_t)tid * JL_PER, n);
    JlMarks m = {0u, 0u};
    if (pos < n) m = jl_classify(bytes, v, pos, n);
    uint64_t tot;
    const uint64_t ex = block_excl_scan<uint64_t, JL_THREADS>(jl_counts(m), sm, &tot);     // its barriers publish s_bytes too
    const int n_pieces = (int)(tot >> 48);
    const uint64_t a0 = scan_a[blockIdx.x];
    const int64_t nl0 = (int64_t)(a0 >> 32), hd0 = (int64_t)(a0 & 0xFFFFFFFFull), ev0 = (int64_t)scan_b[blockIdx.x];
    const int64_t n_local = n - base;
    // The list takes JL_LIST pieces per round; only a tile of blank lines or of stray braces needs a second one.
#pragma unroll 1
    for (int lo = 0; lo < n_pieces; lo += JL_LIST) {
        const uint32_t nl = (uint32_t)(ex & 0xFFFFu);
        uint32_t hd = (uint32_t)((ex >> 16) & 0xFFFFu), ev = (uint32_t)((ex >> 32) & 0xFFFFu), pc = (uint32_t)(ex >> 48);
        for (uint32_t rest = m.kinds; rest;) {               // the thread's piece starts, mostly none or one
            const int k = (__ffs((int)rest) - 1) >> 1;
            const uint32_t kind = (m.kinds >> (2 * k)) & 3u;
            rest &= ~(3u << (2 * k));
            if (pc >= (uint32_t)lo && pc < (uint32_t)(lo + JL_LIST))
                s_piece[pc - lo] = (uint64_t)(tid * JL_PER + k) | (uint64_t)kind << 13 |
                                   (uint64_t)(nl + __popc(m.nl & ((1u << k) - 1u))) << 16 | (uint64_t)hd << 32 | (uint64_t)ev << 48;
            ++pc;
            hd += kind == JSONL_HEADER;
            ev += kind == JSONL_EVENT;
        }
        __syncthreads();
        const int here = n_pieces - lo < JL_LIST ? n_pieces - lo : JL_LIST;
#pragma unroll 1
        for (int i = tid; i < here; i += JL_THREADS) {
            const uint64_t e = s_piece[i];
            const int64_t begin = (int64_t)(e & 0x1FFFu);
            const int kind = (int)((e >> 13) & 3u);
            const int64_t row_s = hd0 + (int64_t)((e >> 32) & 0xFFFFu), row_e = ev0 + (int64_t)(e >> 48);
            int reason;
            if (kind == JSONL_EVENT) {
                uint32_t o_aid = 0;
                int64_t o_ts = 0;
                uint8_t o_type = 0;
                reason = jsonl_parse_event(s_bytes, begin, n_local, &o_aid, &o_ts, &o_type);
                if (row_e < cap_events) {
                    aid[row_e] = o_aid;
                    ts[row_e] = o_ts;
                    type[row_e] = o_type;
                    session[row_e] = (uint32_t)(row_s > 0 ? row_s - 1 : 0);     // the row of its session; k_jsonl_expand maps it to the id
                }
            } else if (kind == JSONL_HEADER) {
                uint32_t o_sess = 0;
                reason = jsonl_parse_header(s_bytes, begin, n_local, &o_sess);
                if (row_s < cap_sessions) {
                    sess_id[row_s] = o_sess;
                    sess_off[row_s] = row_e;
                }
            } else {
                reason = jsonl_parse_lead(s_bytes, begin, n_local);
            }
            if (reason != JSONL_OK) {
                const unsigned long long line = (unsigned long long)(line0 + nl0 + (int64_t)((e >> 16) & 0xFFFFu) + 1);
                atomicMin(err, line << 8 | (unsigned long long)reason);
            }
        }
        __syncthreads();                                     // the list is rewritten in the next round
    }
    if (blockIdx.x == 0 && tid == 0) {
        const int64_t S = (int64_t)(scan_a[n_tiles] & 0xFFFFFFFFull);
        if (S <= cap_sessions) sess_off[S] = (int64_t)scan_b[n_tiles];
    }
}

__global__ __launch_bounds__(256) void k_jsonl_expand(uint32_t* __restrict__ session, const uint32_t* __restrict__ sess_id,
                                                      const uint64_t* __restrict__ scan_a, const uint64_t* __restrict__ scan_b,
                                                      int64_t n_tiles, int64_t cap_sessions, int64_t cap_events) {
    int64_t S = (int64_t)(scan_a[n_tiles] & 0xFFFFFFFFull), E = (int64_t)scan_b[n_tiles];
    if (S > cap_sessions) S = cap_sessions;
    if (E > cap_events) E = cap_events;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < E; i += (int64_t)gridDim.x * 256) {
        const uint32_t row = session[i];
        session[i] = (int64_t)row < S ? sess_id[row] : 0u;
    }
}

// the per-tile counts and their scans
static int jl_count_tiles(const uint8_t* d_bytes, int64_t n_bytes, const JsonlWs& w, hipStream_t s) {
    const int64_t nt = jl_tiles(n_bytes);
    k_jsonl_count<<<(unsigned)((nt + JL_THREADS / WAVE - 1) / (JL_THREADS / WAVE)), JL_THREADS, 0, s>>>(d_bytes, n_bytes, nt, w.cnt_a, w.cnt_b);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(LoadU64{w.cnt_a}, nt, w.scan_a, w.partial, s));
    OTTO_TRY(device_scan(LoadU64{w.cnt_b}, nt, w.scan_b, w.partial, s));
    return 0;
}

static int jl_check_args(const char* what, const uint8_t* d_bytes, int64_t n_bytes, const int64_t* h_counts, const void* d_work,
                         int64_t work_bytes) {
    OTTO_REQUIRE(h_counts, "%s: null h_counts", what);
    OTTO_REQUIRE(n_bytes >= 0 && n_bytes < (1ll << 31), "%s: n_bytes must be in [0, 2^31)", what);
    if (n_bytes == 0) return 0;
    OTTO_REQUIRE(d_bytes && d_work, "%s: null argument", what);
    OTTO_REQUIRE(((uintptr_t)d_bytes & 15) == 0, "%s: d_bytes must be 16-byte aligned", what);
    OTTO_REQUIRE(work_bytes >= otto_jsonl_workspace(n_bytes), "%s: workspace too small (%lld < %lld)", what, (long long)work_bytes,
                 (long long)otto_jsonl_workspace(n_bytes));
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_jsonl_workspace(int64_t n_bytes) {
    if (n_bytes <= 0) return 256;
    return (int64_t)jl_layout(n_bytes, nullptr, nullptr);
}

extern "C" int otto_jsonl_count(const uint8_t* d_bytes, int64_t n_bytes, int64_t* h_counts, void* d_work, int64_t work_bytes,
                                void* stream) {
    OTTO_TRY(jl_check_args("otto_jsonl_count", d_bytes, n_bytes, h_counts, d_work, work_bytes));
    h_counts[0] = h_counts[1] = 0;
    if (n_bytes == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    JsonlWs w;
    jl_layout(n_bytes, (char*)d_work, &w);
    OTTO_TRY(jl_count_tiles(d_bytes, n_bytes, w, s));
    const int64_t nt = jl_tiles(n_bytes);
    uint64_t h[2] = {0, 0};
    OTTO_HIP(hipMemcpyAsync(&h[0], w.scan_a + nt, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&h[1], w.scan_b + nt, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    h_counts[0] = (int64_t)(h[0] & 0xFFFFFFFFull);
    h_counts[1] = (int64_t)h[1];
    return 0;
}

extern "C" int otto_jsonl_parse(const uint8_t* d_bytes, int64_t n_bytes, int64_t line0, int64_t cap_sessions, int64_t cap_events,
                                uint32_t* d_session, uint32_t* d_aid, int64_t* d_ts, uint8_t* d_type, int64_t* d_sess_off,
                                uint32_t* d_sess_id, int64_t* h_counts, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_TRY(jl_check_args("otto_jsonl_parse", d_bytes, n_bytes, h_counts, d_work, work_bytes));
    OTTO_REQUIRE(d_sess_off, "otto_jsonl_parse: null d_sess_off");
    OTTO_REQUIRE(line0 >= 0 && line0 < (1ll << 54), "otto_jsonl_parse: line0 must be in [0, 2^54)");
    OTTO_REQUIRE(cap_sessions >= 0 && cap_events >= 0, "otto_jsonl_parse: negative capacity");
    hipStream_t s = (hipStream_t)stream;
    h_counts[0] = h_counts[1] = 0;
    if (n_bytes == 0) {
        OTTO_HIP(hipMemsetAsync(d_sess_off, 0, 8, s));
        return 0;
    }
    OTTO_REQUIRE(cap_sessions == 0 || d_sess_id, "otto_jsonl_parse: null d_sess_id");
    OTTO_REQUIRE(cap_events == 0 || (d_session && d_aid && d_ts && d_type), "otto_jsonl_parse: null event column");
    JsonlWs w;
    jl_layout(n_bytes, (char*)d_work, &w);
    const int64_t nt = jl_tiles(n_bytes);
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    OTTO_TRY(jl_count_tiles(d_bytes, n_bytes, w, s));
    k_jsonl_parse<<<(unsigned)nt, JL_THREADS, 0, s>>>(d_bytes, n_bytes, line0, w.scan_a, w.scan_b, nt, cap_sessions, cap_events,
                                                     d_session, d_aid, d_ts, d_type, d_sess_off, d_sess_id, w.err);
    OTTO_HIP(hipGetLastError());
    if (cap_events > 0) {
        const int64_t blocks = (cap_events + 255) / 256;
        k_jsonl_expand<<<(unsigned)(blocks < 256 * 16 ? blocks : 256 * 16), 256, 0, s>>>(d_session, d_sess_id, w.scan_a, w.scan_b, nt,
                                                                                       cap_sessions, cap_events);
        OTTO_HIP(hipGetLastError());
    }
    uint64_t h[2] = {0, 0};
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&h[0], w.scan_a + nt, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&h[1], w.scan_b + nt, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    h_counts[0] = (int64_t)(h[0] & 0xFFFFFFFFull);
    h_counts[1] = (int64_t)h[1];
    OTTO_REQUIRE(herr == ~0ull, "otto_jsonl_parse: line %llu: %s", herr >> 8, jsonl_reason((int)(herr & 0xFF)));
    OTTO_REQUIRE(h_counts[0] <= cap_sessions, "otto_jsonl_parse: %lld sessions, cap_sessions is %lld", (long long)h_counts[0],
                 (long long)cap_sessions);
    OTTO_REQUIRE(h_counts[1] <= cap_events, "otto_jsonl_parse: %lld events, cap_events is %lld", (long long)h_counts[1],
                 (long long)cap_events);
    return 0;
}

extern "C" int otto_jsonl_newlines(const void* d_work, int64_t work_bytes, int64_t n_bytes, int64_t* h_newlines, void* stream) {
    OTTO_REQUIRE(h_newlines, "otto_jsonl_newlines: null h_newlines");
    OTTO_REQUIRE(n_bytes >= 0 && n_bytes < (1ll << 31), "otto_jsonl_newlines: n_bytes must be in [0, 2^31)");
    *h_newlines = 0;
    if (n_bytes == 0) return 0;
    OTTO_REQUIRE(d_work && work_bytes >= otto_jsonl_workspace(n_bytes), "otto_jsonl_newlines: not the workspace of a call on %lld bytes",
                 (long long)n_bytes);
    hipStream_t s = (hipStream_t)stream;
    JsonlWs w;
    jl_layout(n_bytes, (char*)d_work, &w);
    uint64_t h = 0;
    OTTO_HIP(hipMemcpyAsync(&h, w.scan_a + jl_tiles(n_bytes), 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    *h_newlines = (int64_t)(h >> 32);
    return 0;
}
