// The two ends of the output path for MI355X (gfx950): per-session top lists -> the bytes of the submission CSV, and event
// columns -> per-type aid counts and their top k. C-ABI and SPEC-SUBMIT in include/otto_submit.h.
// Reference code this replaces: the row loops + to_csv of src/ranker/inference.py:403-408,566-572 and
// src/covisitation/inference.py:387-391,437-447; src/baseline/frequency_statistics.py. Host restatement:
// tests/submit_restatement.py.
//
//   k_submit_len     one lane per (line, slot): branch-free digit counts, summed over the line's lanes -> len u32 [N]
//   device_scan      (scan.h) -> the int64 byte offset of every line, the total last
//   k_submit_format  one workgroup per OTTO_SUBMIT_LINES consecutive lines = one contiguous span of the output. A wave
//                    formats a line, lane j on item j (item 0 the session and its suffix, item j the aid j - 1); the in-line
//                    position is a wave prefix sum of digits + separator; the digits go into an LDS image of the span that
//                    is laid out like the output modulo 16. After one barrier the image goes out in whole aligned 16-byte
//                    words; only the partial words at the two ends of the span are stored by bytes, so a workgroup never
//                    stores a byte of a word that it does not own.
//   k_freq_count     one integer atomic per event
//   k_freq_partial   every wave keeps the sorted top 64 of its aids for the four rows (topk.h), k_freq_merge merges them
#include "common.h"
#include "scan.h"
#include "topk.h"
#include "wave.h"
#include "../../include/otto_submit.h"

namespace otto {

constexpr int SB_THREADS = 256;
constexpr int SB_WAVES = SB_THREADS / WAVE;
constexpr int SB_LINES = OTTO_SUBMIT_LINES;
constexpr int SB_MAX_K = OTTO_SUBMIT_MAX_K;
// longest line at k aids: session digits, "_orders,", per aid 10 digits and its separator; the longest span of a workgroup;
// the bytes of its LDS image (+ the span's offset inside its first 16-byte word). The image is dynamic LDS sized by k:
// 23,120 bytes at k = 64, 7,632 at k = 20, so that a small k is not held to the occupancy of the largest.
__host__ __device__ constexpr int sb_max_line(int k) { return 10 + 8 + 11 * k; }
__host__ __device__ constexpr int sb_span(int k) { return SB_LINES * sb_max_line(k); }
__host__ __device__ constexpr int sb_image(int k) { return (15 + sb_span(k) + 15) / 16 * 16; }
static_assert(sb_image(SB_MAX_K) <= 64 * 1024, "the image of the largest k fits the LDS a workgroup may take");
static_assert(SB_MAX_K <= WAVE, "one lane per aid; the session makes a second round at k = 64");
static_assert(SB_LINES % SB_WAVES == 0, "the waves of a workgroup take the same number of lines");
constexpr int SB_LPW = SB_LINES / SB_WAVES;                  // lines per wave
static_assert((SB_LPW & (SB_LPW - 1)) == 0 && SB_LPW <= WAVE, "lane m holds the metadata of the wave's m-th line");

// err word: the smallest (line << 2 | reason), ~0 without one
constexpr unsigned long long SB_NO_ERR = ~0ull;
constexpr unsigned long long SB_ERR_ROOM = ~0ull - 1;        // first_byte + total > out_bytes: no workgroup writes
enum { SB_BAD_CONTENT = 0, SB_BAD_OFFSETS = 1 };

// Host side only: the kernels take the members as parameters of their own (SB_PARAMS), since a struct argument whose
// members are selected by the table index is put into scratch.
struct SubmitTables {
    const int32_t *top0, *top1, *top2;
    const int32_t *n0, *n1, *n2;
    int32_t types;                // 2 bits per table
};

struct SubmitWs {
    unsigned long long* err;
    uint64_t* off;                // [N + 1] exclusive scan of len, the total last
    uint32_t* len;                // [N]
    uint64_t* partial;
};

static size_t sb_layout(int64_t N, char* base, SubmitWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    SubmitWs t;
    t.err = (unsigned long long*)take(8);
    t.off = (uint64_t*)take((size_t)(N + 1) * 8);
    t.len = (uint32_t*)take((size_t)N * 4);
    t.partial = (uint64_t*)take(scan_partial_bytes(N));
    if (w) *w = t;
    return o;
}

struct LoadU32 {
    const uint32_t* a;
    __device__ uint64_t operator()(int64_t i) const { return a[i]; }
};

// decimal digits of x, without a branch
__device__ __forceinline__ uint32_t dec_digits(uint32_t x) {
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
           (x >= 100000000u) + (x >= 1000000000u);
}

// "_clicks," / "_carts," / "_orders," : length, and the bytes packed little-endian
__device__ __forceinline__ uint32_t sfx_len(int c) { return c == 1 ? 7u : 8u; }
constexpr uint64_t pack8(const char* s) {
    uint64_t v = 0;
    for (int i = 0; i < 8 && s[i]; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
    return v;
}
__device__ __forceinline__ uint64_t sfx_bytes(int c) { return c == 0 ? pack8("_clicks,") : c == 1 ? pack8("_carts,") : pack8("_orders,"); }

// line index -> (session row, table)
__device__ __forceinline__ void sb_line(int64_t i, int64_t S, int T, int interleave, int64_t* s, int* t) {
    if (interleave) {
        const uint64_t q = T == 1 ? (uint64_t)i : T == 2 ? (uint64_t)i >> 1 : (uint64_t)i / 3u;
        *s = (int64_t)q;
        *t = (int)((uint64_t)i - q * (uint64_t)T);
    } else {
        *t = (int)(i >= S) + (int)(i >= 2 * S);
        *s = i - (int64_t)*t * S;
    }
}
#define SB_PARAMS const int32_t *__restrict__ top0, const int32_t *__restrict__ top1, const int32_t *__restrict__ top2, \
                  const int32_t *__restrict__ n0, const int32_t *__restrict__ n1, const int32_t *__restrict__ n2, int types
#define SB_ARGS(tb) (tb).top0, (tb).top1, (tb).top2, (tb).n0, (tb).n1, (tb).n2, (tb).types
__device__ __forceinline__ const int32_t* sb_pick(int t, const int32_t* p0, const int32_t* p1, const int32_t* p2) {
    return t == 0 ? p0 : t == 1 ? p1 : p2;
}
__device__ __forceinline__ int sb_type(int types, int t) { return (types >> (2 * t)) & 3; }

// kp = 1 << kp_log lanes per line, kp the power of two >= k: a line never straddles a wave. A thread takes SL_U lines, a
// workgroup step apart, and issues their loads together: with one line per thread the kernel waits out two dependent
// memory latencies (n, then the row) per wave and runs at a fraction of what the reads allow.
constexpr int SL_U = 4;
__global__ __launch_bounds__(SB_THREADS) void k_submit_len(SB_PARAMS, const int32_t* __restrict__ session_id, int64_t S, int T,
                                                           int k, int64_t ld, int interleave, int kp_log, int64_t N,
                                                           uint32_t* __restrict__ len, unsigned long long* err) {
    const int step = SB_THREADS >> kp_log;                   // lines a workgroup covers at once
    const int64_t first = (int64_t)blockIdx.x * step * SL_U + (threadIdx.x >> kp_log);
    const int j = (int)(threadIdx.x & ((1 << kp_log) - 1));
    int n[SL_U], t[SL_U];
    int64_t s[SL_U];
    int32_t a[SL_U], sid[SL_U];
#pragma unroll
    for (int u = 0; u < SL_U; ++u) {
        const int64_t i = first + (int64_t)u * step;
        n[u] = -1, t[u] = 0, s[u] = 0, sid[u] = 0;
        if (i < N) {
            sb_line(i, S, T, interleave, &s[u], &t[u]);
            n[u] = sb_pick(t[u], n0, n1, n2)[s[u]];
            if (j == 0) sid[u] = session_id[s[u]];
        }
    }
#pragma unroll
    for (int u = 0; u < SL_U; ++u) {
        a[u] = 0;
        if (j < n[u] && n[u] <= k) a[u] = sb_pick(t[u], top0, top1, top2)[s[u] * ld + j];
    }
#pragma unroll
    for (int u = 0; u < SL_U; ++u) {
        const int64_t i = first + (int64_t)u * step;
        uint32_t acc = 0;                                    // digits + separators in bits 0..15, violations above
        if (n[u] > k) acc = 1u << 16;
        else if (j < n[u]) acc = a[u] < 0 ? 1u << 16 : dec_digits((uint32_t)a[u]) + 1u;
        for (int d = 1; d < (1 << kp_log); d <<= 1) acc += (uint32_t)__shfl_xor((int)acc, d, 64);
        if (i < N && j == 0) {
            uint32_t L = 0;
            if (n[u] >= 0) {
                if (sid[u] < 0 || (acc >> 16)) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_CONTENT);
                else L = dec_digits((uint32_t)sid[u]) + sfx_len(sb_type(types, t[u])) + (acc & 0xFFFFu) + (n[u] == 0 ? 1u : 0u);
            }
            len[i] = L;
        }
    }
}

__global__ __launch_bounds__(SB_THREADS) void k_submit_format(SB_PARAMS, const int32_t* __restrict__ session_id, int64_t S, int T,
                                                              int k, int64_t ld, int interleave, int64_t N,
                                                              const uint64_t* __restrict__ off, uint8_t* __restrict__ out,
                                                              int64_t out_bytes, int64_t first_byte, unsigned long long* err) {
    extern __shared__ __attribute__((aligned(16))) uint8_t img[];        // sb_image(k) bytes
    const int tid = threadIdx.x, lane = (int)lane_id(), wave = tid >> 6;
    const int64_t line0 = (int64_t)blockIdx.x * SB_LINES;
    const int64_t line1 = line0 + SB_LINES < N ? line0 + SB_LINES : N;
    const uint64_t total = off[N], o_lo = off[line0], o_hi = off[line1];
    // Every store below lands in [first_byte + o_lo, first_byte + o_hi); these two refusals (uniform over the workgroup) keep
    // that inside [first_byte, first_byte + total) and inside the buffer and the image, whatever the workspace holds.
    if (!(total <= (uint64_t)out_bytes && (uint64_t)first_byte <= (uint64_t)out_bytes - total)) {
        if (tid == 0) atomicMin(err, SB_ERR_ROOM);
        return;
    }
    if (!(o_lo <= o_hi && o_hi <= total && o_hi - o_lo <= (uint64_t)sb_span(k))) {
        if (tid == 0) atomicMin(err, (unsigned long long)line0 << 2 | SB_BAD_OFFSETS);
        return;
    }
    const uint64_t g_lo = (uint64_t)first_byte + o_lo, g_hi = (uint64_t)first_byte + o_hi;
    const int a0 = (int)(g_lo & 15u);                        // image byte p is output byte g_lo - a0 + p
    // The wave's SB_LPW lines are line0 + wave + m * SB_WAVES. Lane m loads the metadata of line m, then every lane loads
    // its first-round item of all of them: two memory latencies for the wave, not three per line.
    uint64_t m_lo = 0, m_hi = 0;
    int m_n = -1;
    int32_t m_sid = 0;
    {
        const int64_t mi = line0 + wave + (int64_t)(lane & (SB_LPW - 1)) * SB_WAVES;
        if (mi < line1) {
            int64_t s;
            int t;
            sb_line(mi, S, T, interleave, &s, &t);
            m_lo = off[mi], m_hi = off[mi + 1];
            m_n = sb_pick(t, n0, n1, n2)[s];
            m_sid = session_id[s];
        }
    }
    int32_t first_item[SB_LPW];
#pragma unroll
    for (int m = 0; m < SB_LPW; ++m) {
        const int64_t i = line0 + wave + (int64_t)m * SB_WAVES;
        const int n = __shfl(m_n, m, 64);
        const int32_t sid = __shfl(m_sid, m, 64);            // by every lane: a shuffle under `lane == 0` reads an idle lane
        first_item[m] = lane == 0 ? sid : 0;
        if (i < line1 && lane >= 1 && lane <= n && n <= k) {
            int64_t s;
            int t;
            sb_line(i, S, T, interleave, &s, &t);
            first_item[m] = sb_pick(t, top0, top1, top2)[s * ld + lane - 1];
        }
    }
#pragma unroll
    for (int m = 0; m < SB_LPW; ++m) {
        const int64_t i = line0 + wave + (int64_t)m * SB_WAVES;
        if (i >= line1) break;
        const uint64_t lo = __shfl((unsigned long long)m_lo, m, 64), hi = __shfl((unsigned long long)m_hi, m, 64);
        if (!(o_lo <= lo && lo <= hi && hi <= o_hi)) {
            if (lane == 0) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_OFFSETS);
            continue;
        }
        const uint32_t want = (uint32_t)(hi - lo);
        uint8_t* line = img + a0 + (int)(lo - o_lo);
        int64_t s;
        int t;
        sb_line(i, S, T, interleave, &s, &t);
        const int n = __shfl(m_n, m, 64);
        if (n < 0) {
            if (want != 0 && lane == 0) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_OFFSETS);
            continue;
        }
        const int32_t sid = __shfl(m_sid, m, 64);
        if (n > k || sid < 0) {
            if (lane == 0) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_CONTENT);
            continue;
        }
        const int c = sb_type(types, t);
        const int32_t* row = sb_pick(t, top0, top1, top2) + s * ld;
        const int items = n + 1;                             // the session, then the aids
        uint32_t run = 0;
        bool negative = false;
#pragma unroll 1
        for (int base = 0; base < items; base += WAVE) {     // a second round only at n = 64
            const int q = base + lane;
            const bool act = q < items;
            int32_t a = 0;
            if (act) a = base == 0 ? first_item[m] : row[q - 1];
            if (__any(a < 0)) { negative = true; break; }
            uint32_t x = (uint32_t)a, d = 0, tail = 0;
            if (act) {
                d = dec_digits(x);
                tail = q == 0 ? sfx_len(c) + (n == 0 ? 1u : 0u) : 1u;
            }
            const uint32_t item = d + tail;
            const uint32_t incl = wave_incl_scan<uint32_t>(item);
            const uint32_t at = run + incl - item;
            run += (uint32_t)__shfl((int)incl, 63, 64);
            const bool put = act && at + item <= want;       // never past the line's own bytes, whatever the offsets say
            uint8_t* p = line + at;
#pragma unroll
            for (int e = 0; e < 10; ++e) {                   // as many steps as the longest number of the round has digits
                if (__ballot(put && (uint32_t)e < d) == 0) break;
                if (put && (uint32_t)e < d) {
                    const uint32_t q10 = __umulhi(x, 0xCCCCCCCDu) >> 3;
                    p[d - 1 - e] = (uint8_t)('0' + (x - q10 * 10u));
                    x = q10;
                }
            }
            if (put && q != 0) p[d] = q == n ? (uint8_t)'\n' : (uint8_t)' ';
            if (base == 0) {                                 // the session's suffix, comma (and newline at n == 0): a byte per lane
                const uint32_t ds = dec_digits((uint32_t)sid), sl = sfx_len(c), tail0 = sl + (n == 0 ? 1u : 0u);
                if ((uint32_t)lane < tail0 && ds + tail0 <= want)
                    line[ds + lane] = (uint32_t)lane < sl ? (uint8_t)(sfx_bytes(c) >> (8 * (lane & 7))) : (uint8_t)'\n';
            }
        }
        if (lane == 0) {
            if (negative) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_CONTENT);
            else if (run != want) atomicMin(err, (unsigned long long)i << 2 | SB_BAD_OFFSETS);
        }
    }
    __syncthreads();
    const uint64_t g_base = g_lo - (uint64_t)a0;
    const uint64_t w_lo = (g_lo + 15u) & ~(uint64_t)15, w_hi = g_hi & ~(uint64_t)15;
    if (w_lo <= w_hi) {
        if ((uint64_t)tid < w_lo - g_lo) out[g_lo + tid] = img[a0 + tid];
        for (uint64_t w = w_lo + (uint64_t)tid * 16u; w < w_hi; w += (uint64_t)SB_THREADS * 16u)
            *reinterpret_cast<uint4*>(out + w) = *reinterpret_cast<const uint4*>(img + (w - g_base));
        if ((uint64_t)tid < g_hi - w_hi) out[w_hi + tid] = img[(w_hi - g_base) + tid];
    } else if ((uint64_t)tid < g_hi - g_lo) {                // a span inside one word that it does not fill
        out[g_lo + tid] = img[a0 + tid];
    }
}

// ---- most frequent aids ------------------------------------------------------------------------------------------------
constexpr int FQ_THREADS = 256;
constexpr int FQ_TOPK_BLOCKS = 256;                          // grid cap of k_freq_partial: 1024 partial lists

__global__ __launch_bounds__(FQ_THREADS) void k_freq_count(const uint32_t* __restrict__ aid, const uint8_t* __restrict__ type, int64_t E,
                                                           uint64_t n_aids, uint32_t* count, unsigned long long* err) {
    for (int64_t i = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; i < E; i += (int64_t)gridDim.x * FQ_THREADS) {
        const uint32_t a = aid[i];
        const uint32_t t = type[i];
        if (a >= n_aids || t > 2u) atomicMin(err, (unsigned long long)i);
        else atomicAdd(count + (uint64_t)t * n_aids + a, 1u);
    }
}

// partial lists: [list][row][lane] of (count u64, aid u32), sorted best first, count 0 = empty
__global__ __launch_bounds__(FQ_THREADS) void k_freq_partial(const uint32_t* __restrict__ count, int64_t n_aids, int k,
                                                             uint64_t* __restrict__ pw, uint32_t* __restrict__ py) {
    const int lane = (int)lane_id();
    const int64_t list = (int64_t)blockIdx.x * (FQ_THREADS / WAVE) + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * FQ_THREADS;
    KeyW best[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) kclear(best[r]);
#pragma unroll 1
    for (int64_t base = list * WAVE; base < n_aids; base += stride) {
        const int64_t i = base + lane;
        uint32_t c0 = 0, c1 = 0, c2 = 0;
        if (i < n_aids) {
            c0 = count[i];
            c1 = count[n_aids + i];
            c2 = count[2 * n_aids + i];
        }
        const uint64_t w[4] = {(uint64_t)c0 + c1 + c2, c0, c1, c2};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            KeyW c = {w[r], (uint32_t)i};
            if (!w[r]) kclear(c);
            wave_topk_push(best[r], c, k);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pw[(list * 4 + r) * WAVE + lane] = best[r].w;
        py[(list * 4 + r) * WAVE + lane] = best[r].y;
    }
}

// wave r merges row r of every partial list
__global__ __launch_bounds__(FQ_THREADS) void k_freq_merge(const uint64_t* __restrict__ pw, const uint32_t* __restrict__ py, int64_t lists,
                                                           int k, int32_t* __restrict__ top_aid, int64_t* __restrict__ top_count,
                                                           int32_t* __restrict__ n_out) {
    const int lane = (int)lane_id(), r = threadIdx.x >> 6;
    KeyW best;
    kclear(best);
#pragma unroll 1
    for (int64_t p = 0; p < lists; ++p) {
        KeyW c;
        kload(c, pw[(p * 4 + r) * WAVE + lane], py[(p * 4 + r) * WAVE + lane]);
        wave_topk_push(best, c, k);
    }
    const bool valid = lane < k && kvalid(best);
    const uint64_t m = __ballot(valid);
    if (lane < k) {
        top_aid[r * k + lane] = valid ? (int32_t)best.y : -1;
        top_count[r * k + lane] = valid ? (int64_t)best.w : 0;
    }
    if (lane == 0) n_out[r] = __popcll(m);
}

static int64_t fq_lists(int64_t n_aids) {
    const int64_t blocks = (n_aids + FQ_THREADS - 1) / FQ_THREADS;
    return (blocks < FQ_TOPK_BLOCKS ? blocks : FQ_TOPK_BLOCKS) * (FQ_THREADS / WAVE);
}

static int sb_check_args(const char* what, int32_t T, const int32_t* const* h_d_top_aid, const int32_t* const* h_d_n, const int32_t* h_type,
                         const int32_t* d_session_id, int64_t S, int32_t k, int64_t ld, const void* d_work, int64_t work_bytes,
                         SubmitTables* tb) {
    OTTO_REQUIRE(T >= 1 && T <= OTTO_SUBMIT_MAX_TABLES, "%s: T must be in [1, %d] (got %d)", what, OTTO_SUBMIT_MAX_TABLES, T);
    OTTO_REQUIRE(S >= 0 && S < (1ll << 31), "%s: S must be in [0, 2^31)", what);
    OTTO_REQUIRE(k >= 1 && k <= SB_MAX_K, "%s: k must be in [1, %d] (got %d)", what, SB_MAX_K, k);
    OTTO_REQUIRE(ld >= k && ld < (1ll << 31), "%s: ld must be in [k, 2^31)", what);
    OTTO_REQUIRE(h_d_top_aid && h_d_n && h_type, "%s: null table list", what);
    tb->types = 0;
    for (int t = 0; t < T; ++t) {
        OTTO_REQUIRE(h_type[t] >= 0 && h_type[t] <= 2, "%s: type code of table %d must be 0, 1 or 2 (got %d)", what, t, h_type[t]);
        OTTO_REQUIRE(S == 0 || (h_d_top_aid[t] && h_d_n[t]), "%s: null column of table %d", what, t);
        tb->types |= h_type[t] << (2 * t);
    }
    tb->top0 = h_d_top_aid[0], tb->n0 = h_d_n[0];                // tables past T are never selected
    tb->top1 = h_d_top_aid[T > 1 ? 1 : 0], tb->n1 = h_d_n[T > 1 ? 1 : 0];
    tb->top2 = h_d_top_aid[T > 2 ? 2 : 0], tb->n2 = h_d_n[T > 2 ? 2 : 0];
    if (S == 0) return 0;
    OTTO_REQUIRE(d_session_id && d_work, "%s: null argument", what);
    OTTO_REQUIRE(work_bytes >= otto_submit_workspace(S, T), "%s: workspace too small (%lld < %lld)", what, (long long)work_bytes,
                 (long long)otto_submit_workspace(S, T));
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_submit_workspace(int64_t S, int32_t T) {
    if (S <= 0 || T < 1 || T > OTTO_SUBMIT_MAX_TABLES) return 256;
    return (int64_t)sb_layout(S * T, nullptr, nullptr);
}

extern "C" int otto_submit_measure(int32_t T, const int32_t* const* h_d_top_aid, const int32_t* const* h_d_n, const int32_t* h_type,
                                   const int32_t* d_session_id, int64_t S, int32_t k, int64_t ld, int32_t interleave, int64_t* h_bytes,
                                   void* d_work, int64_t work_bytes, void* stream) {
    SubmitTables tb;
    OTTO_REQUIRE(h_bytes, "otto_submit_measure: null h_bytes");
    *h_bytes = 0;
    OTTO_TRY(sb_check_args("otto_submit_measure", T, h_d_top_aid, h_d_n, h_type, d_session_id, S, k, ld, d_work, work_bytes, &tb));
    if (S == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = S * T;
    SubmitWs w;
    sb_layout(N, (char*)d_work, &w);
    int kp_log = 0;
    while ((1 << kp_log) < k) ++kp_log;
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    const int64_t lines_per_block = (int64_t)(SB_THREADS >> kp_log) * SL_U;
    k_submit_len<<<(unsigned)((N + lines_per_block - 1) / lines_per_block), SB_THREADS, 0, s>>>(SB_ARGS(tb), d_session_id, S, T, k, ld, interleave,
                                                                                                 kp_log, N, w.len, w.err);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(LoadU32{w.len}, N, w.off, w.partial, s));
    unsigned long long herr = 0;
    uint64_t total = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&total, w.off + N, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(herr == SB_NO_ERR, "otto_submit_measure: line %llu: n > k, a negative session id or a negative aid among the first n",
                 herr >> 2);
    *h_bytes = (int64_t)total;
    return 0;
}

extern "C" int otto_submit_format(int32_t T, const int32_t* const* h_d_top_aid, const int32_t* const* h_d_n, const int32_t* h_type,
                                  const int32_t* d_session_id, int64_t S, int32_t k, int64_t ld, int32_t interleave, uint8_t* d_out,
                                  int64_t out_bytes, int64_t first_byte, void* d_work, int64_t work_bytes, void* stream) {
    SubmitTables tb;
    OTTO_TRY(sb_check_args("otto_submit_format", T, h_d_top_aid, h_d_n, h_type, d_session_id, S, k, ld, d_work, work_bytes, &tb));
    OTTO_REQUIRE(out_bytes >= 0 && first_byte >= 0, "otto_submit_format: negative out_bytes or first_byte");
    OTTO_REQUIRE(first_byte <= out_bytes, "otto_submit_format: first_byte %lld is past out_bytes %lld", (long long)first_byte,
                 (long long)out_bytes);
    if (S == 0) return 0;
    OTTO_REQUIRE(d_out, "otto_submit_format: null d_out");
    OTTO_REQUIRE(((uintptr_t)d_out & 15) == 0, "otto_submit_format: d_out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = S * T;
    SubmitWs w;
    sb_layout(N, (char*)d_work, &w);
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    k_submit_format<<<(unsigned)((N + SB_LINES - 1) / SB_LINES), SB_THREADS, (size_t)sb_image(k), s>>>(SB_ARGS(tb), d_session_id, S, T, k, ld, interleave, N, w.off,
                                                                                      d_out, out_bytes, first_byte, w.err);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = 0;
    uint64_t total = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&total, w.off + N, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(herr != SB_ERR_ROOM, "otto_submit_format: first_byte %lld + %llu bytes of lines do not fit out_bytes %lld; nothing written",
                 (long long)first_byte, (unsigned long long)total, (long long)out_bytes);
    OTTO_REQUIRE(herr == SB_NO_ERR || (herr & 3) != SB_BAD_OFFSETS,
                 "otto_submit_format: line %llu: the workspace does not hold the offsets otto_submit_measure wrote for these inputs", herr >> 2);
    OTTO_REQUIRE(herr == SB_NO_ERR, "otto_submit_format: line %llu: n > k, a negative session id or a negative aid among the first n",
                 herr >> 2);
    return 0;
}

extern "C" int otto_freq_count(const uint32_t* d_aid, const uint8_t* d_type, int64_t E, int64_t n_aids, uint32_t* d_count, void* stream) {
    OTTO_REQUIRE(E >= 0, "otto_freq_count: negative E");
    OTTO_REQUIRE(n_aids >= 1 && n_aids < (1ll << 31), "otto_freq_count: n_aids must be in [1, 2^31)");
    if (E == 0) return 0;
    OTTO_REQUIRE(d_aid && d_type && d_count, "otto_freq_count: null argument");
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_FREQ, 256, &scratch, s));
    unsigned long long* err = (unsigned long long*)scratch;
    OTTO_HIP(hipMemsetAsync(err, 0xFF, 8, s));
    const int64_t blocks = (E + FQ_THREADS - 1) / FQ_THREADS;
    k_freq_count<<<(unsigned)(blocks < 256 * 16 ? blocks : 256 * 16), FQ_THREADS, 0, s>>>(d_aid, d_type, E, (uint64_t)n_aids, d_count, err);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(herr == ~0ull, "otto_freq_count: event %llu: aid >= n_aids (%lld) or type > 2", herr, (long long)n_aids);
    return 0;
}

extern "C" int otto_freq_topk(const uint32_t* d_count, int64_t n_aids, int32_t k, int32_t* d_top_aid, int64_t* d_top_count, int32_t* d_n,
                              void* stream) {
    OTTO_REQUIRE(n_aids >= 1 && n_aids < (1ll << 31), "otto_freq_topk: n_aids must be in [1, 2^31)");
    OTTO_REQUIRE(k >= 1 && k <= SB_MAX_K, "otto_freq_topk: k must be in [1, %d] (got %d)", SB_MAX_K, k);
    OTTO_REQUIRE(d_count && d_top_aid && d_top_count && d_n, "otto_freq_topk: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t lists = fq_lists(n_aids);
    const size_t pw_bytes = align256((size_t)lists * 4 * WAVE * 8), py_bytes = align256((size_t)lists * 4 * WAVE * 4);
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_FREQ, 256 + pw_bytes + py_bytes, &scratch, s));
    uint64_t* pw = (uint64_t*)((char*)scratch + 256);
    uint32_t* py = (uint32_t*)((char*)scratch + 256 + pw_bytes);
    k_freq_partial<<<(unsigned)(lists / (FQ_THREADS / WAVE)), FQ_THREADS, 0, s>>>(d_count, n_aids, k, pw, py);
    OTTO_HIP(hipGetLastError());
    k_freq_merge<<<1, FQ_THREADS, 0, s>>>(pw, py, lists, k, d_top_aid, d_top_count, d_n);
    OTTO_HIP(hipGetLastError());
    return 0;
}
