// Device-side Snappy encoder for MI355X (gfx950): extents of a device buffer -> one Snappy raw-format stream each. C-ABI
// and SPEC-SNAPPY in include/otto_snappy.h. Reference code this replaces: the Snappy call inside
// pyarrow behind DataFrame.to_parquet of src/covisitation/covisitation.py and src/utilities/split_dataset_writer_parquet.py.
// Host restatement: tests/snappy_restatement.py.
//
// One wave owns a fragment (65,536 input bytes) in both kernels, so nothing but wave_lds_sync orders the LDS traffic.
//   k_snappy_plan   the match finder in batches of 64 positions (hash table of 4,096 positions in LDS; candidates at the
//                   distances 1, 4, 8 and the table's, the near ones out of the 16 bytes around the position), the greedy
//                   selection on ballot masks as in k_deflate_plan; literal tokens are joined into runs across batches, so
//                   the workspace holds ELEMENTS (a literal run or a copy, one word each) and the fragment's size
//   device_scan     (scan.h) over the fragment sizes, k_snappy_sizes -> the bytes of every stream
//   k_snappy_emit   64 elements per step: wave scans of their output and input sizes place them; tags and copies are byte
//                   stores of the owning lane, a literal longer than 16 bytes is copied by the whole wave
// The match finder is a sibling of k_deflate_plan's, not shared code: the candidates, the cap and the token form differ, and
// otto_deflate.hip stays byte for byte what it was.
#include <algorithm>
#include <vector>

#include "common.h"
#include "scan.h"
#include "wave.h"
#include "../../include/otto_snappy.h"

namespace otto {

constexpr int SN_FRAGMENT = OTTO_SNAPPY_FRAGMENT;
constexpr int SN_MIN_MATCH = OTTO_SNAPPY_MIN_MATCH;
constexpr int SN_HASH_BYTES = OTTO_SNAPPY_HASH_BYTES;
constexpr int SN_HASH_BITS = OTTO_SNAPPY_HASH_BITS;
constexpr int SN_MAX_MATCH = OTTO_SNAPPY_MAX_MATCH;
// a copy stands for at least MIN_MATCH bytes and a literal run follows a copy or starts the fragment
constexpr int SN_ELEMS = (2 * (SN_FRAGMENT / SN_MIN_MATCH) + 2 + 63) / 64 * 64;
constexpr int SN_SHORT_LITERAL = 16;                         // up to here the owning lane copies the bytes itself
constexpr unsigned long long SN_NO_ERR = ~0ull;
constexpr uint64_t SN_MAGIC = 0x31595050414E53ull;          // "SNAPPY1"
static_assert(OTTO_SNAPPY_BATCH == WAVE, "a batch of the match finder is one position per lane");
static_assert(SN_MIN_MATCH >= 4 && SN_HASH_BYTES >= 4 && SN_HASH_BYTES <= 8, "a copy is at least 4 bytes; the hash reads one 64-bit value");
static_assert(SN_MAX_MATCH == 64 && SN_FRAGMENT == 65536, "one copy element per match; 2-byte offsets");

struct SnFrag {
    uint64_t src;                 // of the fragment's first byte in d_in
    uint32_t m;                   // its bytes
    uint32_t stream;
};

struct SnHead {                   // the first 64 bytes of the workspace
    unsigned long long err;
    uint64_t magic, hash, n_frags, n_streams, pad[3];
};

struct SnWs {
    SnHead* head;
    uint64_t* off;                // [frags + 1] exclusive scan of size
    uint32_t* size;               // [frags] bytes of the fragment's elements, the stream's preamble with the first
    uint32_t* nelem;              // [frags]
    uint64_t* partial;
    SnFrag* frags;                // [frags]
    uint64_t* frag0;              // [streams + 1] the first fragment of a stream
    uint64_t* slen;               // [streams] the bytes of the extent
    uint64_t* sbytes;             // [streams] the bytes of the stream
    uint64_t* dst;                // [streams]
    uint32_t* elem;               // [frags * SN_ELEMS]
};

static size_t sn_layout(int64_t n_streams, int64_t n_frags, char* base, SnWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    SnWs t;
    t.head = (SnHead*)take(sizeof(SnHead));
    t.off = (uint64_t*)take((size_t)(n_frags + 1) * 8);
    t.size = (uint32_t*)take((size_t)n_frags * 4);
    t.nelem = (uint32_t*)take((size_t)n_frags * 4);
    t.partial = (uint64_t*)take(scan_partial_bytes(n_frags));
    t.frags = (SnFrag*)take((size_t)n_frags * sizeof(SnFrag));
    t.frag0 = (uint64_t*)take((size_t)(n_streams + 1) * 8);
    t.slen = (uint64_t*)take((size_t)n_streams * 8);
    t.sbytes = (uint64_t*)take((size_t)n_streams * 8);
    t.dst = (uint64_t*)take((size_t)n_streams * 8);
    t.elem = (uint32_t*)take((size_t)n_frags * SN_ELEMS * 4);
    if (w) *w = t;
    return o;
}

struct SnLoadSize {
    const uint32_t* a;
    __device__ uint64_t operator()(int64_t i) const { return a[i]; }
};

// an element: a literal run, len - 1; or a copy, bit 31 | distance << 8 | length - 1
__device__ __forceinline__ uint32_t sn_copy_elem(uint32_t length, uint32_t dist) { return 0x80000000u | dist << 8 | (length - 1u); }
__device__ __forceinline__ uint32_t sn_literal_head(uint32_t len) { return len <= 60u ? 1u : len <= 256u ? 2u : 3u; }
__device__ __forceinline__ uint32_t sn_copy_bytes(uint32_t length, uint32_t dist) { return length <= 11u && dist < 2048u ? 2u : 3u; }
__host__ __device__ __forceinline__ uint32_t sn_uleb_bytes(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80u) v >>= 7, ++n;
    return n;
}

// 8 bytes of x at any address, little-endian (gfx950 serves an unaligned global access)
__device__ __forceinline__ uint64_t sn_load8(const uint8_t* __restrict__ x) {
    uint64_t v;
    __builtin_memcpy(&v, x, 8);
    return v;
}
__device__ __forceinline__ void sn_store8(uint8_t* x, uint64_t v) { __builtin_memcpy(x, &v, 8); }

// number of leading bytes x[a ...] and x[b ...] share, at most limit; a < b and b + limit is inside the fragment
__device__ __forceinline__ uint32_t sn_common(const uint8_t* __restrict__ x, uint32_t a, uint32_t b, uint32_t limit) {
    uint32_t i = 0;
    for (; i + 8u <= limit; i += 8u) {
        const uint64_t d = sn_load8(x + a + i) ^ sn_load8(x + b + i);
        if (d) return i + ((uint32_t)__builtin_ctzll(d) >> 3);
    }
    while (i < limit && x[a + i] == x[b + i]) ++i;
    return i;
}

__global__ __launch_bounds__(WAVE) void k_snappy_plan(const uint8_t* __restrict__ in, const SnFrag* __restrict__ frags, const uint64_t* __restrict__ frag0,
                                                      const uint64_t* __restrict__ slen, uint32_t* __restrict__ elem_all, uint32_t* __restrict__ nelem_out,
                                                      uint32_t* __restrict__ size_out) {
    __shared__ uint32_t table[1 << SN_HASH_BITS];            // position + 1, 0 = empty
    const int lane = (int)lane_id();
    const int64_t f = blockIdx.x;
    const SnFrag fr = frags[f];
    const uint32_t m = fr.m;
    const uint8_t* __restrict__ x = in + fr.src;
    uint32_t* __restrict__ elem = elem_all + f * SN_ELEMS;
    const uint32_t preamble = frag0[fr.stream] == (uint64_t)f ? sn_uleb_bytes(slen[fr.stream]) : 0u;
    for (int i = lane; i < (1 << SN_HASH_BITS); i += WAVE) table[i] = 0;
    wave_lds_sync();

    uint32_t frontier = 0, nelem = 0, pending = 0, bytes = 0;    // pending: the literal run that reaches the batch's first position
#pragma unroll 1
    for (uint32_t base = 0; base < m; base += WAVE) {
        const uint32_t p = base + (uint32_t)lane;
        const bool valid = p < m, hashable = p + SN_HASH_BYTES <= m;
        uint32_t slot = 0, seen = 0;
        if (hashable) {
            uint64_t v = 0;
            if (p + 8u <= m) {
                v = sn_load8(x + p) & (~0ull >> (64 - 8 * SN_HASH_BYTES));
            } else {
#pragma unroll
                for (int i = 0; i < SN_HASH_BYTES; ++i) v |= (uint64_t)x[p + i] << (8 * i);
            }
            slot = (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - SN_HASH_BITS));
            seen = table[slot];
        }
        wave_lds_sync();
        if (hashable) atomicMax(&table[slot], p + 1u);
        wave_lds_sync();
        uint32_t mlen = 0, dist = 0;
        if (valid && p >= frontier) {
            const uint32_t limit = m - p < SN_MAX_MATCH ? m - p : SN_MAX_MATCH;
            // candidates in the order of the spec: a tie stays with the earlier one
            if (p >= 8u && limit >= 8u) {
                // the first 8 bytes of the three near candidates come out of the 16 bytes around p: two loads, not six
                const uint64_t hi = sn_load8(x + p), lo = sn_load8(x + p - 8u);
                auto candidate = [&](uint64_t first, uint32_t d) {
                    const uint64_t diff = first ^ hi;
                    const uint32_t l = diff ? (uint32_t)__builtin_ctzll(diff) >> 3 : 8u + sn_common(x + 8, p - d, p, limit - 8u);
                    if (l > mlen) mlen = l, dist = d;
                };
                candidate(lo >> 56 | hi << 8, 1u), candidate(lo >> 32 | hi << 32, 4u), candidate(lo, 8u);
                if (seen) candidate(sn_load8(x + seen - 1u), p - (seen - 1u));
            } else {                                         // the fragment's first 8 and last 7 positions
                auto candidate = [&](uint32_t d) {
                    if (p < d) return;
                    const uint32_t l = sn_common(x, p - d, p, limit);
                    if (l > mlen) mlen = l, dist = d;
                };
                candidate(1u), candidate(4u), candidate(8u);
                if (seen) candidate(p - (seen - 1u));
            }
            if (mlen < SN_MIN_MATCH) mlen = 0;
        }
        const uint64_t matches = __ballot(mlen > 0);
        const uint32_t nvalid = m - base < WAVE ? m - base : WAVE;
        uint32_t cur = frontier > base ? frontier - base : 0u;
        uint64_t reach = 0;                                  // the lanes a token starts at
        while (cur < nvalid) {
            const uint64_t from = ~0ull << cur;
            const uint64_t rest = matches & from;
            const uint32_t stop = rest ? (uint32_t)__builtin_ctzll(rest) : nvalid;      // literals in [cur, stop)
            const uint64_t below = stop >= 64u ? ~0ull : (1ull << stop) - 1ull;
            reach |= from & below;
            if (!rest) { cur = nvalid; break; }
            reach |= 1ull << stop;
            cur = stop + (uint32_t)__shfl((int)mlen, (int)stop, 64);
        }
        if (base + cur > frontier) frontier = base + cur;

        // tokens -> elements. A run of literal lanes that reaches the batch's last position stays pending.
        const uint64_t cop = reach & matches, lit = reach & ~matches;
        if (pending && !(lit & 1ull)) {                      // the run of the earlier batches ends at this batch's first token
            if (lane == 0) {
                elem[nelem] = pending - 1u;
                bytes += sn_literal_head(pending) + pending;
            }
            nelem += 1u;
            pending = 0;
        }
        const uint64_t starts = lit & ~(lit << 1), last = 1ull << (nvalid - 1u);
        const uint64_t ends = lit & ~(lit >> 1) & ~last;
        const uint64_t out = cop | ends;
        if ((out >> lane) & 1ull) {
            const uint32_t at = nelem + (uint32_t)__popcll(out & ((1ull << lane) - 1ull));
            if (mlen) {
                elem[at] = sn_copy_elem(mlen, dist);
                bytes += sn_copy_bytes(mlen, dist);
            } else {
                const uint32_t s = 63u - (uint32_t)__builtin_clzll(starts & (~0ull >> (63 - lane)));
                const uint32_t len = (uint32_t)lane - s + 1u + (s == 0u ? pending : 0u);
                elem[at] = len - 1u;
                bytes += sn_literal_head(len) + len;
            }
        }
        nelem += (uint32_t)__popcll(out);
        if (lit & last) {
            const uint32_t s = 63u - (uint32_t)__builtin_clzll(starts & (~0ull >> (64u - nvalid)));
            pending = nvalid - s + (s == 0u ? pending : 0u);
        } else {
            pending = 0;
        }
    }
    if (pending) {
        if (lane == 0) {
            elem[nelem] = pending - 1u;
            bytes += sn_literal_head(pending) + pending;
        }
        nelem += 1u;
    }
    bytes = wave_reduce<Sum>(bytes) + preamble;
    if (lane == 0) {
        nelem_out[f] = nelem;
        size_out[f] = bytes;
    }
}

__global__ void k_snappy_sizes(const uint64_t* __restrict__ off, const uint64_t* __restrict__ frag0, int64_t n_streams, uint64_t* __restrict__ sbytes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_streams) sbytes[i] = off[frag0[i + 1]] - off[frag0[i]];
}

// Every store of a fragment's wave lands in [lo, hi), a range inside the extent of its stream that the host has checked
// against out_bytes and the other streams: whatever the workspace holds, nothing else is written.
__global__ __launch_bounds__(WAVE) void k_snappy_emit(const uint8_t* __restrict__ in, const SnFrag* __restrict__ frags, const uint64_t* __restrict__ frag0,
                                                      const uint64_t* __restrict__ slen, const uint64_t* __restrict__ sbytes, const uint64_t* __restrict__ dst,
                                                      const uint64_t* __restrict__ off, const uint32_t* __restrict__ size_in,
                                                      const uint32_t* __restrict__ nelem_in, const uint32_t* __restrict__ elem_all, uint8_t* out,
                                                      unsigned long long* err) {
    const int lane = (int)lane_id();
    const int64_t f = blockIdx.x;
    const SnFrag fr = frags[f];
    const uint32_t m = fr.m;
    const uint8_t* __restrict__ x = in + fr.src;
    const uint32_t* __restrict__ elem = elem_all + f * SN_ELEMS;
    const uint64_t f0 = frag0[fr.stream], o_f = off[f], o_0 = off[f0];
    const uint32_t size = size_in[f], nelem = nelem_in[f];
    const bool first = f0 == (uint64_t)f;
    const uint64_t n = slen[fr.stream];
    const uint32_t preamble = first ? sn_uleb_bytes(n) : 0u;
    if (o_f < o_0 || o_f - o_0 > sbytes[fr.stream] || size > sbytes[fr.stream] - (o_f - o_0) || nelem > (uint32_t)SN_ELEMS || size < preamble) {
        if (lane == 0) atomicMin(err, (unsigned long long)f);
        return;
    }
    const uint64_t lo = dst[fr.stream] + (o_f - o_0), hi = lo + size;
    uint64_t o = lo;
    if (first) {
        if (lane < (int)preamble) out[o + lane] = (uint8_t)(((n >> (7 * lane)) & 0x7Fu) | (lane + 1 < (int)preamble ? 0x80u : 0u));
        o += preamble;
    }
    uint32_t ipos = 0;
#pragma unroll 1
    for (uint32_t e0 = 0; e0 < nelem; e0 += WAVE) {
        const bool have = e0 + (uint32_t)lane < nelem;
        const uint32_t e = have ? elem[e0 + lane] : 0u;
        const bool copy = e >> 31;
        uint32_t isz = 0, osz = 0, head = 0;
        if (have) {
            if (copy) {
                isz = (e & 63u) + 1u;
                head = osz = sn_copy_bytes(isz, (e >> 8) & 0xFFFFu);
            } else {
                isz = (e & 0xFFFFu) + 1u;
                head = sn_literal_head(isz);
                osz = head + isz;
            }
        }
        const uint32_t iin = wave_incl_scan<uint32_t>(isz), oin = wave_incl_scan<uint32_t>(osz);
        const uint32_t itot = (uint32_t)__shfl((int)iin, 63, 64), otot = (uint32_t)__shfl((int)oin, 63, 64);
        if (itot > m - ipos || otot > hi - o) {                   // uniform: a plan and an input that do not belong together
            if (lane == 0) atomicMin(err, (unsigned long long)f);
            return;
        }
        const uint32_t my_in = ipos + iin - isz;
        uint8_t* q = out + o + (oin - osz);
        if (have) {
            if (copy) {
                const uint32_t d = (e >> 8) & 0xFFFFu;
                if (head == 2u) {
                    q[0] = (uint8_t)(1u | (isz - 4u) << 2 | (d >> 8) << 5);
                    q[1] = (uint8_t)d;
                } else {
                    q[0] = (uint8_t)(2u | (isz - 1u) << 2);
                    q[1] = (uint8_t)d;
                    q[2] = (uint8_t)(d >> 8);
                }
            } else {
                if (head == 1u) {
                    q[0] = (uint8_t)((isz - 1u) << 2);
                } else if (head == 2u) {
                    q[0] = (uint8_t)(60u << 2);
                    q[1] = (uint8_t)(isz - 1u);
                } else {
                    q[0] = (uint8_t)(61u << 2);
                    q[1] = (uint8_t)(isz - 1u);
                    q[2] = (uint8_t)((isz - 1u) >> 8);
                }
                if (isz <= (uint32_t)SN_SHORT_LITERAL)
                    for (uint32_t i = 0; i < isz; ++i) q[head + i] = x[my_in + i];
            }
        }
        uint64_t wide = __ballot(have && !copy && isz > (uint32_t)SN_SHORT_LITERAL);
        while (wide) {                                       // one long literal at a time, by the whole wave
            const int l = __builtin_ctzll(wide);
            wide &= wide - 1ull;
            const uint32_t len = (uint32_t)__shfl((int)isz, l, 64), src = (uint32_t)__shfl((int)my_in, l, 64);
            const uint32_t rel = (uint32_t)__shfl((int)(oin - osz + head), l, 64);
            uint8_t* to = out + o + rel;
            const uint8_t* __restrict__ from = x + src;
            const uint32_t whole = len & ~7u;
            for (uint32_t i = (uint32_t)lane * 8u; i < whole; i += WAVE * 8u) sn_store8(to + i, sn_load8(from + i));
            for (uint32_t i = whole + (uint32_t)lane; i < len; i += WAVE) to[i] = from[i];
        }
        ipos += itot;
        o += otot;
    }
    if (lane == 0 && (ipos != m || o != hi)) atomicMin(err, (unsigned long long)f);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
struct SnPlan {
    std::vector<SnFrag> frags;
    std::vector<uint64_t> frag0, slen;
    uint64_t hash = 0;
};

static uint64_t sn_fnv(uint64_t h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

// every rule of the header that the host can check; the fragment table; the hash that ties a workspace to a job
static int sn_check(const char* what, const otto_snappy_job* job, SnPlan* plan) {
    OTTO_REQUIRE(job, "%s: null job", what);
    OTTO_REQUIRE(job->n_bytes >= 0 && (job->n_bytes == 0 || job->d_in), "%s: negative n_bytes or null d_in", what);
    OTTO_REQUIRE(job->n_streams >= 0 && (job->n_streams == 0 || (job->src_off && job->src_len)), "%s: negative n_streams or null extent arrays", what);
    plan->frag0.resize((size_t)job->n_streams + 1);
    plan->slen.resize((size_t)job->n_streams);
    for (int64_t i = 0; i < job->n_streams; ++i) {
        const int64_t o = job->src_off[i], n = job->src_len[i];
        OTTO_REQUIRE(n >= 0 && n < (1ll << 32), "%s: stream %lld: src_len %lld is not in [0, 2^32)", what, (long long)i, (long long)n);
        OTTO_REQUIRE(o >= 0 && o <= job->n_bytes && n <= job->n_bytes - o, "%s: stream %lld: source bytes [%lld, %lld) leave the input's %lld", what,
                     (long long)i, (long long)o, (long long)(o + n), (long long)job->n_bytes);
        plan->frag0[(size_t)i] = plan->frags.size();
        plan->slen[(size_t)i] = (uint64_t)n;
        int64_t at = 0;
        do {                                                 // an empty extent has one fragment of 0 bytes: it writes the preamble
            const int64_t m = n - at < SN_FRAGMENT ? n - at : SN_FRAGMENT;
            plan->frags.push_back(SnFrag{(uint64_t)(o + at), (uint32_t)m, (uint32_t)i});
            at += m;
        } while (at < n);
        OTTO_REQUIRE(plan->frags.size() < (1ull << 31) && i < (1ll << 32) - 1, "%s: more than 2^31 - 1 fragments", what);
    }
    plan->frag0[(size_t)job->n_streams] = plan->frags.size();
    uint64_t h = 0xCBF29CE484222325ull;
    h = sn_fnv(h, &job->d_in, sizeof(job->d_in));
    h = sn_fnv(h, &job->n_bytes, 8);
    h = sn_fnv(h, job->src_off, (size_t)job->n_streams * 8);
    h = sn_fnv(h, job->src_len, (size_t)job->n_streams * 8);
    plan->hash = h;
    return 0;
}

static int sn_check_work(const char* what, const otto_snappy_job* job, const SnPlan& plan, SnWs* w) {
    const int64_t need = (int64_t)sn_layout(job->n_streams, (int64_t)plan.frags.size(), nullptr, nullptr);
    OTTO_REQUIRE(job->d_work, "%s: null d_work", what);
    OTTO_REQUIRE(job->work_bytes >= need, "%s: workspace too small (%lld < %lld)", what, (long long)job->work_bytes, (long long)need);
    sn_layout(job->n_streams, (int64_t)plan.frags.size(), (char*)job->d_work, w);
    return 0;
}

static int sn_upload(const SnPlan& plan, const SnWs& w, hipStream_t s) {
    OTTO_HIP(hipMemcpyAsync(w.frags, plan.frags.data(), plan.frags.size() * sizeof(SnFrag), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.frag0, plan.frag0.data(), plan.frag0.size() * 8, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.slen, plan.slen.data(), plan.slen.size() * 8, hipMemcpyHostToDevice, s));
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_snappy_bound(int64_t n) { return n < 0 ? -1 : 32 + n + n / 6; }

extern "C" int64_t otto_snappy_workspace(const otto_snappy_job* job) {
    SnPlan plan;
    OTTO_TRY(sn_check("otto_snappy_workspace", job, &plan));
    return (int64_t)sn_layout(job->n_streams, (int64_t)plan.frags.size(), nullptr, nullptr);
}

extern "C" int otto_snappy_plan(const otto_snappy_job* job, int64_t* h_stream_bytes) {
    SnPlan plan;
    SnWs w;
    OTTO_TRY(sn_check("otto_snappy_plan", job, &plan));
    OTTO_REQUIRE(h_stream_bytes || job->n_streams == 0, "otto_snappy_plan: null h_stream_bytes");
    OTTO_TRY(sn_check_work("otto_snappy_plan", job, plan, &w));
    hipStream_t s = (hipStream_t)job->stream;
    const int64_t ns = job->n_streams, nf = (int64_t)plan.frags.size();
    SnHead head = {SN_NO_ERR, SN_MAGIC, plan.hash, (uint64_t)nf, (uint64_t)ns, {0, 0, 0}};
    OTTO_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, s));
    if (ns) {
        OTTO_TRY(sn_upload(plan, w, s));
        k_snappy_plan<<<(unsigned)nf, WAVE, 0, s>>>(job->d_in, w.frags, w.frag0, w.slen, w.elem, w.nelem, w.size);
        OTTO_HIP(hipGetLastError());
        OTTO_TRY(device_scan(SnLoadSize{w.size}, nf, w.off, w.partial, s));
        k_snappy_sizes<<<(unsigned)((ns + 255) / 256), 256, 0, s>>>(w.off, w.frag0, ns, w.sbytes);
        OTTO_HIP(hipGetLastError());
        static_assert(sizeof(int64_t) == sizeof(uint64_t), "");
        OTTO_HIP(hipMemcpyAsync(h_stream_bytes, w.sbytes, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
    }
    OTTO_HIP(hipStreamSynchronize(s));
    return 0;
}

extern "C" int otto_snappy_emit(const otto_snappy_job* job, const int64_t* h_dst_off, uint8_t* d_out, int64_t out_bytes) {
    SnPlan plan;
    SnWs w;
    OTTO_TRY(sn_check("otto_snappy_emit", job, &plan));
    OTTO_REQUIRE(h_dst_off || job->n_streams == 0, "otto_snappy_emit: null h_dst_off");
    OTTO_REQUIRE(out_bytes >= 0 && (d_out || out_bytes == 0), "otto_snappy_emit: null d_out or negative out_bytes");
    OTTO_TRY(sn_check_work("otto_snappy_emit", job, plan, &w));
    hipStream_t s = (hipStream_t)job->stream;
    const int64_t ns = job->n_streams, nf = (int64_t)plan.frags.size();
    SnHead head;
    std::vector<int64_t> bytes((size_t)ns);
    OTTO_HIP(hipMemcpyAsync(&head, w.head, sizeof(head), hipMemcpyDeviceToHost, s));
    if (ns) OTTO_HIP(hipMemcpyAsync(bytes.data(), w.sbytes, (size_t)ns * 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    const char* foreign = "otto_snappy_emit: the workspace does not hold the plan otto_snappy_plan wrote for this job";
    OTTO_REQUIRE(head.magic == SN_MAGIC && head.hash == plan.hash && head.n_frags == (uint64_t)nf && head.n_streams == (uint64_t)ns && head.err == SN_NO_ERR,
                 "%s", foreign);
    std::vector<int64_t> order((size_t)ns);
    for (int64_t i = 0; i < ns; ++i) {
        OTTO_REQUIRE(bytes[(size_t)i] >= 1 && bytes[(size_t)i] <= otto_snappy_bound(job->src_len[i]), "%s", foreign);
        OTTO_REQUIRE(h_dst_off[i] >= 0 && h_dst_off[i] <= out_bytes && bytes[(size_t)i] <= out_bytes - h_dst_off[i],
                     "otto_snappy_emit: stream %lld: bytes [%lld, %lld) leave out_bytes %lld; nothing written", (long long)i, (long long)h_dst_off[i],
                     (long long)(h_dst_off[i] + bytes[(size_t)i]), (long long)out_bytes);
        order[(size_t)i] = i;
    }
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return h_dst_off[a] < h_dst_off[b]; });
    for (size_t i = 1; i < order.size(); ++i) {
        const int64_t a = order[i - 1], b = order[i];
        OTTO_REQUIRE(h_dst_off[a] + bytes[(size_t)a] <= h_dst_off[b], "otto_snappy_emit: the extents of streams %lld and %lld overlap; nothing written",
                     (long long)a, (long long)b);
    }
    if (ns == 0) return 0;
    // the tables the kernel reads the input by come from the job again, and the checked sizes go back: a fragment's wave
    // stays inside its stream's checked extent whatever else the workspace holds
    OTTO_TRY(sn_upload(plan, w, s));
    OTTO_HIP(hipMemcpyAsync(w.sbytes, bytes.data(), (size_t)ns * 8, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.dst, h_dst_off, (size_t)ns * 8, hipMemcpyHostToDevice, s));
    k_snappy_emit<<<(unsigned)nf, WAVE, 0, s>>>(job->d_in, w.frags, w.frag0, w.slen, w.sbytes, w.dst, w.off, w.size, w.nelem, w.elem, d_out, &w.head->err);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = SN_NO_ERR;
    OTTO_HIP(hipMemcpyAsync(&herr, &w.head->err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != SN_NO_ERR) {
        OTTO_HIP(hipMemsetAsync(&w.head->err, 0xFF, 8, s));
        OTTO_HIP(hipStreamSynchronize(s));
        set_error("otto_snappy_emit: fragment %llu: the workspace does not hold the plan otto_snappy_plan wrote for this input", herr);
        return -22;
    }
    return 0;
}
