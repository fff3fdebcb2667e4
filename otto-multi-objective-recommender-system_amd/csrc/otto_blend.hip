// Robust scaling and outer-join blend of ranker scores (SPEC-BLEND; include/otto_blend.h).
//
// Device, on the caller's stream:
//   k_sel_hist / k_sel_pick   most-significant-digit radix SELECT (not a sort) of up to six order statistics of a
//                    float64 column: eight 8-bit digits of the order-preserving 64-bit image of the double (-0.0 folded
//                    onto +0.0; NaN excluded and counted, +-inf flagged in the first pass). A pass reads x once, counts
//                    the current digit of the values that still match one of the ranks' prefixes in per-workgroup LDS
//                    histograms (one per DISTINCT prefix: ranks that still share a prefix share a histogram) and merges
//                    them with global atomics; k_sel_pick (one workgroup) then moves every rank one digit down. x is
//                    never written. A full sort of the column was not built: it would move 16 n bytes per pass where the
//                    select reads 8 n, and needs 16 n bytes of workspace where the select needs 100 KB.
//   k_blend_scale    (float)((x - center) / scale): a true float64 division, then one rounding.
//   k_join_keys      (session << 32 | aid, score, model) rows of all models, concatenated in model order; negative ids
//                    counted; OR and AND of the keys (which digits vary at all).
//   k_rs_hist / k_rs_scatter  the shared stable LSD radix sort (radix.h) of those rows by key, carrying the model as its
//                    byte column. A digit that is constant over the input turns its pass into a plain copy, decided on the
//                    device, so the host needs no read-back before the passes. The sort is stable and the input is in
//                    model order, so the rows of one key come out in ascending model order.
//   k_join_mark      group heads (first row of a key) that own an output row: some un-flagged model is present. Two
//                    adjacent rows with one key and one model are a duplicate key inside that model.
//   k_join_emit      one lane per output row walks its group's <= M rows straight from global memory -- bounded by n
//                    and by M, not by the workgroup's tile, which is how a group that straddles a tile edge is handled
//                    -- applies left_of_base and writes aid, pred, (double)pred and the row's session.
//   k_join_sessions  CSR of the output's sessions from a second scan (over the output rows).
// The prediction rounds every product and every sum to float32 on its own. Contraction is switched OFF for k_join_emit
// (#pragma clang fp contract(off) in its body) and the sum is written with plain * and +: HIP's __fmul_rn / __fadd_rn are
// plain operators in the headers, and hipcc, which contracts a * b + c by default, fuses them like any other.
#include "common.h"
#include "radix.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_blend.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

namespace otto {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// radix select
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SEL_RANKS = 6;
constexpr int SEL_PASSES = 8;
constexpr int SEL_THREADS = 256;
constexpr int SEL_MAX_GRID = 256 * 8;

struct SelResult {                                          // what the host reads back
    unsigned long long n_nan;
    long long nv;
    double stats[SEL_RANKS];
    unsigned int has_inf, pad;
};

struct SelState {
    unsigned long long hist[SEL_PASSES][SEL_RANKS][256];   // per pass: one histogram per distinct prefix
    unsigned long long prefix[SEL_RANKS];                   // digits fixed so far, per rank
    unsigned long long rank[SEL_RANKS];                     // rank among the values that share the prefix
    unsigned long long uprefix[SEL_RANKS];                  // the distinct prefixes
    int slot[SEL_RANKS];                                    // rank -> index into uprefix
    int nuniq;
    SelResult res;
};

template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void k_sel_hist(const double* __restrict__ x, int64_t n, int pass, SelState* st) {
    __shared__ uint32_t s_h[SEL_RANKS * 256];
    __shared__ unsigned long long s_up[SEL_RANKS];
    const int shift = 56 - 8 * pass;
    const int nu = FIRST ? 1 : st->nuniq;
    for (int i = threadIdx.x; i < nu * 256; i += SEL_THREADS) s_h[i] = 0;
    if (!FIRST && (int)threadIdx.x < nu) s_up[threadIdx.x] = st->uprefix[threadIdx.x];
    __syncthreads();
    unsigned long long nan = 0;
    bool inf = false;
    for (int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEL_THREADS) {
        const double v = x[i];
        if (v != v) { ++nan; continue; }
        const uint64_t k = ordered_key(v);
        if (FIRST) {
            inf |= (v == INFINITY || v == -INFINITY);
            atomicAdd(&s_h[k >> 56], 1u);
        } else {
            for (int u = 0; u < nu; ++u)
                if (((k ^ s_up[u]) >> (shift + 8)) == 0) {        // distinct prefixes: at most one matches
                    atomicAdd(&s_h[u * 256 + (int)((k >> shift) & 255u)], 1u);
                    break;
                }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nu * 256; i += SEL_THREADS) {
        const uint32_t c = s_h[i];
        if (c) atomicAdd(&st->hist[pass][i >> 8][i & 255], (unsigned long long)c);
    }
    if (FIRST) {
        nan = wave_reduce<Sum>(nan);
        if (lane_id() == 0 && nan) atomicAdd(&st->res.n_nan, nan);
        if (inf) atomicOr(&st->res.has_inf, 1u);
    }
}

// one workgroup: every rank moves one digit down
__global__ __launch_bounds__(SEL_THREADS) void k_sel_pick(SelState* st, int64_t n, int pass) {
    __shared__ unsigned long long sm[SEL_THREADS / 64 + 1];
    __shared__ unsigned long long s_pref[SEL_RANKS], s_rank[SEL_RANKS], s_npref[SEL_RANKS], s_nrank[SEL_RANKS];
    __shared__ int s_slot[SEL_RANKS], s_nu;
    const int shift = 56 - 8 * pass;
    if (threadIdx.x == 0) {
        if (pass == 0) {
            const long long nv = (long long)n - (long long)st->res.n_nan;
            st->res.nv = nv;
            const unsigned long long m1 = nv > 0 ? (unsigned long long)(nv - 1) : 0ull;
            unsigned long long r[SEL_RANKS];
            r[0] = m1 >> 1;                       // v[(nv-1)>>1]
            r[1] = (unsigned long long)(nv > 0 ? nv : 0) >> 1;
            r[2] = m1 >> 2;
            r[3] = r[2] + 1 < m1 ? r[2] + 1 : m1;
            r[4] = (3ull * m1) >> 2;
            r[5] = r[4] + 1 < m1 ? r[4] + 1 : m1;
            for (int q = 0; q < SEL_RANKS; ++q) { s_pref[q] = 0; s_rank[q] = r[q]; s_slot[q] = 0; }
            s_nu = 1;
        } else {
            for (int q = 0; q < SEL_RANKS; ++q) { s_pref[q] = st->prefix[q]; s_rank[q] = st->rank[q]; s_slot[q] = st->slot[q]; }
            s_nu = st->nuniq;
        }
        for (int q = 0; q < SEL_RANKS; ++q) { s_npref[q] = s_pref[q]; s_nrank[q] = 0; }
    }
    __syncthreads();
    const int nu = s_nu;
    for (int u = 0; u < nu; ++u) {
        const unsigned long long cnt = st->hist[pass][u][threadIdx.x];
        unsigned long long tot;
        const unsigned long long ex = block_excl_scan<unsigned long long, SEL_THREADS>(cnt, sm, &tot);
#pragma unroll
        for (int q = 0; q < SEL_RANKS; ++q)
            if (s_slot[q] == u && s_rank[q] >= ex && s_rank[q] < ex + cnt) {      // exactly one thread when nv > 0
                s_npref[q] = s_pref[q] | ((unsigned long long)threadIdx.x << shift);
                s_nrank[q] = s_rank[q] - ex;
            }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nuq = 0;
        for (int q = 0; q < SEL_RANKS; ++q) {
            st->prefix[q] = s_npref[q];
            st->rank[q] = s_nrank[q];
            int u = 0;
            while (u < nuq && st->uprefix[u] != s_npref[q]) ++u;
            if (u == nuq) st->uprefix[nuq++] = s_npref[q];
            st->slot[q] = u;
            if (pass == SEL_PASSES - 1) st->res.stats[q] = ordered_key_inv((uint64_t)s_npref[q]);
        }
        st->nuniq = nuq;
    }
}

__global__ __launch_bounds__(256) void k_blend_scale(const double* __restrict__ x, int64_t n, double center, double scale,
                                                     float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = (float)((x[i] - center) / scale);
}

// ---------------------------------------------------------------------------------------------------------------------
// join
// ---------------------------------------------------------------------------------------------------------------------
struct JoinArgs {
    const int32_t* session[OTTO_BLEND_MAX_MODELS];
    const int32_t* aid[OTTO_BLEND_MAX_MODELS];
    const float* score[OTTO_BLEND_MAX_MODELS];
    int64_t off[OTTO_BLEND_MAX_MODELS + 1];          // first row of model m in the concatenation
    float w[OTTO_BLEND_MAX_MODELS];
    uint32_t flagged;                                // bit m: model m is left_of_base
    int M;
};

// per-device scratch of the join: counts, error words, key bits
struct JoinScratch {
    unsigned long long n_out, n_sessions;
    unsigned long long key_bits[2];                  // OR and AND of the keys (key_bits_fold)
    unsigned int n_negative, n_duplicate;
};

__global__ __launch_bounds__(256) void k_join_keys(JoinArgs a, uint64_t* key, uint32_t* val, uint8_t* mod, JoinScratch* sc) {
    const int m = blockIdx.y;
    const int64_t nm = a.off[m + 1] - a.off[m];
    const int32_t* ses = a.session[m];
    const int32_t* aid = a.aid[m];
    const float* score = a.score[m];
    unsigned long long vo = 0, va = ~0ull;
    unsigned int neg = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nm; i += (int64_t)gridDim.x * 256) {
        const int32_t s = ses[i], d = aid[i];
        neg += (s | d) < 0;
        const uint64_t k = ((uint64_t)(uint32_t)s << 32) | (uint64_t)(uint32_t)d;
        const int64_t o = a.off[m] + i;
        key[o] = k;
        val[o] = __float_as_uint(score[i]);
        mod[o] = (uint8_t)m;
        vo |= k;
        va &= k;
    }
    if (neg) atomicAdd(&sc->n_negative, neg);
    key_bits_fold(vo, va, sc->key_bits);
}

// flag[i] = 1 where sorted row i is the first of its key and some un-flagged model holds the key
__global__ __launch_bounds__(256) void k_join_mark(const uint64_t* key, const uint8_t* mod, int64_t n, int M, uint32_t unflagged,
                                                   uint8_t* flag, JoinScratch* sc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t k = key[i];
        uint8_t f = 0;
        if (i > 0 && key[i - 1] == k) {
            if (mod[i - 1] == mod[i]) atomicAdd(&sc->n_duplicate, 1u);
        } else {
            uint32_t present = 0;
            // a group without duplicates has at most M rows; it may end in another workgroup's stretch: bounded by n alone
            for (int64_t j = i; j < n && j < i + M && key[j] == k; ++j) present |= 1u << mod[j];
            f = (present & unflagged) != 0;
        }
        flag[i] = f;
    }
}

__global__ __launch_bounds__(256) void k_join_emit(JoinArgs a, const uint64_t* key, const uint32_t* val, const uint8_t* mod, int64_t n,
                                                   const uint8_t* flag, const uint64_t* pos, int32_t* out_aid, float* out_pred,
                                                   double* out_pred64, int32_t* out_sess, JoinScratch* sc) {
#pragma clang fp contract(off)                       // SPEC-BLEND: no fused multiply-add in the weighted sum
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint64_t k = key[i];
        const bool has_base = mod[i] == 0;
        int64_t j = i;
        const int64_t end = i + a.M < n ? i + a.M : n;
        float p = 0.0f;
        for (int m = 0; m < a.M; ++m) {
            float s = 0.0f;
            if (j < end && key[j] == k && (int)mod[j] == m) {
                s = __uint_as_float(val[j]);
                if (((a.flagged >> m) & 1u) && !has_base) s = 0.0f;
                ++j;
            }
            const float prod = s * a.w[m];
            p = m == 0 ? prod : p + prod;
        }
        const uint64_t o = pos[i];                   // < number of flagged rows <= n
        out_aid[o] = (int32_t)(uint32_t)k;
        out_pred[o] = p;
        if (out_pred64) out_pred64[o] = (double)p;
        out_sess[o] = (int32_t)(uint32_t)(k >> 32);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->n_out = pos[n];
}

struct SessHead {      // 1 where a new session starts among the output rows
    const int32_t* sess;
    const JoinScratch* sc;
    __device__ uint64_t operator()(int64_t i) const {
        return ((uint64_t)i < sc->n_out && (i == 0 || sess[i] != sess[i - 1])) ? 1ull : 0ull;
    }
};

__global__ __launch_bounds__(256) void k_join_sessions(const int32_t* sess, int64_t n, const uint64_t* pos, int32_t* out_sid,
                                                       int64_t* out_row_off, JoinScratch* sc) {
    const int64_t n_out = (int64_t)sc->n_out;        // <= n
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * 256) {
        if (i == 0 || sess[i] != sess[i - 1]) {
            const uint64_t p = pos[i];               // < number of session heads <= n_out
            out_sid[p] = sess[i];
            out_row_off[p] = i;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t ns = pos[n];
        out_row_off[ns] = n_out;
        sc->n_sessions = ns;
    }
}

int grid_for(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g < 256 * 16 ? g : 256 * 16);
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_blend_select_workspace(int64_t n) {
    (void)n;
    return (int64_t)align256(sizeof(SelState));
}

extern "C" int otto_blend_robust_stats(const double* d_x, int64_t n, int64_t* h_nv, double* h_stats, void* d_ws, int64_t ws_bytes,
                                       void* stream) {
    OTTO_REQUIRE(h_nv && h_stats, "otto_blend_robust_stats: null h_nv or h_stats");
    OTTO_REQUIRE(n > 0, "otto_blend_robust_stats: the column is empty (n = %lld)", (long long)n);
    OTTO_REQUIRE(d_x && d_ws, "otto_blend_robust_stats: null d_x or workspace");
    OTTO_REQUIRE(((uintptr_t)d_ws & 7) == 0, "otto_blend_robust_stats: the workspace must be 8-byte aligned");
    OTTO_REQUIRE(ws_bytes >= otto_blend_select_workspace(n), "workspace too small (%lld < %lld)", (long long)ws_bytes,
                 (long long)otto_blend_select_workspace(n));
    hipStream_t s = (hipStream_t)stream;
    SelState* st = (SelState*)d_ws;
    OTTO_HIP(hipMemsetAsync(st, 0, sizeof(SelState), s));
    const int64_t g = (n + SEL_THREADS - 1) / SEL_THREADS;
    const unsigned grid = (unsigned)(g < SEL_MAX_GRID ? g : SEL_MAX_GRID);
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        if (pass == 0) k_sel_hist<true><<<grid, SEL_THREADS, 0, s>>>(d_x, n, pass, st);
        else k_sel_hist<false><<<grid, SEL_THREADS, 0, s>>>(d_x, n, pass, st);
        k_sel_pick<<<1, SEL_THREADS, 0, s>>>(st, n, pass);
    }
    OTTO_HIP(hipGetLastError());
    SelResult h;
    OTTO_HIP(hipMemcpyAsync(&h, &st->res, sizeof h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (h.has_inf) {
        set_error("otto_blend_robust_stats: the column holds an infinite value");
        return OTTO_EINVAL;
    }
    if (h.nv <= 0) {
        set_error("otto_blend_robust_stats: all %lld entries of the column are NaN", (long long)n);
        return OTTO_EINVAL;
    }
    *h_nv = h.nv;
    memcpy(h_stats, h.stats, sizeof h.stats);
    return 0;
}

extern "C" int otto_blend_scale(const double* d_x, int64_t n, double center, double scale, float* d_out, void* stream) {
    OTTO_REQUIRE(n >= 0, "otto_blend_scale: n = %lld", (long long)n);
    if (n == 0) return 0;
    OTTO_REQUIRE(d_x && d_out, "otto_blend_scale: null argument");
    k_blend_scale<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(d_x, n, center, scale, d_out);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t otto_blend_join_workspace(int64_t n_total, int32_t M) {
    (void)M;
    if (n_total <= 0) return 256;
    return (int64_t)radix_ws_layout(n_total, true, nullptr, nullptr);
}

extern "C" int otto_blend_join(int32_t M, const int32_t* const* d_session, const int32_t* const* d_aid, const float* const* d_score,
                               const int64_t* n, const double* weight, const int32_t* left_of_base, int32_t* d_out_session_id,
                               int64_t* d_out_row_off, int32_t* d_out_aid, float* d_out_pred, double* d_out_pred64,
                               int64_t* h_n_out, int64_t* h_n_sessions, void* d_ws, int64_t ws_bytes, void* stream) {
    OTTO_REQUIRE(M >= 1 && M <= OTTO_BLEND_MAX_MODELS, "otto_blend_join: M must be in [1, %d] (got %d)", OTTO_BLEND_MAX_MODELS, M);
    OTTO_REQUIRE(d_session && d_aid && d_score && n && weight && left_of_base && h_n_out && h_n_sessions && d_out_row_off,
                 "otto_blend_join: null argument");
    OTTO_REQUIRE(left_of_base[0] == 0, "otto_blend_join: model 0 is the base and cannot be left_of_base");
    JoinArgs a;
    memset(&a, 0, sizeof a);
    a.M = M;
    int64_t tot = 0, n_max = 0;
    for (int m = 0; m < M; ++m) {
        OTTO_REQUIRE(n[m] >= 0, "otto_blend_join: n[%d] = %lld", m, (long long)n[m]);
        OTTO_REQUIRE(n[m] == 0 || (d_session[m] && d_aid[m] && d_score[m]), "otto_blend_join: null column of model %d", m);
        a.session[m] = d_session[m]; a.aid[m] = d_aid[m]; a.score[m] = d_score[m];
        a.off[m] = tot;
        a.w[m] = (float)weight[m];
        if (left_of_base[m]) a.flagged |= 1u << m;
        tot += n[m];
        n_max = n[m] > n_max ? n[m] : n_max;
        OTTO_REQUIRE(tot < (1ll << 31), "otto_blend_join: more than 2^31 - 1 rows in all");
    }
    a.off[M] = tot;
    hipStream_t s = (hipStream_t)stream;
    if (tot == 0) {
        *h_n_out = 0;
        *h_n_sessions = 0;
        OTTO_HIP(hipMemsetAsync(d_out_row_off, 0, 8, s));
        return 0;
    }
    OTTO_REQUIRE(d_out_session_id && d_out_aid && d_out_pred && d_ws, "otto_blend_join: null output or workspace");
    OTTO_REQUIRE(((uintptr_t)d_ws & 255) == 0, "otto_blend_join: the workspace must be 256-byte aligned");
    OTTO_REQUIRE(ws_bytes >= otto_blend_join_workspace(tot, M), "workspace too small (%lld < %lld)", (long long)ws_bytes,
                 (long long)otto_blend_join_workspace(tot, M));
    RadixWs w;
    radix_ws_layout(tot, true, (char*)d_ws, &w);
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_BLEND, 256, &scratch, s));
    JoinScratch* sc = (JoinScratch*)scratch;
    OTTO_HIP(hipMemsetAsync(sc, 0, sizeof(JoinScratch), s));
    OTTO_HIP(hipMemsetAsync(&sc->key_bits[1], 0xFF, 8, s));      // the AND of the keys starts at all ones
    k_join_keys<<<dim3((unsigned)grid_for(n_max), (unsigned)M), 256, 0, s>>>(a, w.key[0], w.val[0], w.byt[0], sc);
    OTTO_HIP(hipGetLastError());
    int cur = 0;                                     // all eight passes are launched, an even number: the sorted rows end in buffer 0
    OTTO_TRY((radix_passes<true>(w, tot, ~0ull, SkipOnDevice{sc->key_bits}, &cur, s)));
    // buffers 1 are free now: the group flags and the output rows' sessions live there
    uint8_t* flag = w.byt[1];
    int32_t* out_sess = (int32_t*)w.key[1];
    const int grid = grid_for(tot);
    k_join_mark<<<grid, 256, 0, s>>>(w.key[0], w.byt[0], tot, M, ~a.flagged & ((1u << M) - 1u), flag, sc);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(FlagAt{flag}, tot, w.offs, w.partial, s));
    k_join_emit<<<grid, 256, 0, s>>>(a, w.key[0], w.val[0], w.byt[0], tot, flag, w.offs, d_out_aid, d_out_pred, d_out_pred64, out_sess, sc);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(SessHead{out_sess, sc}, tot, w.offs, w.partial, s));
    k_join_sessions<<<grid, 256, 0, s>>>(out_sess, tot, w.offs, d_out_session_id, d_out_row_off, sc);
    OTTO_HIP(hipGetLastError());
    JoinScratch h;
    OTTO_HIP(hipMemcpyAsync(&h, sc, sizeof h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (h.n_negative) {
        set_error("otto_blend_join: %u rows with a negative session or aid", h.n_negative);
        return OTTO_EINVAL;
    }
    if (h.n_duplicate) {
        set_error("otto_blend_join: %u rows repeat a (session, aid) of their own model", h.n_duplicate);
        return OTTO_EINVAL;
    }
    *h_n_out = (int64_t)h.n_out;
    *h_n_sessions = (int64_t)h.n_sessions;
    return 0;
}
