// Skip-gram negative-sampling aid embeddings (SPEC-SGNS; include/otto_sgns.h).
//
// Device, on the caller's stream:
//   device_scan     (scan.h) over the weights: the exclusive sums; cum is their tail (cum[a] = excl[a + 1]).
//   k_sgns_bucket        bucket[b] = min(upper_bound(cum, b << shift), n - 1): one full binary search per bucket.
//   k_sgns_draw          the sampler alone (tests, and the definition the step kernels share: sgns_draw).
//   k_sgns_plan_check    aid range and offset rule; one error word.
//   device_scan     over the keep flags (recomputed from the event index, no flag array): the token position of every event.
//   k_sgns_plan_tokens   one thread per event: session by binary search of sess_off, token record, radius, clipped window.
//   k_sgns_plan_off      tok_off[s] = pos[sess_off[s]].
//   device_scan     over the pair counts: pair_off.
//   k_sgns_step<BATCH, HS>  one lane group of d/4 lanes per centre, grid-stride. h and grad live in registers, rows move as
//                   float4. The 1 + neg target ids of a pair are drawn by the group's lanes into LDS before any row is loaded,
//                   then the rows are fetched four at a time (sg_targets). HOGWILD: plain stores in place. BATCH: float64
//                   atomics into the dense workspaces, no table is written. HS (SPEC-SGNS-HS): the Syn1 rows on the Huffman
//                   path of the context go through sg_targets first; their ids are read from path_node (the same address in
//                   every lane of the group), the pair's code word is one uint64.
//   k_sgns_cbow<BATCH, HS, DOC>  SPEC-CBOW and PV-DM: one lane group per centre. The context rows of In (PV-DM: and the
//                   session's Doc row, found by binary search of tok_off) are gathered as float4, four loads in flight, and
//                   summed into h; the centre's own path and its 1 + neg targets go through sg_targets; the gradient is then
//                   added to every input row in input order. HOGWILD: the target and the input rows take their updates by
//                   float32 atomic adds in place (the centres of a session share these rows, plain read-modify-writes
//                   would lose all but one of their concurrent updates); BATCH: float64 atomic adds into the workspaces.
//   k_sgns_dbow<BATCH, HS>  PV-DBOW: one lane group per session that meets the launch's range; h = Doc[s] in registers.
//   k_sgns_infer<HS, DM> SPEC-DOC2VEC-INFER: one lane group per new session, taken through an order array; every pass and every
//                   token of the session inside the launch, the doc row in registers from its keyed initial value to one store.
//                   The model is frozen: the targets go through sg_targets' FROZEN path (no store, no atomic). No loss partial,
//                   no scratch: the loss is per session.
//   k_sgns_apply         BATCH: table += workspace, workspace = 0 (dense sweep).
//   k_sgns_loss_final    sums the per-workgroup loss partials in a fixed order.
// Device helpers the step kernels share, each defined once above k_sgns_step: sg_targets (four rows at a time against h),
//   sg_path_targets (the Huffman path of an aid through sg_targets), sg_draw_ids (1 + neg ids into LDS between two syncs),
//   sg_gather (the summed context rows), sg_loss_partial, sg_session_of (session of an event or a token), add4 / atomic_add4.
// Host helpers the entry points over those kernels share: check_shape (d, neg), check_n_aids, check_range, check_sessions,
//   check_paths (the Huffman tables), table_or_size (a job's negative table, or only n_aids), launch_dims,
//   apply_and_sum (BATCH apply, then k_sgns_loss_final). otto_sgns_step and otto_sgns_step_hs fill one SgStepCall.
// Host: otto_sgns_hs_tree_sizes / otto_sgns_hs_tree build the Huffman tree and the path tables of SPEC-SGNS-HS (no HIP call).
#include "common.h"
#include "wave.h"
#include "scan.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_sgns.h"

#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

namespace otto {

constexpr int SG_THREADS = 256;
constexpr int SG_MAX_GROUPS = 64;         // lane groups per workgroup: the workgroup is min(256, 64 * d/4) threads
constexpr int SG_GRID = 2048;            // 256 CUs x 8 workgroups
constexpr int SG_MAX_TARGETS = OTTO_SGNS_MAX_NEG + 1;
constexpr uint64_t SG_C_EPOCH = 0xD1342543DE82EF95ull, SG_C_EVENT = 0xA0761D6478BD642Full, SG_C_KEY = 0xE7037ED1A0B428DBull;

static __host__ __device__ __forceinline__ uint64_t sg_base(uint64_t seed, uint64_t epoch) { return mix64(seed ^ (epoch * SG_C_EPOCH)); }
static __host__ __device__ __forceinline__ uint64_t sg_ev(uint64_t base, uint64_t e) { return mix64(base ^ (e * SG_C_EVENT)); }
static __host__ __device__ __forceinline__ uint64_t sg_key(uint64_t ev, uint64_t stream, uint64_t w) {
    return mix64(ev ^ (((stream << 20) | w) * SG_C_KEY));
}

struct SgTable {
    const uint64_t* cum;
    const uint32_t* bucket;
    int64_t n;
    uint64_t total;
    int shift;
};

// first a in [lo, hi] with cum[a] > u; the caller guarantees cum[hi] > u
static __device__ __forceinline__ int64_t sg_upper(const uint64_t* cum, int64_t lo, int64_t hi, uint64_t u) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}

static __device__ __forceinline__ int32_t sgns_draw(const SgTable& t, uint64_t key) {
    const uint64_t u = __umul64hi(key, t.total);          // < total
    const uint64_t b = u >> t.shift;
    return (int32_t)sg_upper(t.cum, t.bucket[b], t.bucket[b + 1], u);
}

// the last s in [0, S) with off[s] <= i: the session of event (sess_off) or token (tok_off) i. Empty sessions share an
// offset; the last one holds i.
static __device__ __forceinline__ int64_t sg_session_of(const int64_t* off, int64_t S, int64_t i) {
    int64_t lo = 0, hi = S - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_sgns_bucket(const uint64_t* cum, int64_t n, uint64_t total, int shift, int64_t n_buckets,
                                                uint32_t* bucket) {
    const int64_t used = total ? (int64_t)((total - 1) >> shift) + 1 : 0;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b <= n_buckets; b += (int64_t)gridDim.x * 256) {
        uint32_t v = (uint32_t)(n - 1);
        if (b < used) {
            const uint64_t u = (uint64_t)b << shift;       // <= total - 1
            v = (uint32_t)sg_upper(cum, 0, n - 1, u);
        }
        bucket[b] = v;
    }
}

__global__ __launch_bounds__(256) void k_sgns_draw(SgTable t, const uint64_t* keys, int64_t m, int32_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) out[i] = sgns_draw(t, keys[i]);
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
struct SgPlanArgs {
    const int32_t* aid;
    int64_t E;
    const int64_t* sess_off;
    int64_t S;
    const uint32_t* keep_q;
    int64_t n_aids;
    uint64_t base;
    int64_t event0;
    int ws;
    uint32_t* err;
    const uint64_t* pos;      // [E + 1]
    uint8_t* npairs;          // [T] (workspace)
    int32_t* tok_aid;
    int64_t* tok_src;
    int64_t* tok_off;
    uint8_t* radius;
    uint8_t* tok_left;
};

struct SgKeepFn {
    const int32_t* aid;
    const uint32_t* keep_q;
    int64_t n_aids;
    uint64_t base;
    int64_t event0;
    __device__ __forceinline__ uint64_t operator()(int64_t e) const {
        const uint32_t a = (uint32_t)aid[e];
        if ((uint64_t)a >= (uint64_t)n_aids) return 0;
        const uint32_t q = keep_q[a];
        if (q == 0) return 0;
        const uint64_t k = sg_key(sg_ev(base, (uint64_t)(event0 + e)), 1, 0);
        return (uint32_t)(k >> 32) <= q ? 1 : 0;
    }
};

struct SgPairFn {
    const uint8_t* npairs;
    __device__ __forceinline__ uint64_t operator()(int64_t t) const { return npairs[t]; }
};

struct SgWeightFn {
    const uint32_t* w;
    __device__ __forceinline__ uint64_t operator()(int64_t a) const { return w[a]; }
};

__global__ __launch_bounds__(256) void k_sgns_plan_check(SgPlanArgs a) {
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * 256, i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t e = i0; e < a.E; e += stride) bad |= (uint64_t)(uint32_t)a.aid[e] >= (uint64_t)a.n_aids;
    for (int64_t s = i0; s < a.S; s += stride) {
        const int64_t lo = a.sess_off[s], hi = a.sess_off[s + 1];
        bad |= lo < 0 || hi < lo || hi > a.E;
    }
    if (i0 == 0) bad |= a.sess_off[0] != 0 || a.sess_off[a.S] != a.E;
    if (bad) atomicOr(a.err, 1u);
}

__global__ __launch_bounds__(256) void k_sgns_plan_tokens(SgPlanArgs a) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * 256) {
        const int64_t t = (int64_t)a.pos[e];
        if ((int64_t)a.pos[e + 1] == t) continue;          // not kept
        const int64_t lo = sg_session_of(a.sess_off, a.S, e);
        const int64_t tlo = (int64_t)a.pos[a.sess_off[lo]], thi = (int64_t)a.pos[a.sess_off[lo + 1]];
        const uint64_t ev = sg_ev(a.base, (uint64_t)(a.event0 + e));
        const int64_t r = 1 + (int64_t)(((sg_key(ev, 2, 0) >> 32) * (uint64_t)a.ws) >> 32);
        const int64_t left = min(r, t - tlo), right = min(r, thi - 1 - t);
        a.tok_aid[t] = a.aid[e];
        a.tok_src[t] = a.event0 + e;
        a.radius[t] = (uint8_t)r;
        a.tok_left[t] = (uint8_t)left;
        a.npairs[t] = (uint8_t)(left + right);
    }
}

__global__ __launch_bounds__(256) void k_sgns_plan_off(SgPlanArgs a) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s <= a.S; s += (int64_t)gridDim.x * 256)
        a.tok_off[s] = (int64_t)a.pos[a.sess_off[s]];
}

// ---------------------------------------------------------------------------
// step
// ---------------------------------------------------------------------------
struct SgStepArgs {
    const int32_t* tok_aid;
    const int64_t* tok_src;
    const uint8_t* tok_left;
    const int64_t* pair_off;
    int64_t T, t0, t1;
    float* In;
    float* Out;
    int d, G, neg;
    float lr;
    uint64_t base;
    SgTable tab;
    double* partial;          // [SG_GRID]
    int32_t* ctx_out;
    int32_t* neg_out;
    int64_t out_pairs;
    double* gin;
    double* gout;
    // SPEC-SGNS-HS (read by the HS instantiations alone)
    const int64_t* path_off;
    const int32_t* path_node;
    const uint64_t* code;
    float* Syn1;
    double* gsyn1;
    uint32_t n_inner;
};

static __device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
static __device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ float sigmoidf_exact(float x) {
    return x >= 0.0f ? 1.0f / (1.0f + expf(-x)) : expf(x) / (1.0f + expf(x));
}
static __device__ __forceinline__ float softplusf_exact(float z) {    // log(1 + exp(z))
    return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)));
}
static __device__ __forceinline__ void add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
static __device__ __forceinline__ void atomic_add4(float* p, const float4& v) {
    atomicAdd(p + 0, v.x); atomicAdd(p + 1, v.y); atomicAdd(p + 2, v.z); atomicAdd(p + 3, v.w);
}
static __device__ __forceinline__ void atomic_add4(double* p, const float4& v) {
    atomicAdd(p + 0, (double)v.x); atomicAdd(p + 1, (double)v.y); atomicAdd(p + 2, (double)v.z); atomicAdd(p + 3, (double)v.w);
}

// negative j of pair k of the centre whose event key is ev: redrawn while equal to the context aid
static __device__ __forceinline__ int32_t sgns_negative(const SgTable& t, uint64_t ev, int k, int j, int32_t ctx) {
    for (int att = 0; att < 16; ++att) {
        const int32_t n = sgns_draw(t, sg_key(ev, 3, ((uint64_t)k << 10) | ((uint64_t)j << 4) | (uint64_t)att));
        if (n != ctx) return n;
    }
    return (int32_t)(((int64_t)ctx + 1) % t.n);
}

// The rows idf(0) .. idf(n - 1) of `tab` against h, four at a time: the loads of a four go out before its first update.
// idf(m) < 0: no row. labf(m): the label. DUP: a row named twice in a four sees its own earlier update (HOGWILD over drawn
// targets; a Huffman path never repeats a node). ATOM (HOGWILD of SPEC-CBOW / SPEC-DOC2VEC): the row takes g * h by float32
// atomic adds, so that lane groups which hold the same row at the same time lose none of their updates. FROZEN
// (SPEC-DOC2VEC-INFER): the table is read-only, the row takes nothing: no store and no atomic.
template <bool BATCH, bool DUP, bool ATOM = false, bool FROZEN = false, class IdFn, class LabelFn>
static __device__ __forceinline__ void sg_targets(float* tab, double* gtab, int d, int G, int gl, int n, float lr, const float4& h,
                                                  float4& grad, double& lsum, IdFn idf, LabelFn labf) {
    for (int m0 = 0; m0 < n; m0 += 4) {
        int32_t id[4];
        float4 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            id[q] = m0 + q < n ? idf(m0 + q) : -1;
            if (id[q] >= 0) row[q] = ld4(tab + (int64_t)id[q] * d + 4 * gl);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (id[q] < 0) continue;
            float* po_ = tab + (int64_t)id[q] * d + 4 * gl;
            if (!BATCH && DUP) {
                bool dup = false;
#pragma unroll
                for (int w = 0; w < q; ++w) dup |= id[w] == id[q];
                if (dup) row[q] = ld4(po_);
            }
            const float4 o = row[q];
            const float x = group_sum(dot4(h, o), G);
            const bool pos = labf(m0 + q);
            const float g = lr * ((pos ? 1.0f : 0.0f) - sigmoidf_exact(x));
            if (gl == 0) lsum += (double)softplusf_exact(pos ? -x : x);
            grad.x += g * o.x; grad.y += g * o.y; grad.z += g * o.z; grad.w += g * o.w;
            if (FROZEN) {
                // nothing is written
            } else if (BATCH) {
                atomic_add4(gtab + (int64_t)id[q] * d + 4 * gl, make_float4(g * h.x, g * h.y, g * h.z, g * h.w));
            } else if (ATOM) {
                atomic_add4(po_, make_float4(g * h.x, g * h.y, g * h.z, g * h.w));
            } else {
                st4(po_, make_float4(o.x + g * h.x, o.y + g * h.y, o.z + g * h.z, o.w + g * h.w));
            }
        }
    }
}

// The Syn1 rows on the Huffman path of `aid` from the root, through sg_targets: label 1 - bit; a row outside [0, n_inner) is
// skipped, never touched. The ids are read from the table (the same address in every lane of the group). a: the kernel's
// argument record, for path_off, path_node, code, n_inner and d.
template <bool BATCH, bool ATOM, bool FROZEN, class Args>
static __device__ __forceinline__ void sg_path_targets(const Args& a, float* Syn1, double* gsyn1, int32_t aid, int G, int gl,
                                                       float lr, const float4& h, float4& grad, double& lsum) {
    const int64_t off = a.path_off[aid];
    const int64_t len = a.path_off[aid + 1] - off;
    const int L = off < 0 || len < 0 ? 0 : (int)(len > 64 ? 64 : len);
    const uint64_t code = a.code[aid];
    const int32_t* pn = a.path_node + off;
    const uint32_t n_inner = a.n_inner;
    sg_targets<BATCH, false, ATOM, FROZEN>(Syn1, gsyn1, a.d, G, gl, L, lr, h, grad, lsum,
                                           [&](int m) { const uint32_t n = (uint32_t)pn[m]; return n < n_inner ? (int32_t)n : -1; },
                                           [&](int m) { return ((code >> m) & 1ull) == 0; });
}

// The nt target ids of a lane group into its LDS row before any row is loaded: `first`, then negf(0) .. negf(nt - 2), drawn
// by the group's lanes. The first sync keeps the draw behind the group's reads of its previous ids.
template <class NegFn>
static __device__ __forceinline__ void sg_draw_ids(int32_t* ids, int G, int gl, int nt, int32_t first, const NegFn& negf) {
    wave_lds_sync();
    for (int m = gl; m < nt; m += G) ids[m] = m == 0 ? first : negf(m - 1);
    wave_lds_sync();
}

// The sum of the In rows of the np contexts of a centre, in pair order, four loads in flight. Context k is token
// cb + k + (k >= left): the centre itself is stepped over. An aid outside the table adds nothing (the plan checked every aid).
static __device__ __forceinline__ float4 sg_gather(const float* In, const int32_t* cb, int np, int left, uint64_t n_aids, int d,
                                                   int gl) {
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < np; k0 += 4) {
        float4 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + q;
            row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < np) {
                const uint32_t x = (uint32_t)cb[k + (k >= left)];
                if ((uint64_t)x < n_aids) row[q] = ld4(In + (int64_t)x * d + 4 * gl);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (k0 + q < np) add4(h, row[q]);
    }
    return h;
}

// per-workgroup loss partial, fixed order inside the workgroup
static __device__ __forceinline__ void sg_loss_partial(double lsum, double* s_red, double* partial) {
    lsum = wave_reduce<Sum>(lsum);
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_red[w];
        partial[blockIdx.x] = t;
    }
}

template <bool BATCH, bool HS>
__global__ __launch_bounds__(SG_THREADS) void k_sgns_step(SgStepArgs a) {
    // the target ids of the pair each lane group is working on
    __shared__ int32_t s_ids[SG_MAX_GROUPS * SG_MAX_TARGETS];
    __shared__ double s_red[SG_THREADS / 64];
    const int G = a.G;
    const int gl = threadIdx.x & (G - 1);
    const int grp = threadIdx.x / G;
    const int64_t gpb = blockDim.x / G;
    int32_t* ids = s_ids + grp * SG_MAX_TARGETS;
    const int nt = 1 + a.neg;
    const float lr = a.lr;
    double lsum = 0.0;
    const int64_t p0 = a.pair_off[a.t0];
    for (int64_t c = a.t0 + (int64_t)blockIdx.x * gpb + grp; c < a.t1; c += (int64_t)gridDim.x * gpb) {
        const int32_t ca = a.tok_aid[c];
        const int64_t pb = a.pair_off[c];
        const int np = (int)(a.pair_off[c + 1] - pb);
        const int left = a.tok_left[c];
        if ((uint64_t)(uint32_t)ca >= (uint64_t)a.tab.n || np <= 0 || np > 2 * OTTO_SGNS_MAX_WS || left > np) continue;
        const uint64_t ev = sg_ev(a.base, (uint64_t)a.tok_src[c]);
        float* pin = a.In + (int64_t)ca * a.d + 4 * gl;
        float4 h = ld4(pin);
        float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);      // BATCH: the centre's whole gradient
        for (int k = 0; k < np; ++k) {
            const int64_t ct = k < left ? c - left + k : c + 1 + (k - left);
            if (ct < 0 || ct >= a.T) continue;               // cannot happen for a plan of T tokens
            const int32_t ctx = a.tok_aid[ct];
            if ((uint64_t)(uint32_t)ctx >= (uint64_t)a.tab.n) continue;
            sg_draw_ids(ids, G, gl, nt, ctx, [&](int j) { return sgns_negative(a.tab, ev, k, j, ctx); });
            const int64_t po = pb + k - p0;
            if (po < a.out_pairs) {
                if (a.ctx_out && gl == 0) a.ctx_out[po] = ctx;
                if (a.neg_out)
                    for (int m = 1 + gl; m < nt; m += G) a.neg_out[po * a.neg + (m - 1)] = ids[m];
            }
            float4 grad = make_float4(0.f, 0.f, 0.f, 0.f);
            if (HS) sg_path_targets<BATCH, false, false>(a, a.Syn1, a.gsyn1, ctx, G, gl, lr, h, grad, lsum);
            sg_targets<BATCH, true>(a.Out, a.gout, a.d, G, gl, nt, lr, h, grad, lsum, [&](int m) { return ids[m]; },
                                    [](int m) { return m == 0; });
            if (BATCH) add4(gsum, grad); else add4(h, grad);
        }
        if (BATCH) atomic_add4(a.gin + (int64_t)ca * a.d + 4 * gl, gsum);
        else st4(pin, h);
    }
    sg_loss_partial(lsum, s_red, a.partial);
}

// ---------------------------------------------------------------------------
// SPEC-CBOW, SPEC-DOC2VEC
// ---------------------------------------------------------------------------
struct SgCbowArgs {
    const int32_t* tok_aid;
    const int64_t* tok_src;
    const uint8_t* tok_left;
    const int64_t* pair_off;
    const int64_t* tok_off;
    int64_t T, S, t0, t1;
    float* In;
    float* Out;
    float* Syn1;
    float* Doc;
    int d, G, neg, variant;
    float lr;
    uint64_t base;
    SgTable tab;              // tab.n = n_aids also when nothing is drawn
    double* partial;          // [SG_GRID]
    int32_t* neg_out;
    double* gin;
    double* gout;
    double* gsyn1;
    double* gdoc;
    const int64_t* path_off;
    const int32_t* path_node;
    const uint64_t* code;
    uint32_t n_inner;
};

// negative j of the centre whose event key is ev: stream 4, redrawn while equal to the centre's aid
static __device__ __forceinline__ int32_t cbow_negative(const SgTable& t, uint64_t ev, int j, int32_t ca) {
    for (int att = 0; att < 16; ++att) {
        const int32_t n = sgns_draw(t, sg_key(ev, 4, ((uint64_t)j << 4) | (uint64_t)att));
        if (n != ca) return n;
    }
    return (int32_t)(((int64_t)ca + 1) % t.n);
}

// The targets of centre c (aid ca, in range) against h: the ids are drawn into LDS before any row is loaded; the path of ca
// on Syn1, then ca and the negatives on Out. grad accumulates.
template <bool BATCH, bool HS>
static __device__ __forceinline__ void cbow_targets(const SgCbowArgs& a, int G, int gl, int32_t* ids, int64_t c, int32_t ca,
                                                    const float4& h, float4& grad, double& lsum) {
    const uint64_t ev = sg_ev(a.base, (uint64_t)a.tok_src[c]);
    const int nt = 1 + a.neg;
    sg_draw_ids(ids, G, gl, nt, ca, [&](int j) { return cbow_negative(a.tab, ev, j, ca); });
    if (a.neg_out)
        for (int m = 1 + gl; m < nt; m += G) a.neg_out[(c - a.t0) * a.neg + (m - 1)] = ids[m];
    if (HS) sg_path_targets<BATCH, !BATCH, false>(a, a.Syn1, a.gsyn1, ca, G, gl, a.lr, h, grad, lsum);
    sg_targets<BATCH, true, !BATCH>(a.Out, a.gout, a.d, G, gl, nt, a.lr, h, grad, lsum, [&](int m) { return ids[m]; },
                                    [](int m) { return m == 0; });
}

// CBOW (DOC = false) and PV-DM (DOC = true): one lane group per centre, grid-stride. The context rows are gathered as float4,
// four loads in flight, and summed in pair order; after the targets the same rows take u in that order (HOGWILD: float32
// atomic adds, BATCH: float64 atomic adds into the workspaces).
template <bool BATCH, bool HS, bool DOC>
__global__ __launch_bounds__(SG_THREADS) void k_sgns_cbow(SgCbowArgs a) {
    __shared__ int32_t s_ids[SG_MAX_GROUPS * SG_MAX_TARGETS];
    __shared__ double s_red[SG_THREADS / 64];
    const int G = a.G;
    const int gl = threadIdx.x & (G - 1);
    const int grp = threadIdx.x / G;
    const int64_t gpb = blockDim.x / G;
    int32_t* ids = s_ids + grp * SG_MAX_TARGETS;
    const uint64_t n_aids = (uint64_t)a.tab.n;
    double lsum = 0.0;
    for (int64_t c = a.t0 + (int64_t)blockIdx.x * gpb + grp; c < a.t1; c += (int64_t)gridDim.x * gpb) {
        const int32_t ca = a.tok_aid[c];
        const int np = (int)(a.pair_off[c + 1] - a.pair_off[c]);
        const int left = a.tok_left[c];
        const int n = np + (DOC ? 1 : 0);
        if ((uint64_t)(uint32_t)ca >= n_aids || np < 0 || np > 2 * OTTO_SGNS_MAX_WS || left > np || n == 0) continue;
        if (c - left < 0 || c + (np - left) >= a.T) continue;         // cannot happen for a plan of T tokens
        // context k is token cb + k + (k >= left): the centre itself is stepped over
        const int32_t* cb = a.tok_aid + (c - left);
        float* pdoc = nullptr;
        double* gdoc = nullptr;
        float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
        if (DOC) {
            const int64_t s = sg_session_of(a.tok_off, a.S, c);
            pdoc = a.Doc + s * a.d + 4 * gl;
            if (BATCH) gdoc = a.gdoc + s * a.d + 4 * gl;
            dr = ld4(pdoc);
        }
        float4 h = sg_gather(a.In, cb, np, left, n_aids, a.d, gl);
        if (DOC) add4(h, dr);
        const float fn = (float)n;
        if (a.variant != OTTO_SGNS_CBOW_SUM) { h.x = h.x / fn; h.y = h.y / fn; h.z = h.z / fn; h.w = h.w / fn; }
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        cbow_targets<BATCH, HS>(a, G, gl, ids, c, ca, h, u, lsum);
        if (a.variant == OTTO_SGNS_CBOW_MEAN) { u.x = u.x / fn; u.y = u.y / fn; u.z = u.z / fn; u.w = u.w / fn; }
        if (BATCH) {
            for (int k = 0; k < np; ++k) {
                const uint32_t x = (uint32_t)cb[k + (k >= left)];
                if ((uint64_t)x < n_aids) atomic_add4(a.gin + (int64_t)x * a.d + 4 * gl, u);
            }
            if (DOC) atomic_add4(gdoc, u);
        } else {
            // row += u as float32 atomic adds, in input order (one lane's adds to one address keep their order, so an aid
            // named m times takes m sequential read-modify-writes). The centres of a session share their context rows, and
            // in PV-DM the doc row: a plain read-modify-write would keep one of their concurrent updates and lose the rest.
            for (int k = 0; k < np; ++k) {
                const uint32_t x = (uint32_t)cb[k + (k >= left)];
                if ((uint64_t)x < n_aids) atomic_add4(a.In + (int64_t)x * a.d + 4 * gl, u);
            }
            if (DOC) atomic_add4(pdoc, u);
        }
    }
    sg_loss_partial(lsum, s_red, a.partial);
}

// PV-DBOW: one lane group per session whose token range meets [t0, t1), grid-stride over the sessions from the one of token
// t0 to the one of token t1 - 1. h = Doc[s] stays in registers over the session's tokens.
template <bool BATCH, bool HS>
__global__ __launch_bounds__(SG_THREADS) void k_sgns_dbow(SgCbowArgs a) {
    __shared__ int32_t s_ids[SG_MAX_GROUPS * SG_MAX_TARGETS];
    __shared__ double s_red[SG_THREADS / 64];
    const int G = a.G;
    const int gl = threadIdx.x & (G - 1);
    const int grp = threadIdx.x / G;
    const int64_t gpb = blockDim.x / G;
    int32_t* ids = s_ids + grp * SG_MAX_TARGETS;
    const uint64_t n_aids = (uint64_t)a.tab.n;
    double lsum = 0.0;
    const int64_t s0 = sg_session_of(a.tok_off, a.S, a.t0), s1 = sg_session_of(a.tok_off, a.S, a.t1 - 1);
    for (int64_t s = s0 + (int64_t)blockIdx.x * gpb + grp; s <= s1; s += (int64_t)gridDim.x * gpb) {
        const int64_t lo = max(a.tok_off[s], a.t0), hi = min(a.tok_off[s + 1], a.t1);
        if (lo >= hi) continue;                                       // an empty session
        float* pdoc = a.Doc + s * a.d + 4 * gl;
        float4 h = ld4(pdoc);
        float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);                // BATCH: the session's whole gradient
        for (int64_t c = lo; c < hi; ++c) {
            const int32_t ca = a.tok_aid[c];
            if ((uint64_t)(uint32_t)ca >= n_aids) continue;           // the plan checked every aid
            float4 grad = make_float4(0.f, 0.f, 0.f, 0.f);
            cbow_targets<BATCH, HS>(a, G, gl, ids, c, ca, h, grad, lsum);
            if (BATCH) add4(gsum, grad); else add4(h, grad);
        }
        if (BATCH) atomic_add4(a.gdoc + s * a.d + 4 * gl, gsum);
        else st4(pdoc, h);
    }
    sg_loss_partial(lsum, s_red, a.partial);
}

// ---------------------------------------------------------------------------
// SPEC-DOC2VEC-INFER
// ---------------------------------------------------------------------------
struct SgInferArgs {
    const int32_t* tok_aid;
    const int64_t* tok_off;
    const uint64_t* sess_key;     // null: the row index
    const int64_t* order;         // null: identity
    int64_t T, S;
    const float* In;
    const float* Out;
    const float* Syn1;
    float* Doc;
    double* loss;                 // [S, 2], nullable
    int32_t* neg_out;             // [P, T, neg], nullable
    uint8_t* radius_out;          // [P, T], nullable
    int d, G, neg, ws, variant, passes;
    SgTable tab;                  // tab.n = n_aids also when nothing is drawn
    const int64_t* path_off;
    const int32_t* path_node;
    const uint64_t* code;
    uint32_t n_inner;
    float lr[OTTO_SGNS_MAX_INFER_PASSES];
    uint64_t base[OTTO_SGNS_MAX_INFER_PASSES];     // sg_base(seed, p)
};

// component j of the initial row of the session whose pass-0 key is sb0: an odd multiple of 2^-24 * 2/d inside (-1/d, 1/d)
static __device__ __forceinline__ float infer_init(uint64_t sb0, int j, float two_over_d) {
    const uint32_t r = (uint32_t)(sg_key(sb0, 5, (uint64_t)j) >> 41);                   // 23 bits
    return ((float)(2u * r + 1u) * 5.9604644775390625e-8f - 0.5f) * two_over_d;         // 2^-24; every step is exact
}

// The targets of token c (aid ca, in range, event key ev) against h on the frozen tables: cbow_targets without a write.
template <bool HS, bool WIN>
static __device__ __forceinline__ void infer_targets(const SgInferArgs& a, int G, int gl, int32_t* ids, int64_t slot, int32_t ca,
                                                     uint64_t ev, float lr, const float4& h, float4& grad, double& lsum) {
    const int nt = 1 + a.neg;
    sg_draw_ids(ids, G, gl, nt, ca, [&](int j) { return cbow_negative(a.tab, ev, j, ca); });
    if (WIN && a.neg_out)
        for (int m = 1 + gl; m < nt; m += G) a.neg_out[slot * a.neg + (m - 1)] = ids[m];
    // FROZEN never writes through these pointers
    if (HS) sg_path_targets<false, false, true>(a, const_cast<float*>(a.Syn1), nullptr, ca, G, gl, lr, h, grad, lsum);
    sg_targets<false, false, false, true>(const_cast<float*>(a.Out), nullptr, a.d, G, gl, nt, lr, h, grad, lsum,
                                          [&](int m) { return ids[m]; }, [](int m) { return m == 0; });
}

// One lane group per session, taken through `order`, grid-stride. The doc row lives in registers from its keyed initial value
// over all passes and tokens to the one store; the model tables are only read. DM: PV-DM, else PV-DBOW. WIN: the tests' window
// (neg_out, radius_out) is compiled in; a call without either pointer runs the kernels without it.
template <bool HS, bool DM, bool WIN>
__global__ __launch_bounds__(SG_THREADS) void k_sgns_infer(SgInferArgs a) {
    __shared__ int32_t s_ids[SG_MAX_GROUPS * SG_MAX_TARGETS];
    const int G = a.G;
    const int gl = threadIdx.x & (G - 1);
    const int grp = threadIdx.x / G;
    const int64_t gpb = blockDim.x / G;
    int32_t* ids = s_ids + grp * SG_MAX_TARGETS;
    const uint64_t n_aids = (uint64_t)a.tab.n;
    const float two_over_d = 2.0f / (float)a.d;
    const bool mean_h = a.variant != OTTO_SGNS_CBOW_SUM, mean_u = a.variant == OTTO_SGNS_CBOW_MEAN;
    for (int64_t it = (int64_t)blockIdx.x * gpb + grp; it < a.S; it += (int64_t)gridDim.x * gpb) {
        const int64_t s = a.order ? a.order[it] : it;
        if (s < 0 || s >= a.S) continue;                              // not a permutation: the row is left alone
        const int64_t lo64 = a.tok_off[s], hi64 = a.tok_off[s + 1];
        const bool plan_ok = lo64 >= 0 && lo64 <= hi64 && hi64 <= a.T;      // always, for a plan of T tokens (T < 2^31)
        const int lo = plan_ok ? (int)lo64 : 0, hi = plan_ok ? (int)hi64 : 0;
        const uint64_t skey = a.sess_key ? a.sess_key[s] : (uint64_t)s;
        const uint64_t sb0 = sg_ev(a.base[0], skey);
        float4 hd = make_float4(infer_init(sb0, 4 * gl + 0, two_over_d), infer_init(sb0, 4 * gl + 1, two_over_d),
                                infer_init(sb0, 4 * gl + 2, two_over_d), infer_init(sb0, 4 * gl + 3, two_over_d));
        // one loop over (pass, token): the passes of a session run in order, each over its tokens in order
        double l_first = 0.0, lsum = 0.0;
        int p = 0;
        int c = lo;
        uint64_t sb = sb0;
        float lr = a.lr[0];
        while (c < hi) {
            const int32_t ca = a.tok_aid[c];
            if ((uint64_t)(uint32_t)ca < n_aids) {                    // the plan checked every aid
                const uint64_t ev = sg_ev(sb, (uint64_t)(c - lo));
                const int64_t slot = (int64_t)p * a.T + c;
                float4 grad = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!DM) {
                    infer_targets<HS, WIN>(a, G, gl, ids, slot, ca, ev, lr, hd, grad, lsum);
                } else {
                    const int r = 1 + (int)(((sg_key(ev, 2, 0) >> 32) * (uint64_t)a.ws) >> 32);
                    if (WIN && a.radius_out && gl == 0) a.radius_out[slot] = (uint8_t)r;
                    const int left = min(r, c - lo), np = left + min(r, hi - 1 - c);
                    // context k is token cb + k + (k >= left): the centre itself is stepped over
                    const int32_t* cb = a.tok_aid + (c - left);
                    float4 h = sg_gather(a.In, cb, np, left, n_aids, a.d, gl);
                    add4(h, hd);
                    const float fn = (float)(np + 1);
                    if (mean_h) { h.x = h.x / fn; h.y = h.y / fn; h.z = h.z / fn; h.w = h.w / fn; }
                    infer_targets<HS, WIN>(a, G, gl, ids, slot, ca, ev, lr, h, grad, lsum);
                    if (mean_u) { grad.x = grad.x / fn; grad.y = grad.y / fn; grad.z = grad.z / fn; grad.w = grad.w / fn; }
                }
                add4(hd, grad);                                       // centre c + 1 sees the doc row that centre c left
            }
            if (++c == hi) {                                          // the pass ends
                if (p == 0) l_first = lsum;
                if (++p == a.passes) break;
                c = lo;
                sb = sg_ev(a.base[p], skey);
                lr = a.lr[p];
                lsum = 0.0;
            }
        }
        const double l_last = lsum;                                   // the sum of the last pass (0 without tokens)
        st4(a.Doc + s * a.d + 4 * gl, hd);
        if (a.loss && gl == 0) { a.loss[2 * s] = l_first; a.loss[2 * s + 1] = l_last; }
    }
}

__global__ __launch_bounds__(256) void k_sgns_loss_final(const double* partial, int n, double* out) {
    __shared__ double s[256];
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) t += partial[i];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// table += workspace, workspace = 0
__global__ __launch_bounds__(256) void k_sgns_apply(float* tab, double* g, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = g[i];
        if (v != 0.0) {
            tab[i] = (float)((double)tab[i] + v);
            g[i] = 0.0;
        }
    }
}

static int grid_for(int64_t n, int per_block) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (int)(g > SG_GRID ? SG_GRID : g);
}

static int table_from(const otto_sgns_table* t, SgTable* out) {
    OTTO_REQUIRE(t && t->d_cum && t->d_bucket, "null negative table");
    OTTO_REQUIRE(t->n_aids >= 1 && t->n_aids < (1ll << 31) && t->n_buckets >= 1, "negative table: bad sizes");
    OTTO_REQUIRE(t->shift >= 0 && t->shift < 64, "negative table: bad shift");
    OTTO_REQUIRE(t->total > 0, "negative table: total weight is 0, nothing can be drawn");
    OTTO_REQUIRE((int64_t)((t->total - 1) >> t->shift) + 1 <= t->n_buckets, "negative table: shift does not fit n_buckets");
    out->cum = t->d_cum; out->bucket = t->d_bucket; out->n = t->n_aids; out->total = t->total; out->shift = t->shift;
    return 0;
}

// ---------------------------------------------------------------------------
// what the three entry points over the step kernels (otto_sgns_step[_hs], otto_sgns_cbow_step, otto_sgns_infer) share
// ---------------------------------------------------------------------------
static int check_shape(int d, int neg) {
    OTTO_REQUIRE(d >= 4 && d <= OTTO_SGNS_MAX_DIM && d % 4 == 0 && ((d / 4) & (d / 4 - 1)) == 0,
                 "d = %d: need a multiple of 4 in [4, %d] with d/4 a power of two", d, OTTO_SGNS_MAX_DIM);
    OTTO_REQUIRE(neg >= 0 && neg <= OTTO_SGNS_MAX_NEG, "neg = %d outside [0, %d]", neg, OTTO_SGNS_MAX_NEG);
    return 0;
}

static int check_n_aids(int64_t n_aids) {
    OTTO_REQUIRE(n_aids >= 1 && n_aids < (1ll << 31), "n_aids = %lld outside [1, 2^31)", (long long)n_aids);
    return 0;
}

static int check_range(int64_t T, int64_t t0, int64_t t1) {
    OTTO_REQUIRE(T >= 0 && T < (1ll << 31) && 0 <= t0 && t0 <= t1 && t1 <= T, "token range [%lld, %lld) outside the plan's %lld",
                 (long long)t0, (long long)t1, (long long)T);
    return 0;
}

static int check_sessions(int64_t S, int64_t T) {
    OTTO_REQUIRE(T >= 0 && T < (1ll << 31) && S >= 0 && S < (1ll << 31) && (T == 0 || S >= 1), "S = %lld sessions for %lld tokens",
                 (long long)S, (long long)T);
    return 0;
}

// the Huffman tables of a caller that gave any of them
static int check_paths(const int64_t* path_off, const int32_t* path_node, const uint64_t* code, const float* Syn1, int64_t n_inner) {
    OTTO_REQUIRE(path_off && path_node && code && Syn1, "null hierarchical-softmax table");
    OTTO_REQUIRE(n_inner >= 1 && n_inner < (1ll << 31), "n_inner = %lld outside [1, 2^31)", (long long)n_inner);
    return 0;
}

// The negative table of a job record when something is drawn (an unset one reads as "total weight is 0"), else only its
// size: tab.n = n_aids either way.
static int table_or_size(const otto_sgns_table& t, int neg, int64_t n_aids, SgTable* out) {
    if (neg > 0) {
        OTTO_REQUIRE(t.total > 0, "negative table: total weight is 0, nothing can be drawn");
        OTTO_TRY(table_from(&t, out));
        OTTO_REQUIRE(t.n_aids == n_aids && n_aids >= 2, "negative sampling needs at least 2 aids and a table over n_aids");
    }
    out->n = n_aids;
    return 0;
}

// one lane group of G = d/4 lanes per item: the workgroup is min(256, 64 * G) threads; returns the grid
static int launch_dims(int G, int64_t items, int* threads) {
    *threads = G >= 4 ? SG_THREADS : 64 * G;
    return grid_for(items, *threads / G);
}

// a table a training launch may have written and its BATCH workspace; tab = null: this launch's arch has no such table
struct SgDense {
    float* tab;
    double* g;
    int64_t rows;
};

// the tail of a training launch: BATCH applies every workspace to its table, in the order given; then the loss sum
static int apply_and_sum(bool batch, std::initializer_list<SgDense> tabs, int d, const double* partial, int grid,
                         double* d_loss_sum, hipStream_t s) {
    for (const SgDense& t : tabs) {
        if (!batch || !t.tab) continue;
        const int64_t n = t.rows * (int64_t)d;
        k_sgns_apply<<<grid_for(n, 256), 256, 0, s>>>(t.tab, t.g, n);
    }
    k_sgns_loss_final<<<1, 256, 0, s>>>(partial, grid, d_loss_sum);
    OTTO_HIP(hipGetLastError());
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_sgns_neg_table_workspace(int64_t n_aids) {
    if (n_aids < 1 || n_aids >= (1ll << 31)) return 0;
    return (int64_t)((size_t)(n_aids + 1) * 8 + scan_partial_bytes(n_aids));
}

extern "C" int otto_sgns_neg_table(const uint32_t* d_weight, int64_t n_aids, int64_t n_buckets, uint64_t* d_cum,
                                   uint32_t* d_bucket, otto_sgns_table* table, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(d_weight && d_cum && d_bucket && table && d_work, "null argument");
    OTTO_TRY(check_n_aids(n_aids));
    OTTO_REQUIRE(n_buckets >= 1 && n_buckets < (1ll << 31), "n_buckets = %lld outside [1, 2^31)", (long long)n_buckets);
    OTTO_REQUIRE(work_bytes >= otto_sgns_neg_table_workspace(n_aids), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    uint64_t* excl = reinterpret_cast<uint64_t*>(d_work);
    uint64_t* partial = excl + (n_aids + 1);
    OTTO_TRY(device_scan(SgWeightFn{d_weight}, n_aids, excl, partial, s));
    OTTO_HIP(hipMemcpyAsync(d_cum, excl + 1, (size_t)n_aids * 8, hipMemcpyDeviceToDevice, s));
    uint64_t total = 0;
    OTTO_HIP(hipMemcpyAsync(&total, excl + n_aids, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    int shift = 0;
    while (total && (int64_t)((total - 1) >> shift) + 1 > n_buckets) ++shift;
    k_sgns_bucket<<<grid_for(n_buckets + 1, 256), 256, 0, s>>>(d_cum, n_aids, total, shift, n_buckets, d_bucket);
    OTTO_HIP(hipGetLastError());
    table->d_cum = d_cum; table->d_bucket = d_bucket; table->n_aids = n_aids; table->n_buckets = n_buckets;
    table->total = total; table->shift = shift;
    return 0;
}

extern "C" int otto_sgns_draw(const otto_sgns_table* table, const uint64_t* d_keys, int64_t m, int32_t* d_out, void* stream) {
    SgTable t;
    OTTO_TRY(table_from(table, &t));
    OTTO_REQUIRE(m >= 0 && (m == 0 || (d_keys && d_out)), "null argument");
    if (m == 0) return 0;
    k_sgns_draw<<<grid_for(m, 256), 256, 0, (hipStream_t)stream>>>(t, d_keys, m, d_out);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t otto_sgns_plan_workspace(int64_t E) {
    if (E < 0 || E >= (1ll << 31)) return 0;
    // pos [E + 1] and the scan partials (the pair scan reuses them: T <= E), then one pair count per token
    return (int64_t)((size_t)(E + 1) * 8 + scan_partial_bytes(E) + (size_t)E + 256);
}

extern "C" int otto_sgns_plan(const int32_t* d_aid, int64_t E, const int64_t* d_sess_off, int64_t S, const uint32_t* d_keep_q,
                              int64_t n_aids, uint64_t seed, uint64_t epoch, int64_t event0, int32_t ws, int64_t cap_tokens,
                              int32_t* d_tok_aid, int64_t* d_tok_src, int64_t* d_tok_off, uint8_t* d_radius,
                              uint8_t* d_tok_left, int64_t* d_pair_off, int64_t* h_counts, void* d_work, int64_t work_bytes,
                              void* stream) {
    OTTO_REQUIRE(E >= 0 && E < (1ll << 31), "E = %lld outside [0, 2^31)", (long long)E);
    OTTO_REQUIRE(S >= 0 && S < (1ll << 31), "S = %lld outside [0, 2^31)", (long long)S);
    OTTO_TRY(check_n_aids(n_aids));
    OTTO_REQUIRE(ws >= 1 && ws <= OTTO_SGNS_MAX_WS, "ws = %d outside [1, %d]", ws, OTTO_SGNS_MAX_WS);
    OTTO_REQUIRE(event0 >= 0 && cap_tokens >= 0, "negative event0 or cap_tokens");
    OTTO_REQUIRE(d_sess_off && d_keep_q && d_tok_off && d_pair_off && h_counts && d_work && (E == 0 || d_aid), "null argument");
    OTTO_REQUIRE(cap_tokens == 0 || (d_tok_aid && d_tok_src && d_radius && d_tok_left), "null token output");
    OTTO_REQUIRE(work_bytes >= otto_sgns_plan_workspace(E), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_SGNS, 256, &scratch, s));
    uint64_t* pos = reinterpret_cast<uint64_t*>(d_work);
    uint64_t* partial = pos + (E + 1);
    uint8_t* npairs = reinterpret_cast<uint8_t*>(partial) + scan_partial_bytes(E);
    SgPlanArgs a;
    memset(&a, 0, sizeof a);
    a.aid = d_aid; a.E = E; a.sess_off = d_sess_off; a.S = S; a.keep_q = d_keep_q; a.n_aids = n_aids;
    a.base = sg_base(seed, epoch); a.event0 = event0; a.ws = ws; a.err = reinterpret_cast<uint32_t*>(scratch);
    a.pos = pos; a.npairs = npairs; a.tok_aid = d_tok_aid; a.tok_src = d_tok_src; a.tok_off = d_tok_off;
    a.radius = d_radius; a.tok_left = d_tok_left;
    OTTO_HIP(hipMemsetAsync(scratch, 0, 256, s));
    k_sgns_plan_check<<<grid_for(E > S ? E : S, 256), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(SgKeepFn{d_aid, d_keep_q, n_aids, a.base, event0}, E, pos, partial, s));
    uint32_t bad = 0;
    uint64_t T = 0;
    OTTO_HIP(hipMemcpyAsync(&bad, scratch, 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&T, pos + E, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(!bad, "otto_sgns_plan: an aid outside [0, %lld) or session offsets that do not ascend from 0 to E",
                 (long long)n_aids);
    OTTO_REQUIRE((int64_t)T <= cap_tokens, "otto_sgns_plan: %lld kept tokens, room for %lld", (long long)T, (long long)cap_tokens);
    if (E > 0 && S > 0) k_sgns_plan_tokens<<<grid_for(E, 256), 256, 0, s>>>(a);
    k_sgns_plan_off<<<grid_for(S + 1, 256), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(SgPairFn{npairs}, (int64_t)T, reinterpret_cast<uint64_t*>(d_pair_off), partial, s));
    uint64_t P = 0;
    OTTO_HIP(hipMemcpyAsync(&P, d_pair_off + T, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    h_counts[0] = (int64_t)T;
    h_counts[1] = (int64_t)P;
    return 0;
}

namespace otto {

// The arguments of otto_sgns_step, in the order of the header, and what otto_sgns_step_hs adds to them.
struct SgStepCall {
    const int32_t* tok_aid;
    const int64_t* tok_src;
    const uint8_t* tok_left;
    const int64_t* pair_off;
    int64_t T, t0, t1;
    float* In;
    float* Out;
    int32_t d, neg;
    float lr;
    int32_t mode;
    uint64_t seed, epoch;
    const otto_sgns_table* table;
    double* loss_sum;
    int32_t* ctx_out;
    int32_t* neg_out;
    int64_t out_pairs;
    double* gin;
    double* gout;
    void* stream;
    // what otto_sgns_step_hs adds, assigned by name
    bool hs = false;
    const int64_t* path_off = nullptr;
    const int32_t* path_node = nullptr;
    const uint64_t* code = nullptr;
    float* Syn1 = nullptr;
    int64_t n_inner = 0;
    double* gsyn1 = nullptr;
};

static int sgns_step(const SgStepCall& c) {
    const bool hs = c.hs, batch = c.mode == OTTO_SGNS_BATCH;
    OTTO_TRY(check_shape(c.d, c.neg));
    OTTO_REQUIRE(c.mode == OTTO_SGNS_HOGWILD || batch, "unknown SGNS mode %d", c.mode);
    OTTO_TRY(check_range(c.T, c.t0, c.t1));
    OTTO_REQUIRE(c.pair_off && c.In && c.Out && c.loss_sum && c.table, "null argument");
    OTTO_REQUIRE(c.T == 0 || (c.tok_aid && c.tok_src && c.tok_left), "null plan array");
    OTTO_REQUIRE(!batch || (c.gin && c.gout), "BATCH mode needs both gradient workspaces");
    OTTO_REQUIRE(c.out_pairs >= 0 && (c.out_pairs > 0 || (!c.ctx_out && !c.neg_out)), "ctx_out / neg_out without out_pairs");
    if (hs) {
        OTTO_TRY(check_paths(c.path_off, c.path_node, c.code, c.Syn1, c.n_inner));
        OTTO_REQUIRE(!batch || c.gsyn1, "BATCH mode needs the Syn1 gradient workspace");
    }
    hipStream_t s = (hipStream_t)c.stream;
    if (c.t0 == c.t1) {
        OTTO_HIP(hipMemsetAsync(c.loss_sum, 0, sizeof(double), s));
        return 0;
    }
    SgStepArgs a;
    memset(&a, 0, sizeof a);
    // the table is this entry point's only source of n_aids
    if (c.neg > 0) {
        OTTO_TRY(table_from(c.table, &a.tab));
        OTTO_REQUIRE(c.table->n_aids >= 2, "negative sampling needs at least 2 aids");
    } else {
        OTTO_REQUIRE(c.table->n_aids >= 1 && c.table->n_aids < (1ll << 31), "negative table: bad sizes");
        a.tab.n = c.table->n_aids;
    }
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_SGNS_STEP, (size_t)SG_GRID * sizeof(double), &scratch, s));
    a.tok_aid = c.tok_aid; a.tok_src = c.tok_src; a.tok_left = c.tok_left; a.pair_off = c.pair_off;
    a.T = c.T; a.t0 = c.t0; a.t1 = c.t1; a.In = c.In; a.Out = c.Out; a.d = c.d; a.G = c.d / 4; a.neg = c.neg; a.lr = c.lr;
    a.base = sg_base(c.seed, c.epoch); a.partial = reinterpret_cast<double*>(scratch);
    a.ctx_out = c.ctx_out; a.neg_out = c.neg > 0 ? c.neg_out : nullptr; a.out_pairs = c.out_pairs; a.gin = c.gin; a.gout = c.gout;
    a.path_off = c.path_off; a.path_node = c.path_node; a.code = c.code; a.Syn1 = c.Syn1; a.gsyn1 = c.gsyn1;
    a.n_inner = (uint32_t)c.n_inner;                          // null and 0 from otto_sgns_step
    int threads;
    const int grid = launch_dims(a.G, c.t1 - c.t0, &threads);
    if (!batch && hs) k_sgns_step<false, true><<<grid, threads, 0, s>>>(a);
    else if (!batch) k_sgns_step<false, false><<<grid, threads, 0, s>>>(a);
    else if (hs) k_sgns_step<true, true><<<grid, threads, 0, s>>>(a);
    else k_sgns_step<true, false><<<grid, threads, 0, s>>>(a);
    return apply_and_sum(batch, {{c.In, c.gin, a.tab.n}, {c.Out, c.gout, a.tab.n}, {a.Syn1, c.gsyn1, c.n_inner}}, c.d, a.partial, grid,
                         c.loss_sum, s);
}

template <bool BATCH, bool HS>
static void launch_cbow(int arch, int grid, int threads, hipStream_t s, const SgCbowArgs& a) {
    if (arch == OTTO_SGNS_ARCH_CBOW) k_sgns_cbow<BATCH, HS, false><<<grid, threads, 0, s>>>(a);
    else if (arch == OTTO_SGNS_ARCH_PVDM) k_sgns_cbow<BATCH, HS, true><<<grid, threads, 0, s>>>(a);
    else k_sgns_dbow<BATCH, HS><<<grid, threads, 0, s>>>(a);
}

template <bool WIN>
static void launch_infer(bool hs, bool dm, int grid, int threads, hipStream_t s, const SgInferArgs& a) {
    if (dm && hs) k_sgns_infer<true, true, WIN><<<grid, threads, 0, s>>>(a);
    else if (dm) k_sgns_infer<false, true, WIN><<<grid, threads, 0, s>>>(a);
    else if (hs) k_sgns_infer<true, false, WIN><<<grid, threads, 0, s>>>(a);
    else k_sgns_infer<false, false, WIN><<<grid, threads, 0, s>>>(a);
}

// The tree of SPEC-SGNS-HS over the in-vocabulary aids: leaves 0..V-1 in (count desc, aid asc) order, inner nodes V..2V-2.
struct SgTree {
    std::vector<int32_t> leaf_aid;      // [V]
    std::vector<int32_t> parent;        // [2V - 1]
    std::vector<uint8_t> bit;           // [2V - 1]
    std::vector<int32_t> depth;         // [2V - 1]: edges from the root
    int64_t V = 0, sum_len = 0, max_len = 0;
};

static int sgns_hs_build(const int64_t* count, int64_t n_aids, int64_t min_count, SgTree* t) {
    OTTO_REQUIRE(count, "null argument");
    OTTO_TRY(check_n_aids(n_aids));
    const int64_t floor_count = min_count > 1 ? min_count : 1;
    int64_t total = 0;
    for (int64_t a = 0; a < n_aids; ++a) {
        OTTO_REQUIRE(count[a] >= 0 && count[a] < (1ll << 62) - total, "count[%lld] is negative or the counts sum past 2^62",
                     (long long)a);
        total += count[a];
        if (count[a] >= floor_count) t->leaf_aid.push_back((int32_t)a);
    }
    std::stable_sort(t->leaf_aid.begin(), t->leaf_aid.end(), [&](int32_t x, int32_t y) { return count[x] > count[y]; });
    const int64_t V = t->V = (int64_t)t->leaf_aid.size();
    if (V < 2) return 0;
    std::vector<int64_t> cnt((size_t)(2 * V - 1), total + 1);       // the sentinel is above any sum
    for (int64_t i = 0; i < V; ++i) cnt[i] = count[t->leaf_aid[i]];
    t->parent.assign((size_t)(2 * V - 1), -1);
    t->bit.assign((size_t)(2 * V - 1), 0);
    int64_t p1 = V - 1, p2 = V;
    for (int64_t a = 0; a < V - 1; ++a) {
        int64_t mn[2];
        for (int w = 0; w < 2; ++w) mn[w] = p1 >= 0 && cnt[p1] < cnt[p2] ? p1-- : p2++;    // a tie takes the inner node
        cnt[V + a] = cnt[mn[0]] + cnt[mn[1]];
        t->parent[mn[0]] = t->parent[mn[1]] = (int32_t)(V + a);
        t->bit[mn[1]] = 1;
    }
    // a parent is made after its children, so it has the larger index: one sweep from the root down gives every depth
    t->depth.assign((size_t)(2 * V - 1), 0);
    for (int64_t n = 2 * V - 3; n >= 0; --n) t->depth[n] = t->depth[t->parent[n]] + 1;
    for (int64_t i = 0; i < V; ++i) {
        t->sum_len += t->depth[i];
        if (t->depth[i] > t->max_len) t->max_len = t->depth[i];
    }
    return 0;
}

}  // namespace otto

extern "C" int otto_sgns_step(const int32_t* d_tok_aid, const int64_t* d_tok_src, const uint8_t* d_tok_left,
                              const int64_t* d_pair_off, int64_t T, int64_t t0, int64_t t1, float* d_In, float* d_Out, int32_t d,
                              int32_t neg, float lr, int32_t mode, uint64_t seed, uint64_t epoch, const otto_sgns_table* table,
                              double* d_loss_sum, int32_t* d_ctx_out, int32_t* d_neg_out, int64_t out_pairs, double* d_gin,
                              double* d_gout, void* stream) {
    return sgns_step({d_tok_aid, d_tok_src, d_tok_left, d_pair_off, T, t0, t1, d_In, d_Out, d, neg, lr, mode, seed, epoch, table,
                      d_loss_sum, d_ctx_out, d_neg_out, out_pairs, d_gin, d_gout, stream});
}

extern "C" int otto_sgns_step_hs(const int32_t* d_tok_aid, const int64_t* d_tok_src, const uint8_t* d_tok_left,
                                 const int64_t* d_pair_off, int64_t T, int64_t t0, int64_t t1, float* d_In, float* d_Out, int32_t d,
                                 int32_t neg, float lr, int32_t mode, uint64_t seed, uint64_t epoch, const otto_sgns_table* table,
                                 double* d_loss_sum, int32_t* d_ctx_out, int32_t* d_neg_out, int64_t out_pairs, double* d_gin,
                                 double* d_gout, const int64_t* d_path_off, const int32_t* d_path_node, const uint64_t* d_code,
                                 float* d_Syn1, int64_t n_inner, double* d_gsyn1, void* stream) {
    SgStepCall c = {d_tok_aid, d_tok_src, d_tok_left, d_pair_off, T, t0, t1, d_In, d_Out, d, neg, lr, mode, seed, epoch, table,
                    d_loss_sum, d_ctx_out, d_neg_out, out_pairs, d_gin, d_gout, stream};
    c.hs = true; c.path_off = d_path_off; c.path_node = d_path_node; c.code = d_code; c.Syn1 = d_Syn1; c.n_inner = n_inner;
    c.gsyn1 = d_gsyn1;
    return sgns_step(c);
}

extern "C" int otto_sgns_cbow_step(const otto_sgns_cbow_job* job) {
    OTTO_REQUIRE(job, "null job");
    const otto_sgns_cbow_job& j = *job;
    const int arch = j.arch, d = j.d, neg = j.neg;
    OTTO_REQUIRE(arch == OTTO_SGNS_ARCH_CBOW || arch == OTTO_SGNS_ARCH_PVDM || arch == OTTO_SGNS_ARCH_DBOW, "unknown arch %d", arch);
    const bool dbow = arch == OTTO_SGNS_ARCH_DBOW, doc = arch != OTTO_SGNS_ARCH_CBOW, batch = j.mode == OTTO_SGNS_BATCH;
    OTTO_REQUIRE(dbow || j.variant == OTTO_SGNS_CBOW_SUM || j.variant == OTTO_SGNS_CBOW_MEAN || j.variant == OTTO_SGNS_CBOW_FASTTEXT,
                 "unknown variant %d", j.variant);
    OTTO_REQUIRE(j.mode == OTTO_SGNS_HOGWILD || batch, "unknown SGNS mode %d", j.mode);
    OTTO_TRY(check_shape(d, neg));
    OTTO_TRY(check_n_aids(j.n_aids));
    OTTO_TRY(check_range(j.T, j.t0, j.t1));
    OTTO_TRY(check_sessions(j.S, j.T));
    OTTO_REQUIRE(j.d_pair_off && j.d_Out && j.d_loss_sum, "null argument");
    OTTO_REQUIRE(j.T == 0 || (j.d_tok_aid && j.d_tok_src && j.d_tok_left), "null plan array");
    OTTO_REQUIRE(dbow || j.d_In, "CBOW and PV-DM need In");
    OTTO_REQUIRE(!doc || (j.d_Doc && j.d_tok_off), "PV-DM and DBOW need Doc and tok_off");
    const bool hs = j.d_path_off || j.d_path_node || j.d_code;
    if (hs) OTTO_TRY(check_paths(j.d_path_off, j.d_path_node, j.d_code, j.d_Syn1, j.n_inner));
    OTTO_REQUIRE(!batch || (j.d_gout && (dbow || j.d_gin) && (!doc || j.d_gdoc) && (!hs || j.d_gsyn1)),
                 "BATCH mode needs the gradient workspaces of its arch");
    SgCbowArgs a;
    memset(&a, 0, sizeof a);
    OTTO_TRY(table_or_size(j.table, neg, j.n_aids, &a.tab));
    hipStream_t s = (hipStream_t)j.stream;
    if (j.t0 == j.t1) {
        OTTO_HIP(hipMemsetAsync(j.d_loss_sum, 0, sizeof(double), s));
        return 0;
    }
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_SGNS_STEP, (size_t)SG_GRID * sizeof(double), &scratch, s));
    a.tok_aid = j.d_tok_aid; a.tok_src = j.d_tok_src; a.tok_left = j.d_tok_left; a.pair_off = j.d_pair_off; a.tok_off = j.d_tok_off;
    a.T = j.T; a.S = j.S; a.t0 = j.t0; a.t1 = j.t1; a.In = j.d_In; a.Out = j.d_Out; a.Syn1 = j.d_Syn1; a.Doc = j.d_Doc;
    a.d = d; a.G = d / 4; a.neg = neg; a.variant = j.variant; a.lr = j.lr; a.base = sg_base(j.seed, j.epoch);
    a.partial = reinterpret_cast<double*>(scratch); a.neg_out = neg > 0 ? j.d_neg_out : nullptr;
    a.gin = j.d_gin; a.gout = j.d_gout; a.gsyn1 = j.d_gsyn1; a.gdoc = j.d_gdoc;
    if (hs) { a.path_off = j.d_path_off; a.path_node = j.d_path_node; a.code = j.d_code; a.n_inner = (uint32_t)j.n_inner; }
    // DBOW: at most one session per token of the range meets it
    int threads;
    const int grid = launch_dims(a.G, dbow ? (j.S < j.t1 - j.t0 ? j.S : j.t1 - j.t0) : j.t1 - j.t0, &threads);
    if (!batch && hs) launch_cbow<false, true>(arch, grid, threads, s, a);
    else if (!batch) launch_cbow<false, false>(arch, grid, threads, s, a);
    else if (hs) launch_cbow<true, true>(arch, grid, threads, s, a);
    else launch_cbow<true, false>(arch, grid, threads, s, a);
    return apply_and_sum(batch, {{dbow ? nullptr : j.d_In, j.d_gin, j.n_aids}, {j.d_Out, j.d_gout, j.n_aids},
                                 {hs ? j.d_Syn1 : nullptr, j.d_gsyn1, j.n_inner}, {doc ? j.d_Doc : nullptr, j.d_gdoc, j.S}},
                         d, a.partial, grid, j.d_loss_sum, s);
}

extern "C" int otto_sgns_infer(const otto_sgns_infer_job* job) {
    OTTO_REQUIRE(job, "null job");
    const otto_sgns_infer_job& j = *job;
    const int arch = j.arch, d = j.d, neg = j.neg;
    OTTO_REQUIRE(arch == OTTO_SGNS_ARCH_PVDM || arch == OTTO_SGNS_ARCH_DBOW, "arch %d: inference is PV-DM or PV-DBOW", arch);
    const bool dm = arch == OTTO_SGNS_ARCH_PVDM;
    OTTO_REQUIRE(j.variant == OTTO_SGNS_CBOW_SUM || j.variant == OTTO_SGNS_CBOW_MEAN || j.variant == OTTO_SGNS_CBOW_FASTTEXT,
                 "unknown variant %d", j.variant);
    OTTO_TRY(check_shape(d, neg));
    OTTO_REQUIRE(j.ws >= 1 && j.ws <= OTTO_SGNS_MAX_WS, "ws = %d outside [1, %d]", j.ws, OTTO_SGNS_MAX_WS);
    OTTO_REQUIRE(j.passes >= 1 && j.passes <= OTTO_SGNS_MAX_INFER_PASSES, "passes = %d outside [1, %d]", j.passes,
                 OTTO_SGNS_MAX_INFER_PASSES);
    OTTO_TRY(check_n_aids(j.n_aids));
    OTTO_TRY(check_sessions(j.S, j.T));
    OTTO_REQUIRE(j.d_tok_off && j.d_Out && j.d_Doc && (j.T == 0 || j.d_tok_aid), "null argument");
    OTTO_REQUIRE(!dm || j.d_In, "PV-DM needs In");
    const bool hs = j.d_path_off || j.d_path_node || j.d_code;
    if (hs) OTTO_TRY(check_paths(j.d_path_off, j.d_path_node, j.d_code, j.d_Syn1, j.n_inner));
    OTTO_REQUIRE(neg > 0 || hs, "neg = 0 without hierarchical-softmax tables leaves nothing to infer against");
    SgInferArgs a;
    memset(&a, 0, sizeof a);
    OTTO_TRY(table_or_size(j.table, neg, j.n_aids, &a.tab));
    if (j.S == 0) return 0;
    a.tok_aid = j.d_tok_aid; a.tok_off = j.d_tok_off; a.sess_key = j.d_sess_key; a.order = j.d_order; a.T = j.T; a.S = j.S;
    a.In = j.d_In; a.Out = j.d_Out; a.Syn1 = j.d_Syn1; a.Doc = j.d_Doc; a.loss = j.d_loss;
    a.neg_out = neg > 0 ? j.d_neg_out : nullptr; a.radius_out = dm ? j.d_radius_out : nullptr;
    a.d = d; a.G = d / 4; a.neg = neg; a.ws = j.ws; a.variant = j.variant; a.passes = j.passes;
    if (hs) { a.path_off = j.d_path_off; a.path_node = j.d_path_node; a.code = j.d_code; a.n_inner = (uint32_t)j.n_inner; }
    for (int p = 0; p < j.passes; ++p) {
        a.lr[p] = j.lr[p];
        a.base[p] = sg_base(j.seed, (uint64_t)p);
    }
    hipStream_t s = (hipStream_t)j.stream;
    int threads;
    const int grid = launch_dims(a.G, j.S, &threads);
    if (a.neg_out || a.radius_out) launch_infer<true>(hs, dm, grid, threads, s, a);
    else launch_infer<false>(hs, dm, grid, threads, s, a);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_sgns_hs_tree_sizes(const int64_t* count, int64_t n_aids, int64_t min_count, int64_t* sizes) {
    OTTO_REQUIRE(sizes, "null argument");
    try {
        SgTree t;
        OTTO_TRY(sgns_hs_build(count, n_aids, min_count, &t));
        sizes[0] = t.V; sizes[1] = t.sum_len; sizes[2] = t.max_len;
    } catch (const std::bad_alloc&) {
        set_error("otto_sgns_hs_tree_sizes: out of host memory");
        return OTTO_ENOMEM;
    }
    return 0;
}

extern "C" int otto_sgns_hs_tree(const int64_t* count, int64_t n_aids, int64_t min_count, int64_t* path_off, int32_t* path_node,
                                 int64_t cap_nodes, uint64_t* code) {
    OTTO_REQUIRE(path_off && code && cap_nodes >= 0 && (cap_nodes == 0 || path_node), "null argument");
    try {
        SgTree t;
        OTTO_TRY(sgns_hs_build(count, n_aids, min_count, &t));
        OTTO_REQUIRE(t.max_len <= 64, "the longest Huffman path has %lld nodes, a code word holds 64", (long long)t.max_len);
        OTTO_REQUIRE(t.sum_len <= cap_nodes, "path_node: %lld ids, room for %lld", (long long)t.sum_len, (long long)cap_nodes);
        const int64_t V = t.V;
        for (int64_t a = 0; a <= n_aids; ++a) path_off[a] = 0;
        for (int64_t a = 0; a < n_aids; ++a) code[a] = 0;
        if (V < 2) return 0;
        for (int64_t i = 0; i < V; ++i) path_off[t.leaf_aid[i] + 1] = t.depth[i];
        for (int64_t a = 0; a < n_aids; ++a) path_off[a + 1] += path_off[a];
        for (int64_t i = 0; i < V; ++i) {
            // from the leaf up: the node at depth j - 1 is path node j - 1, the child below it carries bit j - 1
            int32_t* row = path_node + path_off[t.leaf_aid[i]];
            uint64_t cw = 0;
            int64_t n = i;
            for (int j = t.depth[i]; j > 0; --j) {
                cw |= (uint64_t)t.bit[n] << (j - 1);
                n = t.parent[n];
                row[j - 1] = (int32_t)(n - V);
            }
            code[t.leaf_aid[i]] = cw;
        }
    } catch (const std::bad_alloc&) {
        set_error("otto_sgns_hs_tree: out of host memory");
        return OTTO_ENOMEM;
    }
    return 0;
}
