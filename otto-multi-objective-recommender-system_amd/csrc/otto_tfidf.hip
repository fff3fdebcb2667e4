// TF-IDF similarity model for MI355X (gfx950): document-term counts, weights, transpose and the sparse cosine top-k. C-ABI and
// SPEC-TFIDF in include/otto_tfidf.h.
//
//   k_fit_keys     one thread per token: its document by binary search in doc_off, key = document << 32 | aid (a dropped or
//                  refused token gets document D, which sorts behind every entry); the radix sort of radix.h orders them.
//   k_fit_heads    a sorted token is a head where its key differs from the previous one: one matrix entry. df by integer
//                  atomics (order-free). The scan of the head flags places the entries; k_fit_row_off reads row_off out of it
//                  by binary search for every document's first key.
//   k_fit_start / k_fit_emit   fill: the heads write where their run starts, an entry's tf is the distance to the next start.
//   k_weights      one wave per row; 64 entries at a time are loaded side by side and their squares folded one after the
//                  other, in column order, by every lane alike.
//   k_tr_keys / k_tr_emit      transpose: key = column << 32 | row, value = the entry's position, the same sort.
//   k_cos_plan     one wave per query: the candidate bound (sum of the AT row lengths over q's columns) and the tier.
//   k_cos_small    one wave per query, four to a workgroup. Accumulators in an LDS hash table (linear probing, bounded by the
//                  table's size; at most half full because the bound is at most OTTO_TFIDF_SMALL_CAP).
//   k_cos_large    one 256-thread workgroup per query, taken from a counter; accumulators in the workgroup's dense float64 [R]
//                  row of the workspace, which the workgroup clears before its first query and every query leaves zeroed
//                  behind it; a call without a large query writes none of these rows.
// Both cosine kernels take q's columns in ascending order with a barrier in between and add one product per row and column:
// the sums come out in SPEC's order. Contraction is off for the whole file: a * b + c stays two rounded operations (HIP's
// __dmul_rn / __dadd_rn are plain operators in the headers and would be fused like any other).
#include "common.h"
#include "radix.h"
#include "topk.h"
#include "../../include/otto_tfidf.h"

#include <math.h>

#pragma clang fp contract(off)

namespace otto {
namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_WAVES = TF_THREADS / WAVE;
constexpr int COS_SLOTS = 2 * OTTO_TFIDF_SMALL_CAP;              // LDS hash slots of one small-tier wave (a power of two)
constexpr int COS_MPL = COS_SLOTS / WAVE;                        // slots one lane reads in the selection
constexpr int64_t COS_ACC_BUDGET = 2ll << 30;                    // bytes of dense accumulators the large tier asks for at most
static_assert((COS_SLOTS & (COS_SLOTS - 1)) == 0 && COS_SLOTS % WAVE == 0, "the hash mask and the selection need this");

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TF_THREADS - 1) / TF_THREADS); }

// first position of the sorted keys whose upper half is >= d
__device__ __forceinline__ int64_t first_of_row(const uint64_t* key, int64_t n, uint64_t d) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((key[mid] >> 32) < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Ctrl {                                                    // the first 256 bytes of every workspace here
    unsigned long long err;                                      // smallest offending index, ~0 without one
    unsigned long long key_bits[2];                              // key_bits_fold
    unsigned long long n_kept;                                   // fit: sorted tokens in front of the dropped ones
    unsigned int n_small, n_large, next;                         // cosine: tier sizes, the large tier's query counter
};

// ---------------------------------------------------------------------------------------------------------------------
// count / fill
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TF_THREADS) void k_fit_keys(const int32_t* __restrict__ tok, const int64_t* __restrict__ doc_off, int64_t E,
                                                         int64_t D, int64_t n_aids, int32_t min_aid, uint64_t* key, uint32_t* val,
                                                         Ctrl* ctrl) {
    const int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    unsigned long long vo = 0, va = ~0ull;
    if (i < E) {
        const int32_t a = tok[i];
        uint64_t k = (uint64_t)D << 32;                          // dropped: behind every document
        if (a < 0 || a >= n_aids) {
            atomicMin(&ctrl->err, (unsigned long long)i);
        } else if (a >= min_aid) {
            const int64_t d = segment_of(doc_off, D, i);
            k = (uint64_t)d << 32 | (uint32_t)a;
        }
        key[i] = k;
        val[i] = 0u;
        vo = va = k;
    }
    key_bits_fold(vo, va, ctrl->key_bits);
}

__global__ __launch_bounds__(TF_THREADS) void k_fit_heads(const uint64_t* __restrict__ key, int64_t E, int64_t D, uint8_t* flag, int32_t* df) {
    const int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (i >= E) return;
    const uint64_t k = key[i];
    const bool head = (k >> 32) < (uint64_t)D && (i == 0 || key[i - 1] != k);
    flag[i] = head;
    if (head) atomicAdd(&df[(uint32_t)k], 1);                    // the aid passed k_fit_keys' range check
}

__global__ __launch_bounds__(TF_THREADS) void k_fit_row_off(const uint64_t* __restrict__ key, const uint64_t* __restrict__ pos, int64_t E,
                                                            int64_t D, int64_t* row_off, Ctrl* ctrl) {
    const int64_t d = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (d > D) return;
    const int64_t i = first_of_row(key, E, (uint64_t)d);
    row_off[d] = (int64_t)pos[i];                                // pos has E + 1 entries
    if (d == D) ctrl->n_kept = (unsigned long long)i;
}

__global__ __launch_bounds__(TF_THREADS) void k_fit_start(const uint8_t* __restrict__ flag, const uint64_t* __restrict__ pos, int64_t E,
                                                          uint64_t* start, const Ctrl* ctrl) {
    const int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (i >= E) return;
    if (flag[i]) start[pos[i]] = (uint64_t)i;                    // pos[i] < nnz <= E
    if (i == 0) start[pos[E]] = ctrl->n_kept;                    // start has E + 1 entries
}

__global__ __launch_bounds__(TF_THREADS) void k_fit_emit(const uint64_t* __restrict__ key, const uint64_t* __restrict__ start,
                                                         const uint64_t* __restrict__ pos, int64_t E, int64_t nnz, int32_t* col, int32_t* tf) {
    const int64_t p = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (p >= nnz || (uint64_t)p >= pos[E]) return;               // never past what count found
    const uint64_t s = start[p];
    col[p] = (int32_t)(uint32_t)key[s];
    tf[p] = (int32_t)(start[p + 1] - s);
}

struct FitWs {
    Ctrl* ctrl;
    RadixWs r;
    uint8_t* flag;
    uint64_t* start;
};

size_t fit_layout(int64_t E, char* base, FitWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    FitWs t;
    t.ctrl = (Ctrl*)take(sizeof(Ctrl));
    o += radix_ws_layout(E, false, base ? base + o : nullptr, &t.r);
    t.flag = (uint8_t*)take((size_t)E);
    t.start = (uint64_t*)take(((size_t)E + 1) * 8);
    if (w) *w = t;
    return o;
}

int fit_check(const otto_tfidf_fit_job* j) {
    OTTO_REQUIRE(j, "otto_tfidf: null job");
    OTTO_REQUIRE(j->n_tokens >= 0 && j->n_tokens < (1ll << 31), "otto_tfidf: n_tokens must be in [0, 2^31) (got %lld)", (long long)j->n_tokens);
    OTTO_REQUIRE(j->n_docs >= 0 && j->n_docs < (1ll << 31) - 1, "otto_tfidf: n_docs must be in [0, 2^31 - 1) (got %lld)", (long long)j->n_docs);
    OTTO_REQUIRE(j->n_aids >= 0 && j->n_aids < (1ll << 31), "otto_tfidf: n_aids must be in [0, 2^31) (got %lld)", (long long)j->n_aids);
    OTTO_REQUIRE(j->min_aid >= 0, "otto_tfidf: min_aid must not be negative (got %d)", j->min_aid);
    OTTO_REQUIRE(j->reserved == 0, "otto_tfidf: reserved must be 0");
    OTTO_REQUIRE(j->n_docs > 0 || j->n_tokens == 0, "otto_tfidf: tokens without a document");
    return 0;
}

int fit_ws(const otto_tfidf_fit_job& j, const char* who, FitWs* w) {
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0, "%s: a 256-byte aligned workspace is needed", who);
    const int64_t need = (int64_t)fit_layout(j.n_tokens, nullptr, nullptr);
    OTTO_REQUIRE(j.work_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)j.work_bytes, (long long)need);
    fit_layout(j.n_tokens, (char*)j.d_work, w);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TF_THREADS) void k_weights(const int64_t* __restrict__ row_off, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ tf, const double* __restrict__ idf, double* val,
                                                        int64_t n_rows, int64_t n_cols) {
    const int lane = (int)lane_id();
    const int64_t waves = (int64_t)gridDim.x * TF_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * TF_WAVES + (threadIdx.x >> 6); r < n_rows; r += waves) {      // wave-uniform
        const int64_t beg = row_off[r], end = row_off[r + 1];
        auto weight = [&](int64_t p) {
            if (!idf) return val[p];
            const int32_t c = col[p];
            return (uint32_t)c < (uint64_t)n_cols ? (double)tf[p] * idf[c] : 0.0;
        };
        double ss = 0.0;
        for (int64_t base = beg; base < end; base += WAVE) {
            const int64_t p = base + lane;
            const double w = p < end ? weight(p) : 0.0;
            const double sq = w * w;
            const int cnt = end - base < WAVE ? (int)(end - base) : WAVE;
            for (int t = 0; t < cnt; ++t) ss = ss + __shfl(sq, t, 64);       // column order; every lane folds the same sum
        }
        const double norm = sqrt(ss);
        for (int64_t p = beg + lane; p < end; p += WAVE) {
            const double w = weight(p);                          // in place: only this lane has touched val[p]
            val[p] = norm > 0.0 ? w / norm : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// transpose
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TF_THREADS) void k_tr_keys(const int64_t* __restrict__ off, const int32_t* __restrict__ idx, int64_t R, int64_t C,
                                                        int64_t nnz, uint64_t* key, uint32_t* val, Ctrl* ctrl) {
    const int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    unsigned long long vo = 0, va = ~0ull;
    if (i < nnz) {
        const int32_t c = idx[i];
        uint64_t k = (uint64_t)C << 32;
        if (c < 0 || c >= C) {
            atomicMin(&ctrl->err, (unsigned long long)i);
        } else {
            const int64_t r = segment_of(off, R, i);
            k = (uint64_t)c << 32 | (uint32_t)r;
        }
        key[i] = k;
        val[i] = (uint32_t)i;
        vo = va = k;
    }
    key_bits_fold(vo, va, ctrl->key_bits);
}

__global__ __launch_bounds__(TF_THREADS) void k_tr_emit(const uint64_t* __restrict__ key, const uint32_t* __restrict__ src,
                                                        const double* __restrict__ val, int64_t nnz, int64_t C, int32_t* t_idx, double* t_val) {
    const int64_t p = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t k = key[p];
    if ((k >> 32) >= (uint64_t)C) return;                        // a refused entry
    t_idx[p] = (int32_t)(uint32_t)k;
    t_val[p] = val[src[p]];                                      // src[p] < nnz: it is an entry's position
}

__global__ __launch_bounds__(TF_THREADS) void k_tr_off(const uint64_t* __restrict__ key, int64_t nnz, int64_t C, int64_t* t_off) {
    const int64_t c = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (c <= C) t_off[c] = first_of_row(key, nnz, (uint64_t)c);
}

struct TrWs {
    Ctrl* ctrl;
    RadixWs r;
};

size_t tr_layout(int64_t nnz, char* base, TrWs* w) {
    TrWs t;
    t.ctrl = (Ctrl*)base;
    const size_t o = align256(sizeof(Ctrl));
    const size_t total = o + radix_ws_layout(nnz, false, base ? base + o : nullptr, &t.r);
    if (w) *w = t;
    return total;
}

int tr_check(const otto_tfidf_transpose_job* j) {
    OTTO_REQUIRE(j, "otto_tfidf_transpose: null job");
    OTTO_REQUIRE(j->n_rows >= 0 && j->n_rows < (1ll << 31), "otto_tfidf_transpose: n_rows must be in [0, 2^31) (got %lld)", (long long)j->n_rows);
    OTTO_REQUIRE(j->n_cols >= 0 && j->n_cols < (1ll << 31), "otto_tfidf_transpose: n_cols must be in [0, 2^31) (got %lld)", (long long)j->n_cols);
    OTTO_REQUIRE(j->nnz >= 0 && j->nnz < (1ll << 32), "otto_tfidf_transpose: nnz must be in [0, 2^32) (got %lld)", (long long)j->nnz);
    OTTO_REQUIRE(j->n_rows > 0 || j->nnz == 0, "otto_tfidf_transpose: entries without a row");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// cosine top-k
// ---------------------------------------------------------------------------------------------------------------------
struct CosArgs {
    const int64_t* a_off;
    const int32_t* a_idx;
    const double* a_val;
    const int64_t* t_off;
    const int32_t* t_idx;
    const double* t_val;
    int64_t R, C;
    const int32_t* queries;
    int64_t nq;
    int k, exclude_self;
    int32_t* ids;
    double* sim;
    int32_t* n;
};

// One column of a query's row: its index, A's value there, and AT's postings [tb, te). An index outside [0, C) has none.
struct CosColumn {
    double v;
    int64_t tb, te;
};
__device__ __forceinline__ CosColumn cos_column(const CosArgs& a, int64_t p, int64_t end) {
    CosColumn col = {0.0, 0, 0};
    if (p < end) {
        const int32_t c = a.a_idx[p];
        col.v = a.a_val[p];
        if ((uint32_t)c < (uint64_t)a.C) {
            col.tb = a.t_off[c];
            col.te = a.t_off[c + 1];
        }
    }
    return col;
}

// lane i holds the i-th best: the query's output row, padding included
__device__ __forceinline__ void cos_store(const CosArgs& a, int64_t qi, KeyW best) {
    const int lane = (int)lane_id();
    const bool valid = lane < a.k && kvalid(best);
    const unsigned long long m = __ballot(valid);
    if (lane < a.k) {
        a.ids[qi * a.k + lane] = valid ? (int32_t)best.y : -1;
        a.sim[qi * a.k + lane] = valid ? __longlong_as_double((long long)best.w) : 0.0;
    }
    if (lane == 0) a.n[qi] = __popcll(m);
}

__global__ __launch_bounds__(TF_THREADS) void k_cos_plan(CosArgs a, Ctrl* ctrl, int32_t* small, int32_t* large) {
    const int lane = (int)lane_id();
    const int64_t waves = (int64_t)gridDim.x * TF_WAVES;
    for (int64_t qi = (int64_t)blockIdx.x * TF_WAVES + (threadIdx.x >> 6); qi < a.nq; qi += waves) {     // wave-uniform
        const int32_t q = __builtin_amdgcn_readfirstlane(a.queries[qi]);
        if (q < 0 || q >= a.R) {
            if (lane == 0) atomicMin(&ctrl->err, (unsigned long long)qi);
            KeyW none;
            kclear(none);
            cos_store(a, qi, none);
            continue;
        }
        const int64_t beg = a.a_off[q], end = a.a_off[q + 1];
        unsigned long long bound = 0;
        for (int64_t p = beg + lane; p < end; p += WAVE) {
            const int32_t c = a.a_idx[p];
            if ((uint32_t)c < (uint64_t)a.C) bound += (unsigned long long)(a.t_off[c + 1] - a.t_off[c]);
        }
        bound = wave_reduce<Sum>(bound);
        if (lane == 0) {
            if (bound <= (unsigned long long)OTTO_TFIDF_SMALL_CAP) small[atomicAdd(&ctrl->n_small, 1u)] = (int32_t)qi;      // < nq entries each
            else large[atomicAdd(&ctrl->n_large, 1u)] = (int32_t)qi;
        }
    }
}

__global__ __launch_bounds__(TF_THREADS) void k_cos_small(CosArgs a, const Ctrl* ctrl, const int32_t* __restrict__ small) {
    __shared__ int32_t s_key[TF_WAVES][COS_SLOTS];
    __shared__ double s_acc[TF_WAVES][COS_SLOTS];
    const int lane = (int)lane_id(), w = threadIdx.x >> 6;
    int32_t* keys = s_key[w];
    double* acc = s_acc[w];
    const int64_t waves = (int64_t)gridDim.x * TF_WAVES;
    const int64_t n_small = ctrl->n_small;
    for (int64_t i = (int64_t)blockIdx.x * TF_WAVES + w; i < n_small; i += waves) {                      // wave-uniform
        const int64_t qi = small[i];
        const int32_t q = __builtin_amdgcn_readfirstlane(a.queries[qi]);                               // in range: the plan filed it
        for (int s = lane; s < COS_SLOTS; s += WAVE) {
            keys[s] = -1;
            acc[s] = 0.0;
        }
        wave_lds_sync();
        const int64_t beg = a.a_off[q], end = a.a_off[q + 1];
        CosColumn next = cos_column(a, beg, end);
        for (int64_t p = beg; p < end; ++p) {                    // q's columns, ascending: SPEC's order
            const CosColumn col = next;
            next = cos_column(a, p + 1, end);                    // its loads are in flight while this column's postings are added
            for (int64_t pp = col.tb + lane; pp < col.te; pp += WAVE) {
                const int32_t j = a.t_idx[pp];
                if ((uint32_t)j >= (uint64_t)a.R) continue;
                const double prod = col.v * a.t_val[pp];
                uint32_t h = ((uint32_t)j * 2654435761u) >> 16 & (COS_SLOTS - 1);
                for (int probe = 0; probe < COS_SLOTS; ++probe) {                                      // bounded by the capacity
                    const int32_t seen = atomicCAS(&keys[h], -1, j);
                    if (seen == -1 || seen == j) {
                        acc[h] = acc[h] + prod;                  // a row occurs once per column: this lane alone is at slot h
                        break;
                    }
                    h = (h + 1) & (COS_SLOTS - 1);
                }
            }
            wave_lds_sync();                                     // the next column's lanes read what this column's wrote
        }
        KeyW cand[COS_MPL], best;
#pragma unroll
        for (int t = 0; t < COS_MPL; ++t) {
            const int32_t j = keys[lane + t * WAVE];
            const double s = acc[lane + t * WAVE];
            kclear(cand[t]);
            if (j >= 0 && s > 0.0 && !(a.exclude_self && j == q)) cand[t] = {(uint64_t)__double_as_longlong(s), (uint32_t)j};
        }
        wave_topk_select<COS_MPL>(cand, a.k, best);
        cos_store(a, qi, best);
        wave_lds_sync();                                         // the table is cleared for the next query after these reads
    }
}

__global__ __launch_bounds__(TF_THREADS) void k_cos_large(CosArgs a, Ctrl* ctrl, const int32_t* __restrict__ large, double* acc_rows) {
    __shared__ unsigned int s_next;
    __shared__ uint64_t s_w[TF_WAVES][WAVE];
    __shared__ uint32_t s_y[TF_WAVES][WAVE];
    const int lane = (int)lane_id(), w = threadIdx.x >> 6;
    double* acc = acc_rows + (int64_t)blockIdx.x * a.R;           // all zero between two queries
    const unsigned int n_large = ctrl->n_large;
    bool clean = false;                                          // the row holds what the last call left: cleared before the first query
    for (;;) {
        if (threadIdx.x == 0) s_next = atomicAdd(&ctrl->next, 1u);
        __syncthreads();
        const unsigned int i = s_next;
        __syncthreads();
        if (i >= n_large) break;                                 // workgroup-uniform; a workgroup without a query touches nothing
        if (!clean) {
            for (int64_t j = threadIdx.x; j < a.R; j += TF_THREADS) acc[j] = 0.0;
            clean = true;
            __syncthreads();
        }
        const int64_t qi = large[i];
        const int32_t q = a.queries[qi];
        const int64_t beg = a.a_off[q], end = a.a_off[q + 1];
        CosColumn next = cos_column(a, beg, end);
        for (int64_t p = beg; p < end; ++p) {                    // q's columns, ascending: SPEC's order
            const CosColumn col = next;
            next = cos_column(a, p + 1, end);                    // its loads are in flight while this column's postings are added
            for (int64_t pp = col.tb + threadIdx.x; pp < col.te; pp += TF_THREADS) {
                const int32_t j = a.t_idx[pp];
                if ((uint32_t)j < (uint64_t)a.R) acc[j] = acc[j] + col.v * a.t_val[pp];                // a row occurs once per column
            }
            __syncthreads();                                     // the next column's threads read what this column's wrote
        }
        KeyW best;
        kclear(best);
        next = cos_column(a, beg, end);
        for (int64_t p = beg; p < end; ++p) {                    // the same walk again: the first visit of a row takes its sum and zeroes it
            const CosColumn col = next;
            next = cos_column(a, p + 1, end);
            for (int64_t base = col.tb; base < col.te; base += TF_THREADS) {                           // workgroup-uniform trip count
                const int64_t pp = base + threadIdx.x;
                KeyW cand;
                kclear(cand);
                if (pp < col.te) {
                    const int32_t j = a.t_idx[pp];
                    if ((uint32_t)j < (uint64_t)a.R) {
                        const double s = acc[j];
                        if (s != 0.0) {
                            acc[j] = 0.0;
                            if (s > 0.0 && !(a.exclude_self && j == q)) cand = {(uint64_t)__double_as_longlong(s), (uint32_t)j};
                        }
                    }
                }
                wave_topk_push(best, cand, a.k);
            }
            __syncthreads();
        }
        s_w[w][lane] = best.w;
        s_y[w][lane] = best.y;
        __syncthreads();
        if (w == 0) {
            for (int o = 1; o < TF_WAVES; ++o) {
                KeyW cand;
                kload(cand, s_w[o][lane], s_y[o][lane]);
                wave_topk_push(best, cand, a.k);
            }
            cos_store(a, qi, best);
        }
        __syncthreads();                                         // the lists are read before the next query overwrites them
    }
}

struct CosWs {
    Ctrl* ctrl;
    int32_t* small;
    int32_t* large;
    double* acc;
    int64_t groups;
};

size_t cos_layout(int64_t nq, int64_t R, char* base, CosWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    CosWs t;
    int64_t g = R > 0 ? COS_ACC_BUDGET / (8 * R) : 1;
    g = g > OTTO_TFIDF_MAX_GROUPS ? OTTO_TFIDF_MAX_GROUPS : g;
    g = g > nq ? nq : g;
    t.groups = g < 1 ? 1 : g;
    t.ctrl = (Ctrl*)take(sizeof(Ctrl));
    t.small = (int32_t*)take((size_t)nq * 4);
    t.large = (int32_t*)take((size_t)nq * 4);
    t.acc = (double*)take((size_t)t.groups * (size_t)R * 8);
    if (w) *w = t;
    return o;
}

int cos_check(const otto_tfidf_cosine_job* j) {
    OTTO_REQUIRE(j, "otto_tfidf_cosine: null job");
    OTTO_REQUIRE(j->n_rows >= 0 && j->n_rows < (1ll << 31), "otto_tfidf_cosine: n_rows must be in [0, 2^31) (got %lld)", (long long)j->n_rows);
    OTTO_REQUIRE(j->n_cols >= 0 && j->n_cols < (1ll << 31), "otto_tfidf_cosine: n_cols must be in [0, 2^31) (got %lld)", (long long)j->n_cols);
    OTTO_REQUIRE(j->n_queries >= 0 && j->n_queries < (1ll << 31), "otto_tfidf_cosine: n_queries must be in [0, 2^31) (got %lld)",
                 (long long)j->n_queries);
    OTTO_REQUIRE(j->k >= 1 && j->k <= OTTO_TFIDF_MAX_K, "otto_tfidf_cosine: k must be in [1, %d] (got %d)", OTTO_TFIDF_MAX_K, j->k);
    OTTO_REQUIRE(j->exclude_self == 0 || j->exclude_self == 1, "otto_tfidf_cosine: exclude_self must be 0 or 1 (got %d)", j->exclude_self);
    return 0;
}

int init_ctrl(Ctrl* ctrl, hipStream_t s) {
    OTTO_HIP(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
    OTTO_HIP(hipMemsetAsync(&ctrl->err, 0xFF, 8, s));
    OTTO_HIP(hipMemsetAsync(&ctrl->key_bits[1], 0xFF, 8, s));    // the AND of the keys starts at all ones
    return 0;
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_tfidf_fit_workspace(const otto_tfidf_fit_job* job) {
    if (fit_check(job) != 0) return -22;
    return (int64_t)fit_layout(job->n_tokens, nullptr, nullptr);
}

extern "C" int otto_tfidf_count(const otto_tfidf_fit_job* job, int64_t* h_nnz, int64_t* h_err) {
    OTTO_REQUIRE(h_nnz && h_err, "otto_tfidf_count: null h_nnz or h_err");
    *h_nnz = 0;
    h_err[0] = -1;
    OTTO_TRY(fit_check(job));
    const otto_tfidf_fit_job& j = *job;
    const int64_t E = j.n_tokens, D = j.n_docs;
    OTTO_REQUIRE(j.d_row_off, "otto_tfidf_count: null row_off");
    OTTO_REQUIRE(j.n_aids == 0 || j.d_df, "otto_tfidf_count: null df");
    OTTO_REQUIRE(E == 0 || (j.d_tok_aid && j.d_doc_off), "otto_tfidf_count: null input");
    hipStream_t s = (hipStream_t)j.stream;
    if (j.n_aids > 0) OTTO_HIP(hipMemsetAsync(j.d_df, 0, (size_t)j.n_aids * 4, s));
    if (E == 0) {
        OTTO_HIP(hipMemsetAsync(j.d_row_off, 0, (size_t)(D + 1) * 8, s));
        OTTO_HIP(hipStreamSynchronize(s));
        return 0;
    }
    FitWs w;
    OTTO_TRY(fit_ws(j, "otto_tfidf_count", &w));
    OTTO_TRY(init_ctrl(w.ctrl, s));
    k_fit_keys<<<blocks_for(E), TF_THREADS, 0, s>>>(j.d_tok_aid, j.d_doc_off, E, D, j.n_aids, j.min_aid, w.r.key[0], w.r.val[0], w.ctrl);
    OTTO_HIP(hipGetLastError());
    int cur = 0;                                                 // all eight passes are launched, an even number: the sorted keys end in buffer 0
    OTTO_TRY((radix_passes<false>(w.r, E, ~0ull, SkipOnDevice{w.ctrl->key_bits}, &cur, s)));
    k_fit_heads<<<blocks_for(E), TF_THREADS, 0, s>>>(w.r.key[0], E, D, w.flag, j.d_df);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(FlagAt{w.flag}, E, w.r.offs, w.r.partial, s));
    k_fit_row_off<<<blocks_for(D + 1), TF_THREADS, 0, s>>>(w.r.key[0], w.r.offs, E, D, j.d_row_off, w.ctrl);
    OTTO_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    OTTO_HIP(hipMemcpyAsync(&h[0], &w.ctrl->err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&h[1], w.r.offs + E, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (h[0] != ~0ull) {
        h_err[0] = (int64_t)h[0];
        OTTO_REQUIRE(false, "otto_tfidf_count: token %lld: aid outside [0, n_aids)", (long long)h_err[0]);
    }
    *h_nnz = (int64_t)h[1];
    return 0;
}

extern "C" int otto_tfidf_fill(const otto_tfidf_fit_job* job) {
    OTTO_TRY(fit_check(job));
    const otto_tfidf_fit_job& j = *job;
    const int64_t E = j.n_tokens;
    OTTO_REQUIRE(j.nnz >= 0 && j.nnz <= E, "otto_tfidf_fill: nnz must be in [0, n_tokens] (got %lld)", (long long)j.nnz);
    if (j.nnz == 0) return 0;
    OTTO_REQUIRE(j.d_col && j.d_tf, "otto_tfidf_fill: null output");
    hipStream_t s = (hipStream_t)j.stream;
    FitWs w;
    OTTO_TRY(fit_ws(j, "otto_tfidf_fill", &w));
    k_fit_start<<<blocks_for(E), TF_THREADS, 0, s>>>(w.flag, w.r.offs, E, w.start, w.ctrl);
    OTTO_HIP(hipGetLastError());
    k_fit_emit<<<blocks_for(j.nnz), TF_THREADS, 0, s>>>(w.r.key[0], w.start, w.r.offs, E, j.nnz, j.d_col, j.d_tf);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_tfidf_weights(const otto_tfidf_weights_job* job) {
    OTTO_REQUIRE(job, "otto_tfidf_weights: null job");
    const otto_tfidf_weights_job& j = *job;
    OTTO_REQUIRE(j.n_rows >= 0 && j.n_rows < (1ll << 31), "otto_tfidf_weights: n_rows must be in [0, 2^31) (got %lld)", (long long)j.n_rows);
    OTTO_REQUIRE(j.n_cols >= 0 && j.n_cols < (1ll << 31), "otto_tfidf_weights: n_cols must be in [0, 2^31) (got %lld)", (long long)j.n_cols);
    if (j.n_rows == 0) return 0;
    OTTO_REQUIRE(j.d_row_off, "otto_tfidf_weights: null row_off");           // col, tf and val may be null where every row is empty
    const int64_t blocks = (j.n_rows + TF_WAVES - 1) / TF_WAVES;
    k_weights<<<(unsigned)(blocks < 65536 ? blocks : 65536), TF_THREADS, 0, (hipStream_t)j.stream>>>(j.d_row_off, j.d_col, j.d_tf, j.d_idf, j.d_val,
                                                                                                   j.n_rows, j.n_cols);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t otto_tfidf_transpose_workspace(const otto_tfidf_transpose_job* job) {
    if (tr_check(job) != 0) return -22;
    return (int64_t)tr_layout(job->nnz, nullptr, nullptr);
}

extern "C" int otto_tfidf_transpose(const otto_tfidf_transpose_job* job, int64_t* h_err) {
    OTTO_REQUIRE(h_err, "otto_tfidf_transpose: null h_err");
    h_err[0] = -1;
    OTTO_TRY(tr_check(job));
    const otto_tfidf_transpose_job& j = *job;
    OTTO_REQUIRE(j.d_t_off, "otto_tfidf_transpose: null t_off");
    hipStream_t s = (hipStream_t)j.stream;
    if (j.nnz == 0) {
        OTTO_HIP(hipMemsetAsync(j.d_t_off, 0, (size_t)(j.n_cols + 1) * 8, s));
        OTTO_HIP(hipStreamSynchronize(s));
        return 0;
    }
    OTTO_REQUIRE(j.d_off && j.d_idx && j.d_val && j.d_t_idx && j.d_t_val, "otto_tfidf_transpose: null input or output");
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0, "otto_tfidf_transpose: a 256-byte aligned workspace is needed");
    const int64_t need = (int64_t)tr_layout(j.nnz, nullptr, nullptr);
    OTTO_REQUIRE(j.work_bytes >= need, "otto_tfidf_transpose: workspace too small (%lld < %lld)", (long long)j.work_bytes, (long long)need);
    TrWs w;
    tr_layout(j.nnz, (char*)j.d_work, &w);
    OTTO_TRY(init_ctrl(w.ctrl, s));
    k_tr_keys<<<blocks_for(j.nnz), TF_THREADS, 0, s>>>(j.d_off, j.d_idx, j.n_rows, j.n_cols, j.nnz, w.r.key[0], w.r.val[0], w.ctrl);
    OTTO_HIP(hipGetLastError());
    int cur = 0;
    OTTO_TRY((radix_passes<false>(w.r, j.nnz, ~0ull, SkipOnDevice{w.ctrl->key_bits}, &cur, s)));
    k_tr_emit<<<blocks_for(j.nnz), TF_THREADS, 0, s>>>(w.r.key[0], w.r.val[0], j.d_val, j.nnz, j.n_cols, j.d_t_idx, j.d_t_val);
    OTTO_HIP(hipGetLastError());
    k_tr_off<<<blocks_for(j.n_cols + 1), TF_THREADS, 0, s>>>(w.r.key[0], j.nnz, j.n_cols, j.d_t_off);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, &w.ctrl->err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != ~0ull) {
        h_err[0] = (int64_t)herr;
        OTTO_REQUIRE(false, "otto_tfidf_transpose: entry %lld: index outside [0, n_cols)", (long long)h_err[0]);
    }
    return 0;
}

extern "C" int64_t otto_tfidf_cosine_workspace(const otto_tfidf_cosine_job* job) {
    if (cos_check(job) != 0) return -22;
    return (int64_t)cos_layout(job->n_queries, job->n_rows, nullptr, nullptr);
}

extern "C" int otto_tfidf_cosine_topk(const otto_tfidf_cosine_job* job, int64_t* h_err) {
    OTTO_REQUIRE(h_err, "otto_tfidf_cosine_topk: null h_err");
    h_err[0] = -1;
    OTTO_TRY(cos_check(job));
    const otto_tfidf_cosine_job& j = *job;
    if (j.n_queries == 0) return 0;
    OTTO_REQUIRE(j.d_queries && j.d_ids && j.d_sim && j.d_n, "otto_tfidf_cosine_topk: null queries or output");
    OTTO_REQUIRE(j.d_a_off && j.d_t_off, "otto_tfidf_cosine_topk: null offsets");
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0, "otto_tfidf_cosine_topk: a 256-byte aligned workspace is needed");
    const int64_t need = (int64_t)cos_layout(j.n_queries, j.n_rows, nullptr, nullptr);
    OTTO_REQUIRE(j.work_bytes >= need, "otto_tfidf_cosine_topk: workspace too small (%lld < %lld)", (long long)j.work_bytes, (long long)need);
    CosWs w;
    cos_layout(j.n_queries, j.n_rows, (char*)j.d_work, &w);
    hipStream_t s = (hipStream_t)j.stream;
    OTTO_TRY(init_ctrl(w.ctrl, s));
    const CosArgs a = {j.d_a_off, j.d_a_idx, j.d_a_val, j.d_t_off, j.d_t_idx, j.d_t_val, j.n_rows, j.n_cols, j.d_queries, j.n_queries,
                       j.k, j.exclude_self, j.d_ids, j.d_sim, j.d_n};
    const int64_t blocks = (j.n_queries + TF_WAVES - 1) / TF_WAVES;
    const unsigned grid = (unsigned)(blocks < OTTO_TFIDF_SMALL_GRID ? blocks : OTTO_TFIDF_SMALL_GRID);
    k_cos_plan<<<grid, TF_THREADS, 0, s>>>(a, w.ctrl, w.small, w.large);
    OTTO_HIP(hipGetLastError());
    k_cos_small<<<grid, TF_THREADS, 0, s>>>(a, w.ctrl, w.small);
    OTTO_HIP(hipGetLastError());
    k_cos_large<<<(unsigned)w.groups, TF_THREADS, 0, s>>>(a, w.ctrl, w.large, w.acc);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, &w.ctrl->err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != ~0ull) {
        h_err[0] = (int64_t)herr;
        OTTO_REQUIRE(false, "otto_tfidf_cosine_topk: query %lld: row id outside [0, n_rows)", (long long)h_err[0]);
    }
    return 0;
}
