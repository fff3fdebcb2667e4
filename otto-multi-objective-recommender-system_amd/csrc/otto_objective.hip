// Objectives and metrics of the tree trainers (SPEC-OBJ; include/otto_objective.h). The per-query
// ranking is SPEC-GBDT's (gbdt_device.h), the sort is the shared (key u64, value u32) radix sort (sort.h), the prefix counts
// come from scan.h.
//
// Device, on the caller's stream:
//   k_obj_binary        grid-stride over the rows: one table lookup, two stores per row.
//   k_obj_label_counts  grid-stride count of the positives, one int64 atomic per wave.
//   k_obj_ndcg          one workgroup per query: rank_query, then one thread adds DCG and maxDCG in rank order (k_ap's shape).
//   k_auc_keys          (descending score key, label > 0) into the sort's first buffers.
//   k_auc_groups        after the sort and the scan of the positives: the head of every run of equal keys finds the run's
//                       end (galloping, then binary search) and adds its term; int64 atomics, so the order does not matter.
//   k_logloss_parts / k_logloss_final   a part of the rows per workgroup, whichever workgroup takes it; fixed trees.
#include "gbdt_device.h"
#include "scan.h"
#include "radix.h"
#include "sort.h"
#include "../../include/otto_events.h"
#include "../../include/otto_objective.h"

#include <math.h>

namespace otto {
namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_MAX_BLOCKS = 1024;    // of the grid-stride kernels: 4 workgroups on each of the 256 CUs
constexpr int PARTS = OTTO_OBJ_LOGLOSS_PARTS;

inline unsigned row_grid(int64_t n) {
    const int64_t b = (n + OBJ_THREADS - 1) / OBJ_THREADS;
    return (unsigned)(b < OBJ_MAX_BLOCKS ? b : OBJ_MAX_BLOCKS);
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_binary(const double* score, const int32_t* label, int64_t n, const double* table,
                                                            double t_lo, double factor, double sigma, double w_pos, double w_neg,
                                                            double floor_h, double* grad, double* hess, uint32_t* err) {
#pragma clang fp contract(off)
    const double top = (double)(OTTO_GBDT_SIGMOID_BINS - 1);
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OBJ_THREADS) {
        const int lab = label[i];
        if (lab < 0 || lab > OTTO_GBDT_MAX_LABEL) {
            bad = true;
            grad[i] = 0.0;
            hess[i] = 0.0;
            continue;
        }
        double x = (-(sigma * score[i]) - t_lo) * factor;
        x = x > 0.0 ? x : 0.0;                          // NaN -> 0
        x = x < top ? x : top;
        const double p = table[(size_t)x];
        const double t = lab > 0 ? 1.0 : 0.0;
        const double w = lab > 0 ? w_pos : w_neg;
        double h = sigma * sigma * p * (1.0 - p);
        h = h > floor_h ? h : floor_h;
        grad[i] = sigma * (p - t) * w;
        hess[i] = h * w;
    }
    if (bad) atomicOr(err + ERR_LABEL, 1u);
}

__global__ __launch_bounds__(OBJ_THREADS) void k_obj_label_counts(const int32_t* label, int64_t n, unsigned long long* counts) {
    unsigned long long pos = 0;
    for (int64_t i = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OBJ_THREADS)
        pos += label[i] > 0 ? 1ull : 0ull;
    pos = wave_reduce<Sum>(pos);
    if (lane_id() == 0 && pos) atomicAdd(counts, pos);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[1] = (unsigned long long)n;
}

__device__ __forceinline__ double label_gain(int lab) { return (double)((1ull << lab) - 1ull); }

__global__ __launch_bounds__(256) void k_obj_ndcg(const double* score, const int32_t* label, const int64_t* query_off, int64_t n, int k,
                                                  const double* discount, double* ndcg, uint32_t* err) {
#pragma clang fp contract(off)
    __shared__ QueryLds s;
    int64_t lo;
    int cnt;
    if (!query_range(query_off, blockIdx.x, n, &lo, &cnt, err)) {
        if (threadIdx.x == 0) ndcg[blockIdx.x] = -1.0;
        return;
    }
    const int top = k < cnt ? k : cnt;
    // the discounts the one adding thread needs, fetched by all: rank_query's barriers publish them
    for (int r = threadIdx.x; r < top; r += blockDim.x) s.disc[r] = discount[r];
    if (cnt > 0) rank_query(s, score, label, lo, cnt, err);
    if (threadIdx.x == 0) {
        double dcg = 0.0, best = 0.0;
        for (int r = 0; r < top; ++r) dcg = dcg + label_gain(s.label[r]) * s.disc[r];
        int r = 0;
        for (int lab = OTTO_GBDT_MAX_LABEL; lab >= 0 && r < top; --lab) {
            const double g = label_gain(lab);
            for (uint32_t c = s.lcnt[lab]; c > 0 && r < top; --c, ++r) best = best + g * s.disc[r];
        }
        ndcg[blockIdx.x] = best == 0.0 ? -1.0 : dcg / best;
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_auc_keys(const double* score, const int32_t* label, int64_t n, uint64_t* key,
                                                          uint32_t* val) {
    for (int64_t i = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OBJ_THREADS) {
        key[i] = ~score_key(score[i]);
        val[i] = label[i] > 0 ? 1u : 0u;
    }
}

struct PosFlag {
    const uint32_t* val;
    __device__ uint64_t operator()(int64_t i) const { return (uint64_t)val[i]; }
};

// ppre: n + 1 entries, ppre[n] = P
__global__ __launch_bounds__(OBJ_THREADS) void k_auc_groups(const uint64_t* key, const uint64_t* ppre, int64_t n, unsigned long long* out) {
    unsigned long long mine = 0;
    for (int64_t a = (int64_t)blockIdx.x * OBJ_THREADS + threadIdx.x; a < n; a += (int64_t)gridDim.x * OBJ_THREADS) {
        const uint64_t k = key[a];
        if (a > 0 && key[a - 1] == k) continue;         // not the head of its run
        // the run's end b: the first index in (a, n] whose key differs; key[lo] == k and (hi == n or key[hi] != k) throughout
        int64_t lo = a, hi = n, step = 1;
        while (lo + step < n) {
            if (key[lo + step] != k) { hi = lo + step; break; }
            lo += step;
            step <<= 1;
        }
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (key[mid] == k) lo = mid; else hi = mid;
        }
        const uint64_t pa = ppre[a], pb = ppre[hi];
        const uint64_t neg = (uint64_t)(hi - a) - (pb - pa);
        mine += neg * (pa + pb);
    }
    mine = wave_reduce<Sum>(mine);
    if (lane_id() == 0 && mine) atomicAdd(out, mine);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[1] = ppre[n];
        out[2] = (unsigned long long)n - ppre[n];
    }
}

__device__ __forceinline__ double block_tree_sum(double t, double* s) {
    s[threadIdx.x] = t;
    __syncthreads();
    for (int o = OBJ_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(OBJ_THREADS) void k_logloss_parts(const double* score, const int32_t* label, int64_t n, double sigma,
                                                               int64_t per, double* partial) {
#pragma clang fp contract(off)
    __shared__ double s[OBJ_THREADS];
    for (int part = blockIdx.x; part < PARTS; part += gridDim.x) {
        const int64_t i0 = (int64_t)part * per;
        const int64_t i1 = i0 + per < n ? i0 + per : n;
        double t = 0.0;
        for (int64_t i = i0 + threadIdx.x; i < i1; i += OBJ_THREADS) {
            const double m = sigma * score[i];
            const double z = label[i] > 0 ? -m : m;
            t += z > 0.0 ? z + log1p(exp(-z)) : log1p(exp(z));
        }
        const double sum = block_tree_sum(t, s);
        if (threadIdx.x == 0) partial[part] = sum;
    }
}

__global__ __launch_bounds__(OBJ_THREADS) void k_logloss_final(const double* partial, double* out) {
    __shared__ double s[OBJ_THREADS];
    double t = 0.0;
    for (int i = threadIdx.x; i < PARTS; i += OBJ_THREADS) t += partial[i];
    const double sum = block_tree_sum(t, s);
    if (threadIdx.x == 0) *out = sum;
}

int check_n(int64_t n) {
    OTTO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
    return 0;
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" void otto_obj_constants(int32_t* out) {
    out[0] = OBJ_THREADS;
    out[1] = OBJ_MAX_BLOCKS;
    out[2] = RS_TILE;
    out[3] = SCAN_TILE;
    out[4] = PARTS;
}

extern "C" int otto_obj_binary(const double* d_score, const int32_t* d_label, int64_t n, const double* d_sigmoid, double sigmoid_lo,
                               double sigmoid_factor, double sigma, double w_pos, double w_neg, double hess_floor, double* d_grad,
                               double* d_hess, void* stream) {
    OTTO_TRY(check_n(n));
    OTTO_REQUIRE(sigmoid_factor > 0.0 && sigmoid_lo == sigmoid_lo, "sigmoid_lo = %g, sigmoid_factor = %g", sigmoid_lo, sigmoid_factor);
    OTTO_REQUIRE(sigma > 0.0 && w_pos >= 0.0 && w_neg >= 0.0 && hess_floor >= 0.0, "sigma = %g, w_pos = %g, w_neg = %g, hess_floor = %g: "
                 "sigma must be positive, the others not negative", sigma, w_pos, w_neg, hess_floor);
    if (n == 0) return 0;
    OTTO_REQUIRE(d_score && d_label && d_sigmoid && d_grad && d_hess, "null argument");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    k_obj_binary<<<row_grid(n), OBJ_THREADS, 0, s>>>(d_score, d_label, n, d_sigmoid, sigmoid_lo, sigmoid_factor, sigma, w_pos, w_neg,
                                                     hess_floor, d_grad, d_hess, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_obj_label_counts(const int32_t* d_label, int64_t n, int64_t* d_counts, void* stream) {
    OTTO_TRY(check_n(n));
    OTTO_REQUIRE(d_counts && (d_label || n == 0), "null argument");
    hipStream_t s = (hipStream_t)stream;
    OTTO_HIP(hipMemsetAsync(d_counts, 0, 16, s));
    if (n == 0) return 0;
    k_obj_label_counts<<<row_grid(n), OBJ_THREADS, 0, s>>>(d_label, n, (unsigned long long*)d_counts);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_obj_ndcg_at_k(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                                  int32_t k, const double* d_discount, double* d_ndcg, void* stream) {
    OTTO_TRY(check_query_args(d_score, d_label, d_query_off, Q, n));
    OTTO_REQUIRE(k >= 1 && k <= MAXQ, "k must be in [1, %d] (got %d)", MAXQ, k);
    if (Q == 0) return 0;
    OTTO_REQUIRE(d_discount && d_ndcg, "null d_discount or d_ndcg");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    k_obj_ndcg<<<(unsigned)Q, n / Q <= 96 ? 64 : 256, 0, s>>>(d_score, d_label, d_query_off, n, k, d_discount, d_ndcg, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int64_t otto_obj_auc_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
    return otto_events_sort_workspace(n);
}

extern "C" int otto_obj_auc(const double* d_score, const int32_t* d_label, int64_t n, int64_t* d_out, void* d_work, int64_t work_bytes,
                            void* stream) {
    OTTO_TRY(check_n(n));
    OTTO_REQUIRE(d_out && ((d_score && d_label) || n == 0), "null argument");
    const int64_t need = otto_obj_auc_workspace_bytes(n);
    OTTO_REQUIRE(d_work && work_bytes >= need, "d_work holds %lld bytes, otto_obj_auc_workspace_bytes asks for %lld", (long long)work_bytes,
                 (long long)need);
    hipStream_t s = (hipStream_t)stream;
    OTTO_HIP(hipMemsetAsync(d_out, 0, 24, s));
    if (n == 0) return 0;
    uint64_t *key0, *offs, *partial, *ks;
    uint32_t *val0, *vs;
    otto_sort_ws_buffers(n, d_work, &key0, &val0, &offs, &partial);
    k_auc_keys<<<row_grid(n), OBJ_THREADS, 0, s>>>(d_score, d_label, n, key0, val0);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(otto_sort_pairs_in_ws(key0, n, d_work, &ks, &vs, s));
    OTTO_TRY(device_scan(PosFlag{vs}, n, offs, partial, s));     // the sort is done with both: the workspace keeps them for this
    k_auc_groups<<<row_grid(n), OBJ_THREADS, 0, s>>>(ks, offs, n, (unsigned long long*)d_out);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_obj_logloss_grid(const double* d_score, const int32_t* d_label, int64_t n, double sigma, int32_t grid,
                                     double* d_partials, double* d_loss, void* stream) {
    OTTO_TRY(check_n(n));
    OTTO_REQUIRE(sigma > 0.0, "sigma = %g must be positive", sigma);
    OTTO_REQUIRE(grid >= 1 && grid <= PARTS, "grid = %d outside [1, %d]", grid, PARTS);
    OTTO_REQUIRE(d_partials && d_loss && ((d_score && d_label) || n == 0), "null argument");
    hipStream_t s = (hipStream_t)stream;
    int64_t per = (n + PARTS - 1) / PARTS;
    per = (per + OBJ_THREADS - 1) / OBJ_THREADS * OBJ_THREADS;
    k_logloss_parts<<<(unsigned)grid, OBJ_THREADS, 0, s>>>(d_score, d_label, n, sigma, per, d_partials);
    OTTO_HIP(hipGetLastError());
    k_logloss_final<<<1, OBJ_THREADS, 0, s>>>(d_partials, d_loss);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_obj_logloss(const double* d_score, const int32_t* d_label, int64_t n, double sigma, double* d_partials,
                                double* d_loss, void* stream) {
    // a part is 256 rows at least: no more workgroups than parts that hold rows
    const int64_t live = (n + OBJ_THREADS - 1) / OBJ_THREADS;
    return otto_obj_logloss_grid(d_score, d_label, n, sigma, (int32_t)(live < 1 ? 1 : live < PARTS ? live : PARTS), d_partials, d_loss,
                                 stream);
}
