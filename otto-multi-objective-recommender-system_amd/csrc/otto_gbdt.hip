// LambdaRank gradient-boosted tree training (SPEC-GBDT; include/otto_gbdt.h).
//
// Device, on the caller's stream:
//   k_bin          a tile of 256 rows x 32 features goes through LDS: X is read along its rows, the bins are written
//                  along theirs (uint8 [F, n]); one binary search over the feature's edges per value.
//   k_lambdarank   one workgroup per query. Rank of a row = number of rows that order before it (broadcast LDS reads,
//                  no sort network: cnt <= 1024), then one thread per rank adds that row's pairs in ascending rank of
//                  the partner, in float64 with contraction off. Both rows of a pair compute the same lambda and eta.
//   k_ap           the same ranking; one thread adds the precision terms in rank order.
//   k_absmax, k_quantize   exact max reductions (atomicMax on the bits of a non-negative double), then q = rint(v * 2^e).
//   k_hist         the hot path. grid = (row chunks, groups of 8 features). A workgroup keeps private int64 sums of qg and
//                  qh and uint32 row counts for 8 features x 256 bins in LDS (40 KB) and adds with integer LDS atomics;
//                  a row's (qg, qh) pair is one 8-byte load, its 8 bin bytes come from 8 feature rows of the feature-major
//                  matrix, where ascending row ids (the partition is stable) keep a wave's loads in few lines. One
//                  integer global atomic per touched (feature, bin, plane) and workgroup merges the result.
//   k_hist_sub     larger child = parent - smaller child, in integers.
//   k_best_split   one workgroup per leaf, one wave per feature in turn, 4 bins per lane: int64 prefix sums along the
//                  bins, both NaN variants per edge, float64 gain in the pinned operation order, then a reduction under
//                  the pinned tie order.
//   k_part_count, k_part_scan, k_part_scatter   stable partition of a leaf's row list: left rows per 2048-row block, one
//                  workgroup's exclusive scan of those counts, then the scatter.
//   k_add_tree     one lane per row walks the tree over the bins; bounded, range-checked.
//   device_select  (select.h) the row bag: radix select of the m-th smallest key among all n rows; AllRows reads nothing
//                  from memory.
//   k_bag_count, device_scan (scan.h), k_bag_emit   every wave owns a contiguous run of rows: kept rows (key <= threshold)
//                  per wave, an exclusive scan of the workgroups' sums, then the row ids by ballot rank behind the wave's
//                  base: ascending ids, contiguous writes, every write checked against the caller's buffer.
//   k_hist<true>, k_best_split<true>   the same kernels over an ascending feature list (the per-tree feature sample): a
//                  workgroup's up to 8 list entries are wave-uniform; sums land at the original feature's planes.
// Host: otto_gbdt_grow_tree drives the leaf-wise loop: one small device-to-host copy per split.
#include "gbdt_device.h"
#include "scan.h"
#include "select.h"

#include <math.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace otto {
namespace {

constexpr int BAG_BLOCKS = 1024;    // grid cap of k_bag_count and k_bag_emit (4 waves per workgroup)

// ---------------------------------------------------------------------------------------------------------------------
// binning
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bin(const float* X, int64_t ld, int64_t n, int F, const float* edges, const int32_t* n_edges,
                                             uint8_t* bins) {
    __shared__ float tile[256][33];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    const int rows_here = (int)(n - row0 < 256 ? n - row0 : 256);
    for (int f0 = 0; f0 < F; f0 += 32) {
        const int nf = F - f0 < 32 ? F - f0 : 32;
        // 8 rows x 32 columns per pass: a wave reads two rows' 128-byte runs
        for (int r = tid >> 5; r < rows_here; r += 8) {
            const int c = tid & 31;
            if (c < nf) tile[r][c] = X[(row0 + r) * ld + f0 + c];
        }
        __syncthreads();
        if (tid < rows_here) {
            for (int c = 0; c < nf; ++c) {
                const float x = tile[tid][c];
                const float* e = edges + (int64_t)(f0 + c) * OTTO_GBDT_MAX_EDGES;
                int lo = 0, hi = n_edges[f0 + c];
                hi = hi < 0 ? 0 : (hi > OTTO_GBDT_MAX_EDGES ? OTTO_GBDT_MAX_EDGES : hi);
                while (lo < hi) {                       // the number of edges < x
                    const int mid = (lo + hi) >> 1;
                    if (e[mid] < x) lo = mid + 1; else hi = mid;
                }
                bins[(int64_t)(f0 + c) * n + row0 + tid] = x != x ? (uint8_t)OTTO_GBDT_NAN_BIN : (uint8_t)lo;
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double label_gain(int lab) { return (double)((1u << lab) - 1u); }

struct LambdaArgs {
    const double* score;
    const int32_t* label;
    const int64_t* query_off;
    int64_t Q, n;
    const double* sigmoid;
    double sig_lo, sig_factor;
    const double* discount;
    double sigma;
    int T, norm;
    double* grad;
    double* hess;
    uint32_t* err;
};

__global__ __launch_bounds__(256) void k_lambdarank(LambdaArgs a) {
#pragma clang fp contract(off)
    __shared__ QueryLds s;
    const int tid = threadIdx.x, nt = blockDim.x;
    int64_t lo;
    int cnt;
    if (!query_range(a.query_off, blockIdx.x, a.n, &lo, &cnt, a.err)) return;   // grad / hess were zeroed
    if (cnt == 0) return;
    rank_query(s, a.score, a.label, lo, cnt, a.err);
    for (int r = tid; r < cnt; r += nt) s.disc[r] = a.discount[r];
    if (tid == 0) {
        double sum = 0.0;
        int r = 0;
        for (int lab = OTTO_GBDT_MAX_LABEL; lab >= 0 && r < a.T; --lab) {
            const double g = label_gain(lab);
            for (uint32_t c = 0; c < s.lcnt[lab] && r < a.T; ++c, ++r) sum = sum + g * a.discount[r];
        }
        s.inv_max_dcg = sum > 0.0 ? 1.0 / sum : 0.0;
    }
    __syncthreads();
    const int Tq = a.T < cnt ? a.T : cnt;
    const double inv = s.inv_max_dcg;
    const bool scale = a.norm && s.score[0] != s.score[cnt - 1];
    const double neg_sigma = -a.sigma, sigma2 = a.sigma * a.sigma, top = (double)(OTTO_GBDT_SIGMOID_BINS - 1);
    double part = 0.0;                                  // this thread's share of S = sum of -2 lambda
    for (int r = tid; r < cnt; r += nt) {
        const int lr = s.label[r];
        const double sr = s.score[r], dr = s.disc[r], gr = label_gain(lr);
        double g = 0.0, h = 0.0;
        auto pair = [&](int o) {
#pragma clang fp contract(off)
            const int lo_ = s.label[o];
            if (lo_ == lr) return;
            const bool high = lr > lo_;
            const double so = s.score[o];
            const double d = high ? sr - so : so - sr;
            const double go = label_gain(lo_);
            const double dd = fabs(dr - s.disc[o]);
            double delta = (high ? gr - go : go - gr) * dd * inv;
            if (scale) delta = delta / (0.01 + fabs(d));
            double x = (d - a.sig_lo) * a.sig_factor;
            x = x > 0.0 ? x : 0.0;                      // NaN -> 0
            x = x < top ? x : top;
            const double p = a.sigmoid[(size_t)x];
            const double lam = neg_sigma * delta * p;
            const double eta = sigma2 * delta * p * (1.0 - p);
            g = high ? g + lam : g - lam;
            h = h + eta;
            if (o > r) part = part + -2.0 * lam;        // each pair once, from its i side
        };
        const int first_end = r < Tq ? r : Tq;
        for (int o = 0; o < first_end; ++o) pair(o);    // partners i < min(r, Tq): this row is the pair's j
        if (r < Tq)
            for (int o = r + 1; o < cnt; ++o) pair(o);  // partners j > r: this row is the pair's i
        const int64_t row = lo + s.pos[r];
        a.grad[row] = g;
        a.hess[row] = h;
    }
    if (!a.norm) return;
    part = wave_reduce<Sum>(part);                  // S in any order: the spec does not pin it
    if ((tid & 63) == 0) s.red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double S = 0.0;
        for (int w = 0; w < (nt + 63) / 64; ++w) S += s.red[w];
        s.factor = S > 0.0 ? log2(1.0 + S) / S : 1.0;
    }
    __syncthreads();
    const double f = s.factor;
    if (f != 1.0)
        for (int r = tid; r < cnt; r += nt) {           // each thread rescales the rows it wrote itself
            const int64_t row = lo + s.pos[r];
            a.grad[row] = a.grad[row] * f;
            a.hess[row] = a.hess[row] * f;
        }
}

__global__ __launch_bounds__(256) void k_ap(const double* score, const int32_t* label, const int64_t* query_off, int64_t n, int k,
                                            double* ap, uint32_t* err) {
#pragma clang fp contract(off)
    __shared__ QueryLds s;
    int64_t lo;
    int cnt;
    if (!query_range(query_off, blockIdx.x, n, &lo, &cnt, err)) {
        if (threadIdx.x == 0) ap[blockIdx.x] = -1.0;
        return;
    }
    if (cnt > 0) rank_query(s, score, label, lo, cnt, err);
    if (threadIdx.x == 0) {
        int64_t n_pos = 0;
        if (cnt > 0)
            for (int lab = 1; lab <= OTTO_GBDT_MAX_LABEL; ++lab) n_pos += s.lcnt[lab];
        double sum = 0.0;
        int hits = 0;
        const int top = k < cnt ? k : cnt;
        for (int r = 0; r < top; ++r)
            if (s.label[r] > 0) {
                ++hits;
                sum = sum + (double)hits / (double)(r + 1);
            }
        ap[blockIdx.x] = n_pos > 0 ? sum / (double)(n_pos < k ? n_pos : k) : -1.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// quantisation
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_absmax(const double* grad, const double* hess, int64_t n, unsigned long long* mx) {
    double mg = 0.0, mh = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double g = fabs(grad[i]), h = hess[i];
        mg = g > mg ? g : mg;                           // NaN never wins
        mh = h > mh ? h : mh;
    }
    mg = wave_reduce<Max>(mg);
    mh = wave_reduce<Max>(mh);
    if (lane_id() == 0) {                               // the bits of non-negative doubles order like the values
        atomicMax(mx + 0, (unsigned long long)__double_as_longlong(mg));
        atomicMax(mx + 1, (unsigned long long)__double_as_longlong(mh));
    }
}

__device__ __forceinline__ int quant_exp(double m) {
    if (!(m > 0.0)) return 0;
    int x;
    (void)frexp(m, &x);
    return 30 - x;
}

__global__ __launch_bounds__(256) void k_quantize(const double* grad, const double* hess, int64_t n, const unsigned long long* mx,
                                                  int2* gh, int32_t* exps) {
    const double mg = __longlong_as_double((long long)mx[0]), mh = __longlong_as_double((long long)mx[1]);
    const int eg = quant_exp(mg), eh = quant_exp(mh);
    if (blockIdx.x == 0 && threadIdx.x == 0) { exps[0] = eg; exps[1] = eh; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int2 q;
        q.x = mg > 0.0 ? (int)rint(ldexp(grad[i], eg)) : 0;
        q.y = mh > 0.0 ? (int)rint(ldexp(hess[i], eh)) : 0;
        gh[i] = q;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------------------------------------------------
// rows == nullptr: the rows are 0 .. n_rows - 1 (the root). LIST: blockIdx.y counts groups of 8 entries of feats (n_list
// ascending feature ids inside [0, F), checked by the host); the sums go to the listed feature's own planes.
template <bool LIST>
__global__ __launch_bounds__(HIST_THREADS) void k_hist(const uint8_t* bins, int64_t n, int F, const int2* gh, const int32_t* rows,
                                                       int64_t n_rows, int64_t chunk, unsigned long long* hist, uint32_t* err,
                                                       const int32_t* feats, int n_list) {
    auto range = [&](int64_t* i0, int64_t* i1) {
        *i0 = (int64_t)blockIdx.x * chunk;
        *i1 = *i0 + chunk < n_rows ? *i0 + chunk : n_rows;
    };
    hist_block<LIST>(bins, n, F, gh, rows, range, blockIdx.y * HIST_FG, hist, err, feats, n_list);
}

__global__ __launch_bounds__(256) void k_hist_sub(int64_t* parent, const int64_t* small, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) parent[i] -= small[i];
}

// feats == nullptr: every feature; otherwise the planes of the features outside the list stay zero
int launch_hist(const uint8_t* bins, int64_t n, int F, const int32_t* gh, const int32_t* rows, int64_t n_rows, int64_t* hist,
                uint32_t* err, const int32_t* feats, int n_list, hipStream_t s) {
    OTTO_HIP(hipMemsetAsync(hist, 0, (size_t)3 * F * 256 * 8, s));
    if (n_rows == 0) return 0;
    // about 512 chunks for a large leaf; never below 2048 rows, so that the 6144 merge atomics of a workgroup stay small
    // beside its LDS work
    int64_t chunk = (n_rows + 511) / 512;
    chunk = chunk < 2048 ? 2048 : (chunk + HIST_THREADS - 1) / HIST_THREADS * HIST_THREADS;
    const dim3 grid((unsigned)((n_rows + chunk - 1) / chunk), (unsigned)(((feats ? n_list : F) + HIST_FG - 1) / HIST_FG));
    if (feats)
        k_hist<true><<<grid, HIST_THREADS, 0, s>>>(bins, n, F, (const int2*)gh, rows, n_rows, chunk, (unsigned long long*)hist, err,
                                                   feats, n_list);
    else
        k_hist<false><<<grid, HIST_THREADS, 0, s>>>(bins, n, F, (const int2*)gh, rows, n_rows, chunk, (unsigned long long*)hist, err,
                                                    nullptr, 0);
    OTTO_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// split search
// ---------------------------------------------------------------------------------------------------------------------
struct SplitJobs {
    const int64_t* hist[2];
    int64_t* out[2];
};

template <bool LIST>
__global__ __launch_bounds__(256) void k_best_split(SplitJobs jobs, int F, const int32_t* n_edges, const int32_t* exps, SplitParams p,
                                                    const int32_t* feats, int n_list) {
    best_split_block<LIST>(jobs.hist[blockIdx.x], jobs.out[blockIdx.x], F, n_edges, exps, p, feats, n_list);
}

int launch_best_split(const SplitJobs& jobs, int n_jobs, int F, const int32_t* n_edges, const int32_t* exps, const SplitParams& p,
                      const int32_t* feats, int n_list, hipStream_t s) {
    if (feats) k_best_split<true><<<n_jobs, 256, 0, s>>>(jobs, F, n_edges, exps, p, feats, n_list);
    else k_best_split<false><<<n_jobs, 256, 0, s>>>(jobs, F, n_edges, exps, p, nullptr, 0);
    OTTO_HIP(hipGetLastError());
    return 0;
}


// ---------------------------------------------------------------------------------------------------------------------
// stable partition
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_part_count(const uint8_t* col, int64_t n, int split_bin, int default_left, const int32_t* rows,
                                                    int64_t n_rows, uint32_t* block_left, uint32_t* err) {
    part_count_block(col, n, split_bin, default_left, rows, n_rows, (int64_t)blockIdx.x * PART_ROWS, block_left + blockIdx.x, err);
}

__global__ __launch_bounds__(256) void k_part_scan(uint32_t* block_left, uint32_t n_blocks, int64_t* n_left_out) {
    part_scan_block(block_left, n_blocks, n_left_out);
}

__global__ __launch_bounds__(256) void k_part_scatter(const uint8_t* col, int64_t n, int split_bin, int default_left, const int32_t* rows,
                                                      int64_t n_rows, const uint32_t* block_before, const int64_t* n_left, int32_t* out) {
    part_scatter_block(col, n, split_bin, default_left, rows, n_rows, (int64_t)blockIdx.x * PART_ROWS, block_before[blockIdx.x], *n_left,
                       out);
}


int launch_partition(const uint8_t* bins, int64_t n, int feature, int bin, int default_left, const int32_t* rows, int64_t n_rows,
                     int32_t* out, int64_t* n_left, uint32_t* block_left, uint32_t* err, hipStream_t s) {
    const unsigned nb = (unsigned)part_blocks(n_rows);
    const uint8_t* col = bins + (int64_t)feature * n;
    k_part_count<<<nb, 256, 0, s>>>(col, n, bin, default_left, rows, n_rows, block_left, err);
    OTTO_HIP(hipGetLastError());
    k_part_scan<<<1, 256, 0, s>>>(block_left, nb, n_left);
    OTTO_HIP(hipGetLastError());
    k_part_scatter<<<nb, 256, 0, s>>>(col, n, bin, default_left, rows, n_rows, block_left, n_left, out);
    OTTO_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// score update
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_add_tree(const uint8_t* bins, int64_t n, int F, int L, const int32_t* sf, const int32_t* sb,
                                                  const int32_t* dl, const int32_t* lc, const int32_t* rc, const double* lv,
                                                  double* score, int32_t* leaf_out, uint32_t* err) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int c = L > 1 ? 0 : -1;
    for (int step = 0; step < L - 1 && c >= 0; ++step) {
        if (c >= L - 1) break;
        const int f = sf[c];
        if (f < 0 || f >= F) break;
        c = goes_left(bins[(int64_t)f * n + r], sb[c], dl[c]) ? lc[c] : rc[c];
    }
    const int leaf = ~c;
    if (c >= 0 || leaf >= L) {
        atomicOr(err + ERR_WALK, 1u);
        return;
    }
    score[r] += lv[leaf];
    if (leaf_out) leaf_out[r] = leaf;
}

// ---------------------------------------------------------------------------------------------------------------------
// row bag
// ---------------------------------------------------------------------------------------------------------------------
// row source of the select: every row, one per item
struct AllRows {
    template <typename F>
    __device__ void operator()(int64_t i, F count) const { count(i); }
};

// wave w of the grid owns rows [w * per, (w + 1) * per), per a multiple of 64; wave_cnt[w] = its rows with key <= sel[0]
__global__ __launch_bounds__(256) void k_bag_count(int64_t n, int64_t per, uint64_t seed, const uint64_t* sel, uint32_t* wave_cnt) {
    const int lane = (int)lane_id();
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t threshold = sel[0];
    const int64_t lo = w * per, hi = lo + per < n ? lo + per : n;
    uint32_t cnt = 0;
    for (int64_t r0 = lo; r0 < hi; r0 += 64) {
        const int64_t r = r0 + lane;
        cnt += (uint32_t)__popcll(__ballot(r < hi && row_key(seed, (uint64_t)r) <= threshold));
    }
    if (lane == 0) wave_cnt[w] = cnt;
}

struct BagBlockCount {
    const uint32_t* wave_cnt;
    __device__ uint64_t operator()(int64_t b) const {
        return (uint64_t)wave_cnt[4 * b] + wave_cnt[4 * b + 1] + wave_cnt[4 * b + 2] + wave_cnt[4 * b + 3];
    }
};

// scan [blocks + 1]: kept rows in front of every workgroup and in all. Nothing is written at or behind out[cap].
__global__ __launch_bounds__(256) void k_bag_emit(int64_t n, int64_t per, uint64_t seed, const uint64_t* sel, const uint32_t* wave_cnt,
                                                  const uint64_t* scan, int64_t m, int64_t cap, int32_t* out, uint32_t* err) {
    const int lane = (int)lane_id(), wv = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * 4 + wv;
    if (w == 0 && lane == 0 && ((int64_t)scan[gridDim.x] != m || m > cap)) atomicOr(err + ERR_BAG, 1u);
    const uint64_t threshold = sel[0];
    const uint64_t below = (1ull << lane) - 1ull;
    int64_t at = (int64_t)scan[blockIdx.x];
    for (int j = 0; j < wv; ++j) at += wave_cnt[4 * blockIdx.x + j];
    const int64_t lo = w * per, hi = lo + per < n ? lo + per : n;
    bool over = false;
    for (int64_t r0 = lo; r0 < hi; r0 += 64) {
        const int64_t r = r0 + lane;
        const bool keep = r < hi && row_key(seed, (uint64_t)r) <= threshold;
        const uint64_t mask = __ballot(keep);
        const int64_t pos = at + __popcll(mask & below);
        if (keep) {
            if (pos < cap && pos < m) out[pos] = (int32_t)r;
            else over = true;
        }
        at += __popcll(mask);
    }
    if (over) atomicOr(err + ERR_BAG, 1u);
}

struct BagLayout {
    int64_t hist, sel, wave_cnt, scan, partial, bytes;
};
BagLayout bag_layout() {
    BagLayout w;
    int64_t at = 0;
    w.hist = at; at += SELECT_HIST_BYTES;
    w.sel = at; at += SELECT_SEL_BYTES;
    w.wave_cnt = at; at += align256((int64_t)BAG_BLOCKS * 4 * 4);
    w.scan = at; at += align256((int64_t)(BAG_BLOCKS + 1) * 8);
    w.partial = at; at += align256((int64_t)scan_partial_bytes(BAG_BLOCKS));
    w.bytes = at;
    return w;
}



struct WorkLayout {
    int64_t rows_a, rows_b, block_left, n_left, split, hist, total;
};
WorkLayout work_layout(int64_t n, int32_t F, int32_t num_leaves) {
    WorkLayout w;
    int64_t at = 0;
    w.rows_a = at; at += align256(n * 4);
    w.rows_b = at; at += align256(n * 4);
    w.block_left = at; at += align256(part_blocks(n) * 4);
    w.n_left = at; at += 256;
    w.split = at; at += align256((int64_t)2 * SW * 8);
    w.hist = at; at += (int64_t)num_leaves * 3 * F * 256 * 8;
    w.total = at;
    return w;
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_gbdt_workspace_bytes(int64_t n, int32_t F, int32_t num_leaves) {
    if (n < 0 || n >= ((int64_t)1 << 31) || F < 1 || F > OTTO_FOREST_MAX_FEATURES || num_leaves < 1 ||
        num_leaves > OTTO_FOREST_MAX_LEAVES)
        return 0;
    return work_layout(n, F, num_leaves).total;
}

extern "C" int otto_gbdt_bin(const float* d_X, int64_t ld, int64_t n, int32_t F, const float* d_edges, const int32_t* d_n_edges,
                             uint8_t* d_bins, void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(ld >= F, "row stride ld = %lld below F = %d", (long long)ld, F);
    if (n == 0) return 0;
    OTTO_REQUIRE(d_X && d_edges && d_n_edges, "null argument");
    k_bin<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_X, ld, n, F, d_edges, d_n_edges, d_bins);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_gbdt_lambdarank(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                                    const double* d_sigmoid, double sigmoid_lo, double sigmoid_factor, const double* d_discount,
                                    double sigma, int32_t truncation_level, int32_t norm, double* d_grad, double* d_hess,
                                    void* stream) {
    OTTO_TRY(check_query_args(d_score, d_label, d_query_off, Q, n));
    OTTO_REQUIRE(sigma > 0.0 && sigmoid_factor > 0.0 && sigmoid_lo == sigmoid_lo, "sigma = %g, sigmoid_factor = %g", sigma,
                 sigmoid_factor);
    OTTO_REQUIRE(truncation_level >= 1, "truncation_level = %d", truncation_level);
    OTTO_REQUIRE((d_grad && d_hess) || n == 0, "null d_grad or d_hess");
    hipStream_t s = (hipStream_t)stream;
    if (n) {
        OTTO_HIP(hipMemsetAsync(d_grad, 0, (size_t)n * 8, s));
        OTTO_HIP(hipMemsetAsync(d_hess, 0, (size_t)n * 8, s));
    }
    if (Q == 0) return 0;
    OTTO_REQUIRE(d_sigmoid && d_discount, "null d_sigmoid or d_discount");
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    LambdaArgs a{d_score, d_label, d_query_off, Q, n, d_sigmoid, sigmoid_lo, sigmoid_factor, d_discount, sigma,
                 truncation_level > MAXQ ? MAXQ : truncation_level, norm != 0, d_grad, d_hess, err};
    // short queries (OTTO: 50 to 100 candidates) get one wave, long ones four
    const unsigned threads = n / Q <= 96 ? 64 : 256;
    k_lambdarank<<<(unsigned)Q, threads, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_gbdt_quantize(const double* d_grad, const double* d_hess, int64_t n, int32_t* d_gh, int32_t* d_exp, void* stream) {
    OTTO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(d_exp, "null d_exp");
    OTTO_REQUIRE((d_grad && d_hess && d_gh) || n == 0, "null argument");
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_GBDT_MAX, 256, &scratch, s));
    OTTO_HIP(hipMemsetAsync(scratch, 0, 16, s));
    const unsigned grid = (unsigned)(n == 0 ? 1 : (n + 1023) / 1024 < 2048 ? (n + 1023) / 1024 : 2048);
    k_absmax<<<grid, 256, 0, s>>>(d_grad, d_hess, n, (unsigned long long*)scratch);
    OTTO_HIP(hipGetLastError());
    k_quantize<<<grid, 256, 0, s>>>(d_grad, d_hess, n, (const unsigned long long*)scratch, (int2*)d_gh, d_exp);
    OTTO_HIP(hipGetLastError());
    return 0;
}

extern "C" int otto_gbdt_hist(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_rows,
                              int64_t n_rows, const int32_t* d_features, int32_t n_used, int64_t* d_hist, void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows = %lld outside [0, 2^31)", (long long)n_rows);
    OTTO_REQUIRE(d_hist, "null d_hist");
    OTTO_REQUIRE((d_gh && d_rows) || n_rows == 0, "null d_gh or d_rows");
    hipStream_t s = (hipStream_t)stream;
    if (d_features) OTTO_TRY(check_feature_list(d_features, n_used, F, s));
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_TRY(launch_hist(d_bins, n, F, d_gh, d_rows, n_rows, d_hist, err, d_features, n_used, s));
    return err_end(err, s);
}

extern "C" int otto_gbdt_best_split(const int64_t* d_hist, int32_t F, const int32_t* d_n_edges, const int32_t* d_exp,
                                    int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double lambda_l2,
                                    double min_gain_to_split, const int32_t* d_features, int32_t n_used, int64_t* d_split,
                                    void* stream) {
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    OTTO_REQUIRE(d_hist && d_n_edges && d_exp && d_split, "null argument");
    OTTO_TRY(check_split_params(min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split));
    if (d_features) OTTO_TRY(check_feature_list(d_features, n_used, F, (hipStream_t)stream));
    SplitJobs jobs{{d_hist, d_hist}, {d_split, d_split}};
    SplitParams p{min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split};
    return launch_best_split(jobs, 1, F, d_n_edges, d_exp, p, d_features, n_used, (hipStream_t)stream);
}

extern "C" int64_t otto_gbdt_bag_workspace_bytes(int64_t n) {
    if (n < 1 || n >= ((int64_t)1 << 31)) return 0;
    return bag_layout().bytes;
}

extern "C" int otto_gbdt_bag(int64_t n, int64_t m, uint64_t seed, int32_t* d_rows_out, int64_t out_rows, void* d_work,
                             int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "n = %lld outside [1, 2^31)", (long long)n);
    OTTO_REQUIRE(m >= 1 && m <= n, "m = %lld outside [1, n = %lld]", (long long)m, (long long)n);
    OTTO_REQUIRE(d_rows_out && out_rows >= m, "d_rows_out holds %lld row ids, the bag has %lld", (long long)(d_rows_out ? out_rows : 0),
                 (long long)m);
    const BagLayout w = bag_layout();
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, otto_gbdt_bag_workspace_bytes asks for %lld",
                 (long long)(d_work ? work_bytes : 0), (long long)w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_work;
    uint32_t* hist = (uint32_t*)(base + w.hist);
    uint64_t* sel = (uint64_t*)(base + w.sel);
    uint32_t* wave_cnt = (uint32_t*)(base + w.wave_cnt);
    uint64_t* scan = (uint64_t*)(base + w.scan);
    uint64_t* partial = (uint64_t*)(base + w.partial);
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_TRY(device_select(AllRows{}, n, m, seed, hist, sel, s));
    const unsigned blocks = (unsigned)((n + 255) / 256 < BAG_BLOCKS ? (n + 255) / 256 : BAG_BLOCKS);
    const int64_t waves = (int64_t)blocks * 4;
    const int64_t per = ((n + waves - 1) / waves + 63) / 64 * 64;
    k_bag_count<<<blocks, 256, 0, s>>>(n, per, seed, sel, wave_cnt);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(BagBlockCount{wave_cnt}, (int64_t)blocks, scan, partial, s));
    k_bag_emit<<<blocks, 256, 0, s>>>(n, per, seed, sel, wave_cnt, scan, m, out_rows, d_rows_out, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_gbdt_partition(const uint8_t* d_bins, int64_t n, int32_t feature, int32_t bin, int32_t default_left,
                                   const int32_t* d_rows, int64_t n_rows, int32_t* d_out, int64_t* d_n_left, void* d_work,
                                   int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows = %lld outside [0, 2^31)", (long long)n_rows);
    OTTO_REQUIRE(feature >= 0 && feature < OTTO_FOREST_MAX_FEATURES, "feature = %d", feature);
    OTTO_REQUIRE(bin >= 0 && bin < OTTO_GBDT_MAX_EDGES, "bin = %d outside [0, %d)", bin, OTTO_GBDT_MAX_EDGES);
    OTTO_REQUIRE(d_n_left, "null d_n_left");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        OTTO_HIP(hipMemsetAsync(d_n_left, 0, 8, s));
        return 0;
    }
    OTTO_REQUIRE(d_bins && d_rows && d_out, "null argument");
    OTTO_REQUIRE(d_work && work_bytes >= part_blocks(n_rows) * 4, "d_work holds %lld bytes, the partition needs %lld",
                 (long long)work_bytes, (long long)(part_blocks(n_rows) * 4));
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_TRY(launch_partition(d_bins, n, feature, bin, default_left, d_rows, n_rows, d_out, d_n_left, (uint32_t*)d_work, err, s));
    return err_end(err, s);
}

extern "C" int otto_gbdt_add_tree(const uint8_t* d_bins, int64_t n, int32_t F, int32_t n_leaves, const int32_t* d_split_feature,
                                  const int32_t* d_split_bin, const int32_t* d_default_left, const int32_t* d_left_child,
                                  const int32_t* d_right_child, const double* d_leaf_value, double* d_score, int32_t* d_leaf,
                                  void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(n_leaves >= 1 && n_leaves <= OTTO_FOREST_MAX_LEAVES, "n_leaves = %d outside [1, %d]", n_leaves, OTTO_FOREST_MAX_LEAVES);
    if (n == 0) return 0;
    OTTO_REQUIRE(d_leaf_value && d_score, "null d_leaf_value or d_score");
    OTTO_REQUIRE(n_leaves == 1 || (d_split_feature && d_split_bin && d_default_left && d_left_child && d_right_child), "null node array");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    k_add_tree<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_bins, n, F, n_leaves, d_split_feature, d_split_bin, d_default_left,
                                                            d_left_child, d_right_child, d_leaf_value, d_score, d_leaf, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_gbdt_ap_at_k(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                                 int32_t k, double* d_ap, void* stream) {
    OTTO_TRY(check_query_args(d_score, d_label, d_query_off, Q, n));
    OTTO_REQUIRE(k >= 1 && k <= MAXQ, "k must be in [1, %d] (got %d)", MAXQ, k);
    if (Q == 0) return 0;
    OTTO_REQUIRE(d_ap, "null d_ap");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    k_ap<<<(unsigned)Q, n / Q <= 96 ? 64 : 256, 0, s>>>(d_score, d_label, d_query_off, n, k, d_ap, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_gbdt_grow_tree(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_exp,
                                   const int32_t* d_n_edges, const float* h_edges, int32_t num_leaves,
                                   int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double lambda_l2,
                                   double min_gain_to_split, double learning_rate, const int32_t* d_bag, int64_t n_bag,
                                   const int32_t* d_features, int32_t n_used, int32_t* h_n_leaves, int32_t* h_split_feature,
                                   int32_t* h_split_bin, double* h_threshold, int8_t* h_decision_type, int32_t* h_left_child,
                                   int32_t* h_right_child, double* h_split_gain, double* h_leaf_value, int64_t* h_leaf_count,
                                   int64_t* h_hist_rows, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(!d_bag || (n_bag >= 1 && n_bag <= n), "n_bag = %lld outside [1, n = %lld]", (long long)n_bag, (long long)n);
    OTTO_REQUIRE(n >= 1, "n = 0: nothing to grow a tree on");
    OTTO_REQUIRE(num_leaves >= 2 && num_leaves <= OTTO_FOREST_MAX_LEAVES, "num_leaves = %d outside [2, %d]", num_leaves,
                 OTTO_FOREST_MAX_LEAVES);
    OTTO_TRY(check_split_params(min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split));
    OTTO_REQUIRE(d_gh && d_exp && d_n_edges && h_edges && h_n_leaves && h_split_feature && h_split_bin && h_threshold &&
                 h_decision_type && h_left_child && h_right_child && h_split_gain && h_leaf_value && h_leaf_count, "null argument");
    const WorkLayout w = work_layout(n, F, num_leaves);
    OTTO_REQUIRE(d_work && work_bytes >= w.total, "d_work holds %lld bytes, otto_gbdt_workspace_bytes asks for %lld",
                 (long long)work_bytes, (long long)w.total);
    hipStream_t s = (hipStream_t)stream;
    if (d_features) OTTO_TRY(check_feature_list(d_features, n_used, F, s));
    char* base = (char*)d_work;
    int32_t* rows_a = (int32_t*)(base + w.rows_a);
    int32_t* rows_b = (int32_t*)(base + w.rows_b);
    uint32_t* block_left = (uint32_t*)(base + w.block_left);
    int64_t* d_n_left = (int64_t*)(base + w.n_left);
    int64_t* d_split = (int64_t*)(base + w.split);
    int64_t* hist0 = (int64_t*)(base + w.hist);
    const int64_t hist_words = (int64_t)3 * F * 256;
    SplitParams p{min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split};
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    int32_t exps[2];
    OTTO_HIP(hipMemcpyAsync(exps, d_exp, 8, hipMemcpyDeviceToHost, s));

    struct Leaf {
        int64_t begin, cnt, gq, hq;
        int slot;           // which histogram of the workspace is this leaf's
        int parent, side;   // the internal node that points here (-1: the root), 0 left / 1 right
        bool rows_set;      // false: the root before its first partition (rows 0 .. n - 1, no list)
        int64_t split[SW];
    };
    std::vector<Leaf> leaves(1);
    leaves[0] = Leaf{0, d_bag ? n_bag : n, 0, 0, 0, -1, 0, d_bag != nullptr, {0}};
    int64_t hist_rows = leaves[0].cnt;
    // the bag is the root's row list: every sum, count and partition below is over in-bag rows
    if (d_bag) OTTO_HIP(hipMemcpyAsync(rows_a, d_bag, (size_t)n_bag * 4, hipMemcpyDeviceToDevice, s));
    OTTO_TRY(launch_hist(d_bins, n, F, d_gh, d_bag ? rows_a : nullptr, leaves[0].cnt, hist0, err, d_features, n_used, s));
    {
        SplitJobs jobs{{hist0, hist0}, {d_split, d_split}};
        OTTO_TRY(launch_best_split(jobs, 1, F, d_n_edges, d_exp, p, d_features, n_used, s));
        OTTO_HIP(hipMemcpyAsync(leaves[0].split, d_split, SW * 8, hipMemcpyDeviceToHost, s));
        // a bag is the caller's: an entry outside [0, n) is reported here, before the counts it spoils are compared
        if (d_bag) OTTO_TRY(err_end(err, s));
        else OTTO_HIP(hipStreamSynchronize(s));
        leaves[0].gq = leaves[0].split[9];
        leaves[0].hq = leaves[0].split[10];
    }
    auto gain_of = [](const Leaf& l) { double g; memcpy(&g, &l.split[4], 8); return g; };
    int n_nodes = 0;
    while ((int)leaves.size() < num_leaves) {
        int best = -1;
        for (int i = 0; i < (int)leaves.size(); ++i)
            if (leaves[i].split[0] && (best < 0 || gain_of(leaves[i]) > gain_of(leaves[best]))) best = i;
        if (best < 0) break;
        const int node = n_nodes++, right = (int)leaves.size();
        Leaf P = leaves[best];
        const int f = (int)P.split[1], b = (int)P.split[2], dl = (int)P.split[3];
        OTTO_REQUIRE(f >= 0 && f < F && b >= 0 && b < OTTO_GBDT_MAX_EDGES && P.split[5] >= 0 && P.split[5] <= P.cnt,
                     "the split search returned feature %d, bin %d, %lld of %lld rows left", f, b, (long long)P.split[5],
                     (long long)P.cnt);
        h_split_feature[node] = f;
        h_split_bin[node] = b;
        h_threshold[node] = (double)h_edges[(int64_t)f * OTTO_GBDT_MAX_EDGES + b];
        h_decision_type[node] = (int8_t)((2 << 2) | (dl ? 2 : 0));
        h_split_gain[node] = gain_of(P);
        h_left_child[node] = ~best;
        h_right_child[node] = ~right;
        if (P.parent >= 0) (P.side ? h_right_child : h_left_child)[P.parent] = node;
        // stable partition of the leaf's rows into the other buffer, then back into place
        OTTO_TRY(launch_partition(d_bins, n, f, b, dl, P.rows_set ? rows_a + P.begin : nullptr, P.cnt, rows_b + P.begin, d_n_left,
                                  block_left, err, s));
        OTTO_HIP(hipMemcpyAsync(rows_a + P.begin, rows_b + P.begin, (size_t)P.cnt * 4, hipMemcpyDeviceToDevice, s));
        const int64_t cL = P.split[5], cR = P.cnt - cL;
        Leaf L{P.begin, cL, P.split[6], P.split[7], P.slot, node, 0, true, {0}};
        Leaf R{P.begin + cL, cR, P.gq - P.split[6], P.hq - P.split[7], right, node, 1, true, {0}};
        if (right + 1 < num_leaves) {
            // the smaller child's histogram is built, the larger one is the parent's minus that
            Leaf& small = cL <= cR ? L : R;
            Leaf& large = cL <= cR ? R : L;
            small.slot = right;
            large.slot = P.slot;
            int64_t* hs = hist0 + (int64_t)small.slot * hist_words;
            int64_t* hl = hist0 + (int64_t)large.slot * hist_words;
            OTTO_TRY(launch_hist(d_bins, n, F, d_gh, rows_a + small.begin, small.cnt, hs, err, d_features, n_used, s));
            hist_rows += small.cnt;
            k_hist_sub<<<(unsigned)((hist_words + 255) / 256), 256, 0, s>>>(hl, hs, hist_words);
            OTTO_HIP(hipGetLastError());
            SplitJobs jobs{{hist0 + (int64_t)L.slot * hist_words, hist0 + (int64_t)R.slot * hist_words}, {d_split, d_split + SW}};
            OTTO_TRY(launch_best_split(jobs, 2, F, d_n_edges, d_exp, p, d_features, n_used, s));
            int64_t both[2 * SW];
            OTTO_HIP(hipMemcpyAsync(both, d_split, sizeof(both), hipMemcpyDeviceToHost, s));
            OTTO_HIP(hipStreamSynchronize(s));
            memcpy(L.split, both, SW * 8);
            memcpy(R.split, both + SW, SW * 8);
            OTTO_REQUIRE(L.split[8] == cL && R.split[8] == cR && L.split[9] == L.gq && R.split[9] == R.gq,
                         "the children's histograms disagree with the split that made them (node %d)", node);
        }
        leaves[best] = L;
        leaves.push_back(R);
    }
    OTTO_TRY(err_end(err, s));
    const double lr = learning_rate;
    for (int i = 0; i < (int)leaves.size(); ++i) {
        const double G = ldexp((double)leaves[i].gq, -exps[0]), H = ldexp((double)leaves[i].hq, -exps[1]);
        h_leaf_value[i] = -(G / (H + lambda_l2)) * lr;
        h_leaf_count[i] = leaves[i].cnt;
    }
    *h_n_leaves = (int32_t)leaves.size();
    if (h_hist_rows) *h_hist_rows = hist_rows;
    return 0;
}
