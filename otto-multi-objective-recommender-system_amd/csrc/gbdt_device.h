// Device and host pieces of SPEC-GBDT that more than one trainer uses (otto_gbdt.hip: leaf-wise LambdaRank; otto_xgb.hip:
// depth-wise rank:pairwise): the per-query ranking in LDS, the bodies of the histogram, split-search and partition
// kernels as workgroup functions (a kernel decides which rows, which histogram and which output a workgroup works on, the
// body is the same), the error words of a call and the argument checks. Everything sits in an unnamed namespace: each
// translation unit gets its own copy, as it did when the code lived in otto_gbdt.hip.
#pragma once
#include "common.h"
#include "wave.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_forest.h"
#include "../../include/otto_gbdt.h"

namespace otto {
namespace {

constexpr int MAXQ = OTTO_GBDT_MAX_QUERY;
constexpr int HIST_FG = 8;          // features per histogram workgroup
constexpr int HIST_THREADS = 256;
constexpr int PART_ROWS = 2048;     // rows per partition workgroup
constexpr int SW = OTTO_GBDT_SPLIT_WORDS;
// error words of a call
constexpr int ERR_QUERY = 0, ERR_LABEL = 1, ERR_ROW = 2, ERR_WALK = 3, ERR_BAG = 4, ERR_WORDS = 5;

// ---------------------------------------------------------------------------------------------------------------------
// per-query ranking, shared by the objectives and AP@k
// ---------------------------------------------------------------------------------------------------------------------
struct QueryLds {
    uint64_t key[MAXQ];       // by position
    double score[MAXQ];       // by rank
    double disc[MAXQ];        // discount[r] (LambdaRank only)
    uint16_t pos[MAXQ];       // by rank: the row's position in the query
    uint8_t label[MAXQ];      // by rank
    uint32_t lcnt[OTTO_GBDT_MAX_LABEL + 1];
    double red[16];
    double inv_max_dcg, factor;
};

// false (and the error word counted) for a query the spec refuses
__device__ __forceinline__ bool query_range(const int64_t* query_off, int64_t q, int64_t n, int64_t* lo, int* cnt, uint32_t* err) {
    const int64_t a = query_off[q], b = query_off[q + 1];
    if (!(a >= 0 && a <= b && b <= n && b - a <= MAXQ)) {
        if (threadIdx.x == 0) atomicAdd(err + ERR_QUERY, 1u);
        return false;
    }
    *lo = a;
    *cnt = (int)(b - a);
    return true;
}

// fills s.score / s.pos / s.label by rank and s.lcnt; ends with a barrier. S: QueryLds, or arrays of the same names for
// fewer rows
template <typename S>
__device__ __forceinline__ void rank_query(S& s, const double* score, const int32_t* label, int64_t lo, int cnt, uint32_t* err) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int p = tid; p < cnt; p += nt) s.key[p] = score_key(score[lo + p]);
    if (tid <= OTTO_GBDT_MAX_LABEL) s.lcnt[tid] = 0;
    __syncthreads();
    for (int p = tid; p < cnt; p += nt) {
        const uint64_t k = s.key[p];
        int r = 0;
        for (int o = 0; o < cnt; ++o) {
            const uint64_t ko = s.key[o];
            r += (ko > k || (ko == k && o < p)) ? 1 : 0;
        }
        int lab = label[lo + p];
        if (lab < 0 || lab > OTTO_GBDT_MAX_LABEL) {
            atomicOr(err + ERR_LABEL, 1u);
            lab = lab < 0 ? 0 : OTTO_GBDT_MAX_LABEL;
        }
        s.score[r] = score[lo + p];
        s.pos[r] = (uint16_t)p;
        s.label[r] = (uint8_t)lab;
        atomicAdd(&s.lcnt[lab], 1u);
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// histogram: one workgroup adds the rows [i0, i1) of a row list into the planes of up to 8 features
// ---------------------------------------------------------------------------------------------------------------------
// rows == nullptr: the rows are their own indices (the root). LIST: f0 is the first of up to 8 entries of feats (n_list
// ascending feature ids inside [0, F), checked by the host); the sums go to the listed feature's own planes.
// range(&i0, &i1) names the rows, once the LDS sums are cleared.
template <bool LIST, typename Range>
__device__ __forceinline__ void hist_block(const uint8_t* bins, int64_t n, int F, const int2* gh, const int32_t* rows, Range range,
                                           int f0, unsigned long long* hist, uint32_t* err, const int32_t* feats, int n_list) {
    __shared__ unsigned long long sg[HIST_FG * 256];
    __shared__ unsigned long long sh[HIST_FG * 256];
    __shared__ uint32_t sc[HIST_FG * 256];
    const int tid = threadIdx.x;
    const int nf = LIST ? (n_list - f0 < HIST_FG ? n_list - f0 : HIST_FG) : (F - f0 < HIST_FG ? F - f0 : HIST_FG);
    for (int j = tid; j < HIST_FG * 256; j += HIST_THREADS) { sg[j] = 0; sh[j] = 0; sc[j] = 0; }
    __syncthreads();
    int64_t i0, i1;
    range(&i0, &i1);
    const uint8_t* col = bins + (int64_t)f0 * n;
    int fid[HIST_FG];                                   // LIST: the group's feature ids, the same in every lane
    if constexpr (LIST) {
#pragma unroll
        for (int f = 0; f < HIST_FG; ++f) fid[f] = f < nf ? feats[f0 + f] : 0;
    }
    bool bad = false;
    for (int64_t i = i0 + tid; i < i1; i += HIST_THREADS) {
        const int64_t rid = rows ? (int64_t)rows[i] : i;
        if (rid < 0 || rid >= n) { bad = true; continue; }
        const int2 q = gh[rid];
        uint32_t b[HIST_FG];
#pragma unroll
        for (int f = 0; f < HIST_FG; ++f) {
            if constexpr (LIST) b[f] = f < nf ? bins[(int64_t)fid[f] * n + rid] : 0u;
            else b[f] = f < nf ? col[(int64_t)f * n + rid] : 0u;
        }
        const unsigned long long qg = (unsigned long long)(long long)q.x, qh = (unsigned long long)(long long)q.y;
#pragma unroll
        for (int f = 0; f < HIST_FG; ++f)
            if (f < nf) {
                const int j = f * 256 + (int)b[f];
                atomicAdd(&sg[j], qg);
                atomicAdd(&sh[j], qh);
                atomicAdd(&sc[j], 1u);
            }
    }
    if (bad) atomicOr(err + ERR_ROW, 1u);
    __syncthreads();
    const int64_t plane = (int64_t)F * 256;
    if constexpr (LIST) {
        for (int j = tid; j < nf * 256; j += HIST_THREADS) {
            const uint32_t c = sc[j];
            if (c) {
                unsigned long long* out = hist + (int64_t)feats[f0 + (j >> 8)] * 256 + (j & 255);
                atomicAdd(out, sg[j]);
                atomicAdd(out + plane, sh[j]);
                atomicAdd(out + 2 * plane, (unsigned long long)c);
            }
        }
    } else {
        unsigned long long* out = hist + (int64_t)f0 * 256;
        for (int j = tid; j < nf * 256; j += HIST_THREADS) {
            const uint32_t c = sc[j];
            if (c) {
                atomicAdd(out + j, sg[j]);
                atomicAdd(out + plane + j, sh[j]);
                atomicAdd(out + 2 * plane + j, (unsigned long long)c);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// split search: one workgroup of 256 threads searches one histogram
// ---------------------------------------------------------------------------------------------------------------------
struct SplitParams {
    int64_t min_data;
    double min_hess, l2, min_gain;
};
struct Cand {
    double gain;
    int32_t found, f, b, dl;
    int64_t cntL, gL, hL;
};

__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
    if (!a.found || !b.found) return a.found && !b.found;
    if (a.gain != b.gain) return a.gain > b.gain;
    if (a.f != b.f) return a.f < b.f;
    if (a.b != b.b) return a.b < b.b;
    return a.dl < b.dl;
}

__device__ __forceinline__ void cand_try(Cand& best, int f, int b, int dl, int64_t gL, int64_t hL, int64_t cL, int64_t gP, int64_t hP,
                                         int64_t cP, int eg, int eh, const SplitParams& p) {
#pragma clang fp contract(off)
    const int64_t cR = cP - cL, gR = gP - gL, hR = hP - hL;
    if (cL < p.min_data || cR < p.min_data) return;
    const double GL = ldexp((double)gL, -eg), HL = ldexp((double)hL, -eh);
    const double GR = ldexp((double)gR, -eg), HR = ldexp((double)hR, -eh);
    if (HL < p.min_hess || HR < p.min_hess) return;
    const double GP = ldexp((double)gP, -eg), HP = ldexp((double)hP, -eh);
    const double tl = GL * GL / (HL + p.l2);
    const double tr = GR * GR / (HR + p.l2);
    const double tp = GP * GP / (HP + p.l2);
    const double gain = (tl + tr) - tp;
    if (!(gain > p.min_gain)) return;
    Cand c;
    c.gain = gain; c.found = 1; c.f = f; c.b = b; c.dl = dl; c.cntL = cL; c.gL = gL; c.hL = hL;
    if (cand_better(c, best)) best = c;
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) { return (int64_t)__shfl((long long)v, src, 64); }

// LIST: the waves walk the n_list entries of feats (ascending, so "smallest f" is over the listed features) and the
// parent's sums come from the first listed feature
template <bool LIST>
__device__ __forceinline__ void best_split_block(const int64_t* hist, int64_t* out, int F, const int32_t* n_edges, const int32_t* exps,
                                                 const SplitParams& p, const int32_t* feats, int n_list) {
    __shared__ Cand s_best[4];
    const int l = (int)lane_id(), w = threadIdx.x >> 6;
    const int64_t plane = (int64_t)F * 256;
    const int eg = exps[0], eh = exps[1];
    // the parent's sums: all 256 bins of feature 0 (LIST: of the first listed feature)
    const int64_t* h0 = LIST ? hist + (int64_t)feats[0] * 256 : hist;
    int64_t gP = 0, hP = 0, cP = 0;
    for (int e = 0; e < 4; ++e) {
        gP += h0[l * 4 + e];
        hP += h0[plane + l * 4 + e];
        cP += h0[2 * plane + l * 4 + e];
    }
    gP = wave_reduce<Sum>(gP);
    hP = wave_reduce<Sum>(hP);
    cP = wave_reduce<Sum>(cP);
    Cand best;
    best.found = 0; best.gain = 0.0; best.f = best.b = best.dl = 0; best.cntL = best.gL = best.hL = 0;
    for (int i = w; i < (LIST ? n_list : F); i += 4) {
        const int f = LIST ? feats[i] : i;
        const int64_t* hf = hist + (int64_t)f * 256 + l * 4;
        int64_t g[4], h[4], c[4];
        for (int e = 0; e < 4; ++e) { g[e] = hf[e]; h[e] = hf[plane + e]; c[e] = hf[2 * plane + e]; }
        for (int e = 1; e < 4; ++e) { g[e] += g[e - 1]; h[e] += h[e - 1]; c[e] += c[e - 1]; }
        const int64_t og = wave_incl_scan<int64_t>(g[3]) - g[3], oh = wave_incl_scan<int64_t>(h[3]) - h[3],
                      oc = wave_incl_scan<int64_t>(c[3]) - c[3];
        // bin 255 alone: lane 63's last element minus the one before it
        const int64_t ng = shfl64(g[3] - g[2], 63), nh = shfl64(h[3] - h[2], 63), nc = shfl64(c[3] - c[2], 63);
        int ne = n_edges[f];
        ne = ne < 0 ? 0 : (ne > OTTO_GBDT_MAX_EDGES ? OTTO_GBDT_MAX_EDGES : ne);
        for (int e = 0; e < 4; ++e) {
            const int b = l * 4 + e;
            if (b >= ne) break;
            const int64_t gL = og + g[e], hL = oh + h[e], cL = oc + c[e];
            cand_try(best, f, b, 0, gL, hL, cL, gP, hP, cP, eg, eh, p);
            cand_try(best, f, b, 1, gL + ng, hL + nh, cL + nc, gP, hP, cP, eg, eh, p);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        Cand o;
        o.gain = __shfl_xor(best.gain, d, 64);
        o.found = __shfl_xor(best.found, d, 64);
        o.f = __shfl_xor(best.f, d, 64);
        o.b = __shfl_xor(best.b, d, 64);
        o.dl = __shfl_xor(best.dl, d, 64);
        o.cntL = (int64_t)__shfl_xor((long long)best.cntL, d, 64);
        o.gL = (int64_t)__shfl_xor((long long)best.gL, d, 64);
        o.hL = (int64_t)__shfl_xor((long long)best.hL, d, 64);
        if (cand_better(o, best)) best = o;
    }
    if (l == 0) s_best[w] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i)
            if (cand_better(s_best[i], best)) best = s_best[i];
        out[0] = best.found;
        out[1] = best.f;
        out[2] = best.b;
        out[3] = best.dl;
        out[4] = (int64_t)__double_as_longlong(best.gain);
        out[5] = best.cntL;
        out[6] = best.gL;
        out[7] = best.hL;
        out[8] = cP;
        out[9] = gP;
        out[10] = hP;
        out[11] = 0;
    }
}

inline int check_split_params(int64_t min_data, double min_hess, double l2, double min_gain) {
    OTTO_REQUIRE(min_data >= 0, "min_data_in_leaf = %lld", (long long)min_data);
    OTTO_REQUIRE(min_hess >= 0.0 && l2 >= 0.0 && min_gain == min_gain, "min_sum_hessian_in_leaf = %g, lambda_l2 = %g, "
                 "min_gain_to_split = %g", min_hess, l2, min_gain);
    OTTO_REQUIRE(min_hess + l2 > 0.0, "min_sum_hessian_in_leaf + lambda_l2 must be positive (a leaf value divides by H + lambda_l2)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// stable partition: a row list is cut into blocks of PART_ROWS rows, one workgroup of 256 threads each
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool goes_left(uint32_t bin, int split_bin, int default_left) {
    return bin == OTTO_GBDT_NAN_BIN ? default_left != 0 : (int)bin <= split_bin;
}

// *out_left = the rows of the block at i0 that go left. rows == nullptr: the rows are their own indices; a row id outside
// [0, n) goes right unread
__device__ __forceinline__ void part_count_block(const uint8_t* col, int64_t n, int split_bin, int default_left, const int32_t* rows,
                                                 int64_t n_rows, int64_t i0, uint32_t* out_left, uint32_t* err) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int e = 0; e < PART_ROWS / 256; ++e) {
        const int64_t i = i0 + e * 256 + threadIdx.x;
        if (i < n_rows) {
            const int64_t rid = rows ? (int64_t)rows[i] : i;
            if (rid < 0 || rid >= n) atomicOr(err + ERR_ROW, 1u);
            else mine += goes_left(col[rid], split_bin, default_left) ? 1u : 0u;
        }
    }
    mine = wave_reduce<Sum>(mine);
    if (lane_id() == 0) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) *out_left = s_n;
}

// one workgroup: block_left becomes its own exclusive prefix sum (below 2^31, as n is), the total goes to n_left_out
__device__ __forceinline__ void part_scan_block(uint32_t* block_left, uint32_t n_blocks, int64_t* n_left_out) {
    __shared__ uint32_t smem[8];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t c = b < n_blocks ? block_left[b] : 0u;
        uint32_t tile;
        const uint32_t ex = block_excl_scan<uint32_t, 256>(c, smem, &tile);
        if (b < n_blocks) block_left[b] = carry + ex;
        carry += tile;
    }
    if (threadIdx.x == 0) *n_left_out = (int64_t)carry;
}

// before: the left rows in front of the block at i0; total: the left rows of the whole list. out receives the n_rows rows.
__device__ __forceinline__ void part_scatter_block(const uint8_t* col, int64_t n, int split_bin, int default_left, const int32_t* rows,
                                                   int64_t n_rows, int64_t i0, int64_t before, int64_t total, int32_t* out) {
    __shared__ uint32_t smem[8];
    int64_t left_at = before, right_at = total + (i0 - before);
    for (int e = 0; e < PART_ROWS / 256; ++e) {
        const int64_t i = i0 + e * 256 + threadIdx.x;
        int32_t rid = 0;
        uint32_t left = 0;
        const bool live = i < n_rows;
        if (live) {
            rid = rows ? rows[i] : (int32_t)i;
            left = (rid >= 0 && rid < n && goes_left(col[rid], split_bin, default_left)) ? 1u : 0u;
        }
        uint32_t n_l;
        const uint32_t ex = block_excl_scan<uint32_t, 256>(left, smem, &n_l);
        if (live) {
            if (left) out[left_at + ex] = rid;
            else out[right_at + (threadIdx.x - ex)] = rid;
        }
        const int64_t live_here = n_rows - (i0 + e * 256) < 256 ? n_rows - (i0 + e * 256) : 256;
        left_at += n_l;
        right_at += (live_here > 0 ? live_here : 0) - n_l;
    }
}

__host__ __device__ inline int64_t part_blocks(int64_t n_rows) { return (n_rows + PART_ROWS - 1) / PART_ROWS; }

// ---------------------------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------------------------
inline int err_begin(uint32_t** err, hipStream_t s) {
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_GBDT, 256, &scratch, s));
    *err = (uint32_t*)scratch;
    OTTO_HIP(hipMemsetAsync(scratch, 0, 64, s));
    return 0;
}

// the error words of a call, on the host, as a return code
inline int err_code(const uint32_t* bad) {
    if (bad[ERR_QUERY]) {
        set_error("%u quer%s with query_off not in 0 <= query_off[q] <= query_off[q+1] <= n or with more than %d rows: left "
                  "zero", bad[ERR_QUERY], bad[ERR_QUERY] == 1 ? "y" : "ies", MAXQ);
        return OTTO_EINVAL;
    }
    if (bad[ERR_LABEL]) {
        set_error("a label outside 0..%d", OTTO_GBDT_MAX_LABEL);
        return OTTO_EINVAL;
    }
    if (bad[ERR_ROW]) {
        set_error("a row id outside [0, n) in a leaf's row list: skipped");
        return OTTO_EINVAL;
    }
    if (bad[ERR_WALK]) {
        set_error("a tree walk did not reach a leaf of its tree within n_leaves - 1 steps, or read a feature outside [0, F)");
        return OTTO_EINVAL;
    }
    if (bad[ERR_BAG]) {
        set_error("the bag did not come to exactly m rows inside d_rows_out");
        return OTTO_EINVAL;
    }
    return 0;
}

// drains the stream and turns the error words into a return code
inline int err_end(uint32_t* err, hipStream_t s) {
    uint32_t bad[ERR_WORDS] = {0, 0, 0, 0, 0};
    OTTO_HIP(hipMemcpyAsync(bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    return err_code(bad);
}

inline int check_bins_args(const uint8_t* d_bins, int64_t n, int32_t F) {
    OTTO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    OTTO_REQUIRE(d_bins || n == 0, "null d_bins");
    return 0;
}

// copies the list to the host (one synchronisation): n_used ascending feature ids inside [0, F)
inline int check_feature_list(const int32_t* d_features, int32_t n_used, int32_t F, hipStream_t s) {
    OTTO_REQUIRE(n_used >= 1 && n_used <= F, "n_used = %d outside [1, F = %d]", n_used, F);
    int32_t h[OTTO_FOREST_MAX_FEATURES];
    OTTO_HIP(hipMemcpyAsync(h, d_features, (size_t)n_used * 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n_used; ++i)
        OTTO_REQUIRE(h[i] >= 0 && h[i] < F && (i == 0 || h[i] > h[i - 1]), "d_features[%d] = %d: the list must ascend strictly inside "
                     "[0, F = %d)", i, h[i], F);
    return 0;
}

inline int check_query_args(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n) {
    OTTO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(Q >= 0 && Q < ((int64_t)1 << 31), "Q = %lld outside [0, 2^31)", (long long)Q);
    OTTO_REQUIRE(d_query_off || Q == 0, "null d_query_off");
    OTTO_REQUIRE((d_score && d_label) || n == 0, "null d_score or d_label");
    return 0;
}

}  // namespace
}  // namespace otto
