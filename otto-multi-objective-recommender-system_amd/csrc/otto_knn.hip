// Exact k-nearest-neighbour table over aid embeddings (SPEC-KNN; include/otto_knn.h).
//
// Three kernels on the caller's stream:
//   k_knn_items   one thread per item: the per-item pair (mul, add) that turns the tile's accumulator into the ranked
//                 score  s = fma(acc, mul, add)  (larger = nearer, so the desc lists of sclist.h are reused as they are):
//                     euclidean  acc = <2a, b>            (mul, add) = (1, -|b|^2)      s = 2<a,b> - |b|^2 = |a|^2 - D2
//                     angular    acc = <2a/|a|, b>        (mul, add) = (1/|b|, -2)      s = 2 cos - 2     = -key
//                     dot        acc = <a, b>             (mul, add) = (1, 0)           s = <a,b>         = -key
//                 an item with valid == 0 gets (0, -inf): s = -inf never passes a threshold. The row-side factor
//                 (2, 2/|a|, 1) is applied once to the A fragments; 2 is exact, 1/|a| costs one rounding per element.
//   k_knn         the structure of k_score (otto_mf.hip): 128 query rows per workgroup held as MFMA A fragments for the
//                 whole item loop, 32-item tiles staged through LDS with the next tile (and its (mul, add) pairs) prefetched
//                 under the MFMAs, 32x32 accumulators, per-row threshold test by ballot, insertion into the row's sorted
//                 k-list in LDS. The lists are DYNAMIC LDS of exactly 128 x k x 8 bytes (23 KB at k = 45 .. 64 KB at k = 64),
//                 so the workgroups per CU follow k instead of the worst case. Self is skipped at insertion time by id
//                 (the row's aid sits in LDS), which costs no register in the tile loop.
//   k_knn_merge   one wave per row: exact merge of the item-range splits (sclist.h), score -> dist, padding, n.
#include "common.h"
#include "wave.h"
#include "sclist.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_knn.h"

#include <math.h>
#include <string.h>

namespace otto {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int KN_BM = 128;      // rows per workgroup (4 waves x 32)
constexpr int KN_BN = 32;       // items per tile
constexpr int64_t KN_HDR = 256; // workspace header: the error word


struct KnnArgs {
    const float* E;
    const float2* item;        // [N] (mul, add)
    const int32_t* rows;       // nullable
    int64_t R, N;
    int k, metric;
    int nsplit;
    int64_t items_per_split;   // multiple of KN_BN
    float* part_s;             // [nsplit][Rpad][k]
    int32_t* part_i;
    uint32_t* err;
};

template <int D>
__global__ __launch_bounds__(256) void k_knn_items(const float* E, const uint8_t* valid, int64_t N, int metric, float2* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float2 o = make_float2(0.f, -INFINITY);
    if (!valid || valid[i]) {
        float n2 = 0.f;
#pragma unroll
        for (int q = 0; q < D; q += 4) {
            const float4 t = ld4(E + i * D + q);
            n2 = fmaf(t.x, t.x, n2); n2 = fmaf(t.y, t.y, n2); n2 = fmaf(t.z, t.z, n2); n2 = fmaf(t.w, t.w, n2);
        }
        if (metric == OTTO_KNN_EUCLIDEAN) o = make_float2(1.f, -n2);
        else if (metric == OTTO_KNN_ANGULAR) o = make_float2(n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f, -2.f);
        else o = make_float2(1.f, 0.f);
    }
    out[i] = o;
}

template <int D>
__global__ __launch_bounds__(256) void k_knn(KnnArgs a) {
    constexpr int HD = D / 2;               // k range of one lane half
    constexpr int LDV = D + 4;              // padded LDS row (floats): conflict-free ds_read_b128
    __shared__ float s_v[KN_BN * LDV];
    __shared__ int32_t s_rid[4][32];
    extern __shared__ float s_lists[];      // float [128][k] scores, then int32 [128][k] ids

    const int wid = threadIdx.x >> 6;
    const unsigned l = lane_id();
    const int r = l & 31, h = l >> 5;
    const int k = a.k;
    const int64_t row_tile = blockIdx.x;
    const int split = blockIdx.y;
    const int64_t grow = row_tile * KN_BM + wid * 32 + r;
    float* const w_ls = s_lists + (size_t)wid * 32 * k;
    int32_t* const w_li = reinterpret_cast<int32_t*>(s_lists + (size_t)KN_BM * k) + (size_t)wid * 32 * k;

    // the query aid of this lane's row; an id outside [0, N) is reported and the row left empty (never dereferenced)
    int32_t rid = -1;
    if (grow < a.R) {
        rid = a.rows ? a.rows[grow] : (int32_t)grow;
        if ((uint32_t)rid >= (uint64_t)a.N) {
            if (h == 0 && split == 0) atomicAdd(a.err, 1u);
            rid = -1;
        }
    }
    float scale = 0.f;
    if (rid >= 0) scale = a.metric == OTTO_KNN_EUCLIDEAN ? 2.f : (a.metric == OTTO_KNN_ANGULAR ? 2.f * a.item[rid].x : 1.f);
    // A fragments: scale * E[rid][h*HD + s], s = 0..HD-1, kept in registers for the whole item loop
    float ua[HD];
#pragma unroll
    for (int q = 0; q < HD; q += 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rid >= 0) t = ld4(a.E + (int64_t)rid * D + h * HD + q);
        ua[q] = t.x * scale; ua[q + 1] = t.y * scale; ua[q + 2] = t.z * scale; ua[q + 3] = t.w * scale;
    }
    if (h == 0) s_rid[wid][r] = rid;
    for (int i = l; i < 32 * k; i += 64) { w_ls[i] = -INFINITY; w_li[i] = 0x7FFFFFFF; }
    float thr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) thr[q] = -INFINITY;

    const int64_t n_lo = (int64_t)split * a.items_per_split;
    int64_t n_hi = n_lo + a.items_per_split;
    if (n_hi > a.N) n_hi = a.N;

    // staging: thread t loads KN_BN*D/256 floats of the next item tile (contiguous float4s) and its column's (mul, add)
    constexpr int F4_PER_THREAD = (KN_BN * D / 4 + 255) / 256;
    float4 stage[F4_PER_THREAD];
    float2 stage_it;
    auto load_tile = [&](int64_t n0) {
#pragma unroll
        for (int q = 0; q < F4_PER_THREAD; ++q) {
            const int f = threadIdx.x + q * 256;          // float4 index inside the tile
            const int item = f / (D / 4), c4 = f % (D / 4);
            stage[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f < KN_BN * D / 4 && n0 + item < n_hi) stage[q] = ld4(a.E + (n0 + item) * D + 4 * c4);
        }
        stage_it = make_float2(0.f, -INFINITY);
        if (n0 + r < n_hi) stage_it = a.item[n0 + r];
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int q = 0; q < F4_PER_THREAD; ++q) {
            const int f = threadIdx.x + q * 256;
            const int item = f / (D / 4), c4 = f % (D / 4);
            if (f < KN_BN * D / 4) st4(&s_v[item * LDV + 4 * c4], stage[q]);
        }
    };

    if (n_lo < n_hi) load_tile(n_lo);
    for (int64_t n0 = n_lo; n0 < n_hi; n0 += KN_BN) {
        __syncthreads();            // previous tile fully consumed (and, first time round, the lists initialised)
        store_tile();
        const float2 it = stage_it;
        __syncthreads();
        if (n0 + KN_BN < n_hi) load_tile(n0 + KN_BN);   // prefetch under the MFMAs

        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        const float* vb = &s_v[r * LDV + h * HD];
#pragma unroll
        for (int q = 0; q < HD; q += 4) {
            const float4 b = ld4(vb + q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[q], b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[q + 1], b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[q + 2], b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[q + 3], b.w, acc, 0, 0, 0);
        }
        // acc[q]: item column = lane & 31, row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float sc = fmaf(acc[q], it.x, it.y);     // -inf for an invalid or out-of-range column
            uint64_t m = __ballot(sc > thr[q]);
            while (m) {
                const int src = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int srow = (q & 3) + 8 * (q >> 2) + 4 * (src >> 5);
                const int32_t id2 = (int32_t)(n0 + (src & 31));
                if (id2 == s_rid[wid][srow]) continue;      // self, excluded by id; met once per row
                const float s2 = __shfl(sc, src, 64);
                const float nt = list_insert(w_ls + srow * k, w_li + srow * k, k, s2, id2);
                if (h == (src >> 5)) thr[q] = nt;
                m &= __ballot(sc > thr[q]);
            }
        }
    }
    __syncthreads();
    // partial lists of this (row tile, split)
    const int64_t Rpad = (int64_t)gridDim.x * KN_BM;
    for (int i = l; i < 32 * k; i += 64) {
        const int rr = i / k, c = i % k;
        const int64_t prow = row_tile * KN_BM + wid * 32 + rr;
        const int64_t o = ((int64_t)split * Rpad + prow) * k + c;
        a.part_s[o] = w_ls[i];
        a.part_i[o] = w_li[i];
    }
}

// one wave per query row: merge the splits, turn the ranked score back into the metric's value, pad, count
__global__ __launch_bounds__(64) void k_knn_merge(KnnArgs a, int64_t Rpad, int32_t* ids, float* dist, int32_t* n) {
    const int64_t row = blockIdx.x;
    if (row >= a.R) return;
    const unsigned l = lane_id();
    const int k = a.k;
    float bs;
    int32_t bi;
    merge_row_lists(a.part_s, a.part_i, a.nsplit, Rpad, row, k, bs, bi);
    const int32_t rid = a.rows ? a.rows[row] : (int32_t)row;
    float2 self = make_float2(0.f, -INFINITY);
    if ((uint32_t)rid < (uint64_t)a.N) self = a.item[rid];
    const bool filled = (int)l < k && self.y != -INFINITY && bi != 0x7FFFFFFF;
    float v = INFINITY;
    if (filled) {
        if (a.metric == OTTO_KNN_EUCLIDEAN) v = sqrtf(fmaxf(-self.y - bs, 0.f));   // |a|^2 - (2<a,b> - |b|^2)
        else if (a.metric == OTTO_KNN_ANGULAR) v = sqrtf(fmaxf(-bs, 0.f));
        else v = bs;
    }
    const int cnt = __popcll(__ballot(filled));
    if ((int)l < k) {
        ids[row * k + l] = filled ? bi : -1;
        dist[row * k + l] = v;
    }
    if (l == 0) n[row] = cnt;
}

// item-range splits so that a few row tiles still fill the machine (as score_nsplit of otto_mf.hip)
int knn_nsplit(int64_t R, int64_t N) {
    const int64_t row_tiles = (R + KN_BM - 1) / KN_BM;
    int64_t ns = (1024 + row_tiles - 1) / row_tiles;
    const int64_t max_ns = (N + 32 * KN_BN - 1) / (32 * KN_BN);   // at least 32 tiles per split
    if (ns > max_ns) ns = max_ns;
    if (ns < 1) ns = 1;
    return (int)ns;
}

bool knn_d_ok(int d) { return d == 8 || d == 16 || d == 32 || d == 64 || d == 128; }


template <int D>
int launch(const KnnArgs& a, const uint8_t* valid, float2* item, dim3 grid, size_t lds, hipStream_t s) {
    // the lists pass 64 KB together with the tile from k = 57 on: lift the default cap on dynamic LDS
    OTTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_knn<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_knn_items<D><<<(unsigned)((a.N + 255) / 256), 256, 0, s>>>(a.E, valid, a.N, a.metric, item);
    OTTO_HIP(hipGetLastError());
    k_knn<D><<<grid, 256, lds, s>>>(a);
    OTTO_HIP(hipGetLastError());
    return 0;
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_knn_workspace(int64_t n_rows, int64_t N, int32_t d, int32_t k, int32_t metric) {
    if (n_rows <= 0 || N <= 0 || N >= 0x7FFFFFFF || n_rows >= 0x7FFFFFFF || k < 1 || k > OTTO_KNN_MAX_K || !knn_d_ok(d) ||
        metric < OTTO_KNN_EUCLIDEAN || metric > OTTO_KNN_DOT)
        return 0;
    const int64_t Rpad = (n_rows + KN_BM - 1) / KN_BM * KN_BM;
    return KN_HDR + align256(N * 8) + (int64_t)knn_nsplit(n_rows, N) * Rpad * k * 8;
}

extern "C" int otto_knn_table(const float* d_E, int64_t N, int32_t d, const uint8_t* d_valid, const int32_t* d_rows,
                              int64_t n_rows, int32_t k, int32_t metric, int32_t* d_ids, float* d_dist, int32_t* d_n,
                              void* d_workspace, int64_t workspace_bytes, void* stream) {
    OTTO_REQUIRE(d_E && d_ids && d_dist && d_n && d_workspace, "null argument");
    OTTO_REQUIRE(N > 0 && N < 0x7FFFFFFF, "N = %lld outside (0, 2^31 - 1)", (long long)N);
    OTTO_REQUIRE(n_rows > 0 && n_rows < 0x7FFFFFFF, "n_rows = %lld outside (0, 2^31 - 1)", (long long)n_rows);
    OTTO_REQUIRE(d_rows || n_rows == N, "without d_rows the query aids are all N = %lld items (n_rows = %lld)", (long long)N,
                 (long long)n_rows);
    OTTO_REQUIRE(k >= 1 && k <= OTTO_KNN_MAX_K, "k must be in [1, %d] (got %d)", OTTO_KNN_MAX_K, k);
    OTTO_REQUIRE(knn_d_ok(d), "the neighbour table supports d in {8,16,32,64,128} (got %d)", d);
    OTTO_REQUIRE(metric >= OTTO_KNN_EUCLIDEAN && metric <= OTTO_KNN_DOT, "unknown metric %d", metric);
    OTTO_REQUIRE(workspace_bytes >= otto_knn_workspace(n_rows, N, d, k, metric), "workspace too small: %lld < %lld bytes",
                 (long long)workspace_bytes, (long long)otto_knn_workspace(n_rows, N, d, k, metric));
    hipStream_t s = (hipStream_t)stream;
    const int64_t row_tiles = (n_rows + KN_BM - 1) / KN_BM;
    const int64_t Rpad = row_tiles * KN_BM;
    const int ns = knn_nsplit(n_rows, N);
    int64_t per = (N + ns - 1) / ns;
    per = (per + KN_BN - 1) / KN_BN * KN_BN;
    char* ws = (char*)d_workspace;
    float2* item = (float2*)(ws + KN_HDR);
    float* part_s = (float*)(ws + KN_HDR + align256(N * 8));
    KnnArgs a;
    memset(&a, 0, sizeof a);
    a.E = d_E; a.item = item; a.rows = d_rows; a.R = n_rows; a.N = N; a.k = k; a.metric = metric; a.nsplit = ns;
    a.items_per_split = per; a.part_s = part_s; a.part_i = (int32_t*)(part_s + (size_t)ns * Rpad * k); a.err = (uint32_t*)ws;
    OTTO_HIP(hipMemsetAsync(a.err, 0, 4, s));
    const dim3 grid((unsigned)row_tiles, (unsigned)ns);
    const size_t lds = (size_t)KN_BM * k * 8;
    switch (d) {
        case 8: OTTO_TRY(launch<8>(a, d_valid, item, grid, lds, s)); break;
        case 16: OTTO_TRY(launch<16>(a, d_valid, item, grid, lds, s)); break;
        case 32: OTTO_TRY(launch<32>(a, d_valid, item, grid, lds, s)); break;
        case 64: OTTO_TRY(launch<64>(a, d_valid, item, grid, lds, s)); break;
        default: OTTO_TRY(launch<128>(a, d_valid, item, grid, lds, s)); break;
    }
    k_knn_merge<<<(unsigned)n_rows, 64, 0, s>>>(a, Rpad, d_ids, d_dist, d_n);
    OTTO_HIP(hipGetLastError());
    uint32_t bad = 0;
    OTTO_HIP(hipMemcpyAsync(&bad, a.err, 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (bad) {
        set_error("%u entr%s of d_rows outside [0, %lld): those rows were left empty", bad, bad == 1 ? "y" : "ies", (long long)N);
        return OTTO_EINVAL;
    }
    return 0;
}
