// Gradient-boosted forest scoring and per-session top-k (SPEC-FOREST; include/otto_forest.h).
//
// Host:   otto_forest_pack validates the unpacked trees and writes the packed image (layout in the header): float32
//         thresholds t32 = the largest float32 <= the float64 threshold, 16-byte nodes, whole trees gathered into groups
//         of at most OTTO_FOREST_GROUP_BYTES.
// Device, on the caller's stream:
//   k_forest_check   validates the header, the tree and group tables and every node's feature index of the image it is
//                    handed, so that k_forest can trust them; a mismatch sets the error word and k_forest does nothing.
//   k_forest         one lane per row, 256 rows per workgroup. The row tile is staged once into LDS transposed
//                    (feat[f][row]: a wave's lanes read their own bank whatever feature each of them asks for). The
//                    forest streams through one LDS buffer group by group: the next group is loaded into registers
//                    while the current one is walked. A tree larger than a group is walked from global memory. Each
//                    lane adds the leaf values of its row in tree order in float64. Every walk runs at most L - 1
//                    steps and range-checks the child and the leaf it ends on.
//   k_session_topk   one wave per session: its rows stream 64 at a time against the sorted list that topk.h keeps one
//                    entry per lane (key = order-preserving image of the float64 score, then the row position).
#include "common.h"
#include "wave.h"
#include "topk.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_forest.h"

#include <math.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace otto {
namespace {

constexpr uint32_t F_MAGIC = 0x3152464Fu;            // 'OFR1'
constexpr int F_ROWS = 256;                          // rows per workgroup
constexpr int F_GROUP16 = OTTO_FOREST_GROUP_BYTES / 16;
constexpr int F_STAGE = F_GROUP16 / F_ROWS;          // 16-byte units of the next group held per thread
static_assert(F_GROUP16 % F_ROWS == 0, "a group is a whole number of 16-byte units per thread");
// the error words: [0] written by k_forest_check only (k_forest reads it), [1] by the walks
constexpr int ERR_IMAGE = 0, ERR_WALK = 1;

struct FHeader {
    uint32_t magic, version;
    int32_t T, F, n_groups, max_leaves, total_nodes, total_leaves;
    int64_t total_bytes, off_trees, off_groups, off_blob;
};
static_assert(sizeof(FHeader) == 64, "packed header");
struct FTree { uint32_t off16; int32_t n_leaves; };
struct FGroup { int32_t first_tree, n_trees; uint32_t off16, len16; };

__host__ __device__ inline int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }
__host__ __device__ inline int64_t tree_units(int64_t L) { return ((L - 1) * 16 + L * 8 + 15) / 16; }
__host__ __device__ inline int64_t image_bytes(int64_t T, int64_t nodes, int64_t leaves) {
    return 64 + align16(T * 8) + T * 16 + nodes * 16 + leaves * 8 + T * 8;
}

struct ForestArgs {
    const char* img;
    int64_t packed_bytes;
    const float* X;
    int64_t ld, n_rows;
    int F, T;                  // T: only the leaf output checks it
    double* raw;
    double* acc;
    double divisor;
    int32_t* leaf;
    uint32_t* err;
};

// fixed grid: every block checks the header for itself, then the blocks share the groups and the trees
__global__ __launch_bounds__(256) void k_forest_check(ForestArgs a) {
    const FHeader h = *reinterpret_cast<const FHeader*>(a.img);
    bool ok = h.magic == F_MAGIC && h.version == 1 && h.T >= 1 && h.F == a.F && h.total_bytes == a.packed_bytes &&
              h.total_nodes >= 0 && h.total_leaves >= h.T && h.n_groups >= 1 && h.n_groups <= h.T &&
              (a.leaf == nullptr || h.T == a.T);
    ok = ok && h.total_bytes == image_bytes(h.T, h.total_nodes, h.total_leaves) && h.off_trees == 64 &&
         h.off_groups == 64 + align16((int64_t)h.T * 8) && h.off_blob == h.off_groups + (int64_t)h.T * 16;
    if (!ok) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(a.err + ERR_IMAGE, 1u);
        return;
    }
    const FTree* trees = reinterpret_cast<const FTree*>(a.img + h.off_trees);
    const FGroup* groups = reinterpret_cast<const FGroup*>(a.img + h.off_groups);
    const uint4* blob = reinterpret_cast<const uint4*>(a.img + h.off_blob);
    const int64_t blob16 = (h.total_bytes - h.off_blob) / 16;
    bool bad = false;
    // groups: consecutive, covering every tree once; each tree inside its group's byte range
    for (int g = blockIdx.x * 256 + threadIdx.x; g < h.n_groups; g += gridDim.x * 256) {
        const FGroup G = groups[g];
        const int want_first = g == 0 ? 0 : groups[g - 1].first_tree + groups[g - 1].n_trees;
        bool gok = G.n_trees >= 1 && G.first_tree == want_first && (int64_t)G.first_tree + G.n_trees <= h.T &&
                   G.len16 <= (uint32_t)F_GROUP16 && (int64_t)G.off16 + G.len16 <= blob16 && (G.len16 != 0 || G.n_trees == 1);
        if (g == h.n_groups - 1) gok = gok && G.first_tree + G.n_trees == h.T;
        if (gok) {
            for (int t = G.first_tree; t < G.first_tree + G.n_trees; ++t) {
                const FTree tr = trees[t];
                if (tr.n_leaves < 1 || tr.n_leaves > OTTO_FOREST_MAX_LEAVES) { gok = false; break; }
                const int64_t u = tree_units(tr.n_leaves);
                if (G.len16 ? (tr.off16 < G.off16 || (int64_t)tr.off16 + u > (int64_t)G.off16 + G.len16)
                            : ((int64_t)tr.off16 + u > blob16)) { gok = false; break; }
            }
        }
        bad |= !gok;
    }
    if (__syncthreads_or(bad)) {          // the trees' ranges are not to be trusted
        if (threadIdx.x == 0) atomicOr(a.err + ERR_IMAGE, 1u);
        return;
    }
    // nodes: feature index and missing type (a tree's range was checked by the block that owns its group; a tree
    // outside the blob is skipped here and reported there)
    for (int t = blockIdx.x; t < h.T; t += gridDim.x) {
        const FTree tr = trees[t];
        if (tr.n_leaves < 1 || tr.n_leaves > OTTO_FOREST_MAX_LEAVES || (int64_t)tr.off16 + tree_units(tr.n_leaves) > blob16) continue;
        for (int i = threadIdx.x; i < tr.n_leaves - 1; i += 256) {
            const uint32_t y = blob[tr.off16 + i].y;
            bad |= (y & 0xFFFFu) >= (uint32_t)h.F || ((y >> 16) & 3u) == 3u || (y >> 19) != 0;
        }
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(a.err + ERR_IMAGE, 1u);
}

// walk one tree for this lane's row; nodes -> the tree's (L-1) nodes followed by its L float64 leaf values.
// Returns the leaf index, or -1 when the walk did not end on a leaf of this tree within L - 1 steps.
__device__ __forceinline__ int walk_tree(const uint4* nodes, int L, const float* feat_lane) {
    const int nint = L - 1;
    int c = nint > 0 ? 0 : -1;
    for (int step = 0; step < nint; ++step) {
        if ((unsigned)c >= (unsigned)nint) break;          // a leaf (negative), or a child outside the tree
        const uint4 nd = nodes[c];
        float x = feat_lane[(nd.y & 0xFFFFu) * F_ROWS];
        const uint32_t missing = (nd.y >> 16) & 3u;
        const bool nan = x != x;
        if (nan && missing != 2u) x = 0.f;
        bool left = x <= __uint_as_float(nd.x);
        if ((missing == 1u && fabsf(x) <= 1e-35f) || (missing == 2u && nan)) left = (nd.y >> 18) & 1u;
        c = left ? (int)nd.z : (int)nd.w;
    }
    const int leaf = ~c;
    return (c < 0 && leaf < L) ? leaf : -1;
}

// this thread's share of the next group: global -> registers
__device__ __forceinline__ void load_group(uint4 (&stage)[F_STAGE], const uint4* src, uint32_t len16, int tid) {
#pragma unroll
    for (int q = 0; q < F_STAGE; ++q) {
        const uint32_t i = tid + q * F_ROWS;
        stage[q] = i < len16 ? src[i] : make_uint4(0u, 0u, 0u, 0u);
    }
}

template <bool LEAF>
__global__ __launch_bounds__(256) void k_forest(ForestArgs a) {
    extern __shared__ uint4 s_mem[];                 // the tree group, then float feat[F][256]
    if (a.err[ERR_IMAGE]) return;                           // k_forest_check refused the image
    uint4* const s_grp = s_mem;
    float* const s_feat = reinterpret_cast<float*>(s_mem + F_GROUP16);
    const FHeader* h = reinterpret_cast<const FHeader*>(a.img);
    const FTree* trees = reinterpret_cast<const FTree*>(a.img + h->off_trees);
    const FGroup* groups = reinterpret_cast<const FGroup*>(a.img + h->off_groups);
    const uint4* blob = reinterpret_cast<const uint4*>(a.img + h->off_blob);
    const int n_groups = h->n_groups, T = h->T;
    const int F = a.F;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * F_ROWS;
    const int rows_here = (int)(a.n_rows - row0 < F_ROWS ? a.n_rows - row0 : F_ROWS);

    // the row tile, transposed: consecutive threads read consecutive floats of the row-major matrix
    for (int i = tid; i < F_ROWS * F; i += F_ROWS) {
        const int r = i / F, f = i - r * F;
        s_feat[f * F_ROWS + r] = r < rows_here ? a.X[(row0 + r) * a.ld + f] : 0.f;
    }

    uint4 stage[F_STAGE];
    FGroup G = groups[0];
    load_group(stage, blob + G.off16, G.len16, tid);
    const float* const feat_lane = s_feat + tid;
    double sum = 0.0;
    bool bad = false;
    for (int g = 0; g < n_groups; ++g) {
        __syncthreads();                             // the previous group is consumed (first time: the tile is staged)
#pragma unroll
        for (int q = 0; q < F_STAGE; ++q) {
            const uint32_t i = tid + q * F_ROWS;
            if (i < G.len16) s_grp[i] = stage[q];
        }
        __syncthreads();
        const FGroup cur = G;
        if (g + 1 < n_groups) {                      // the next group's loads fly under this group's walks
            G = groups[g + 1];
            load_group(stage, blob + G.off16, G.len16, tid);
        }
        FTree tr = trees[cur.first_tree];
        for (int t = cur.first_tree; t < cur.first_tree + cur.n_trees; ++t) {
            const FTree me = tr;
            if (t + 1 < T) tr = trees[t + 1];
            int leaf;
            if (cur.len16) leaf = walk_tree(s_grp + (me.off16 - cur.off16), me.n_leaves, feat_lane);
            else leaf = walk_tree(blob + me.off16, me.n_leaves, feat_lane);
            bad |= leaf < 0;
            if (leaf < 0) leaf = 0;
            if (LEAF) {
                if (tid < rows_here) a.leaf[(row0 + tid) * T + t] = leaf;
            } else {
                if (cur.len16) sum += reinterpret_cast<const double*>(s_grp + (me.off16 - cur.off16) + (me.n_leaves - 1))[leaf];
                else sum += reinterpret_cast<const double*>(blob + me.off16 + (me.n_leaves - 1))[leaf];
            }
        }
    }
    if (bad) atomicOr(a.err + ERR_WALK, 1u);
    if (!LEAF && tid < rows_here) {
        if (a.raw) a.raw[row0 + tid] = sum;
        if (a.acc) a.acc[row0 + tid] += (double)(float)sum / a.divisor;
    }
}

__global__ __launch_bounds__(256) void k_session_topk(const double* score, const int32_t* aid, const int64_t* row_off, int64_t S,
                                                      int64_t n_rows, int k, int32_t* top_aid, double* top_score, int32_t* n_out,
                                                      uint32_t* err) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= S) return;
    const unsigned l = lane_id();
    int64_t lo = row_off[s], hi = row_off[s + 1];
    if (!(lo >= 0 && lo <= hi && hi <= n_rows && hi - lo < (1ll << 32))) {
        if (l == 0) atomicAdd(err, 1u);
        lo = hi = 0;
    }
    KeyW best;
    kclear(best);
    for (int64_t p0 = lo; p0 < hi; p0 += 64) {
        const int64_t p = p0 + l;
        KeyW c;
        kclear(c);
        if (p < hi) { c.w = score_key(score[p]); c.y = (uint32_t)(p - lo); }
        wave_topk_push(best, c, k);
    }
    const bool filled = (int)l < k && kvalid(best);
    if ((int)l < k) {
        top_aid[s * k + l] = filled ? aid[lo + best.y] : -1;
        top_score[s * k + l] = filled ? score[lo + best.y] : -INFINITY;   // the stored bits, -0.0 and NaN payloads included
    }
    if (l == 0) n_out[s] = (int32_t)(hi - lo < k ? hi - lo : k);
}

// the largest float32 <= t (t not NaN)
float floor_f32(double t) {
    float f = (float)t;
    if ((double)f > t) f = nextafterf(f, -INFINITY);
    return f;
}

int run_forest(ForestArgs a, hipStream_t s) {
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_FOREST, 256, &scratch, s));
    a.err = (uint32_t*)scratch;
    OTTO_HIP(hipMemsetAsync(a.err, 0, 8, s));
    k_forest_check<<<64, 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    const size_t lds = (size_t)OTTO_FOREST_GROUP_BYTES + (size_t)a.F * F_ROWS * 4;
    const unsigned grid = (unsigned)((a.n_rows + F_ROWS - 1) / F_ROWS);
    // the tile passes 64 KB together with the group from F = 41 on: lift the default cap on dynamic LDS
    if (a.leaf) {
        OTTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_forest<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_forest<true><<<grid, F_ROWS, lds, s>>>(a);
    } else {
        OTTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_forest<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_forest<false><<<grid, F_ROWS, lds, s>>>(a);
    }
    OTTO_HIP(hipGetLastError());
    uint32_t bad[2] = {0, 0};
    OTTO_HIP(hipMemcpyAsync(bad, a.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (bad[ERR_IMAGE]) {
        set_error("the packed forest image does not match its header, packed_bytes = %lld, F = %d%s: nothing was computed",
                  (long long)a.packed_bytes, a.F, a.leaf ? " or T" : "");
        return OTTO_EINVAL;
    }
    if (bad[ERR_WALK]) {
        set_error("a tree walk did not reach a leaf of its tree within n_leaves - 1 steps: the packed image is damaged");
        return OTTO_EINVAL;
    }
    return 0;
}

int check_predict_args(const void* d_packed, int64_t packed_bytes, const float* d_X, int64_t ld, int64_t n_rows, int32_t F) {
    OTTO_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 39), "n_rows = %lld outside [0, 2^39)", (long long)n_rows);
    OTTO_REQUIRE(d_packed && packed_bytes >= 64 + 16 + 16, "no packed image (packed_bytes = %lld)", (long long)packed_bytes);
    OTTO_REQUIRE(((uintptr_t)d_packed & 15) == 0, "d_packed must be 16-byte aligned");
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    OTTO_REQUIRE(ld >= F, "row stride ld = %lld below F = %d", (long long)ld, F);
    OTTO_REQUIRE(d_X || n_rows == 0, "null d_X");
    return 0;
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_forest_packed_bytes(int32_t T, int64_t total_nodes, int64_t total_leaves) {
    if (T < 1 || total_leaves < T || total_nodes != total_leaves - T || total_leaves > 0x7FFFFFFF) return 0;
    return image_bytes(T, total_nodes, total_leaves);
}

extern "C" int otto_forest_pack(int32_t T, int32_t F, const int64_t* node_off, const int64_t* leaf_off,
                                const int32_t* split_feature, const double* threshold, const int8_t* decision_type,
                                const int32_t* left_child, const int32_t* right_child, const double* leaf_value, void* out,
                                int64_t out_bytes) {
    OTTO_REQUIRE(T >= 1, "a forest needs at least one tree (T = %d)", T);
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    OTTO_REQUIRE(node_off && leaf_off && leaf_value && out, "null argument");
    OTTO_REQUIRE(node_off[0] == 0 && leaf_off[0] == 0, "node_off[0] and leaf_off[0] must be 0");
    for (int t = 0; t < T; ++t) {
        const int64_t L = leaf_off[t + 1] - leaf_off[t], n = node_off[t + 1] - node_off[t];
        OTTO_REQUIRE(L >= 1 && L <= OTTO_FOREST_MAX_LEAVES, "tree %d: %lld leaves outside [1, %d]", t, (long long)L, OTTO_FOREST_MAX_LEAVES);
        OTTO_REQUIRE(n == L - 1, "tree %d: %lld internal nodes for %lld leaves", t, (long long)n, (long long)L);
    }
    const int64_t total_nodes = node_off[T], total_leaves = leaf_off[T];
    const int64_t bytes = otto_forest_packed_bytes(T, total_nodes, total_leaves);
    OTTO_REQUIRE(bytes > 0, "forest too large to pack (%lld leaves)", (long long)total_leaves);
    OTTO_REQUIRE(out_bytes >= bytes, "output buffer too small: %lld < %lld bytes", (long long)out_bytes, (long long)bytes);
    OTTO_REQUIRE(total_nodes == 0 || (split_feature && threshold && decision_type && left_child && right_child), "null node array");

    // structure: every internal node and every leaf reached exactly once from the root
    std::vector<int> stack;
    std::vector<uint8_t> seen_node, seen_leaf;
    for (int t = 0; t < T; ++t) {
        const int64_t n0 = node_off[t], l0 = leaf_off[t];
        const int L = (int)(leaf_off[t + 1] - l0), nint = L - 1;
        for (int i = 0; i < L; ++i)
            OTTO_REQUIRE(std::isfinite(leaf_value[l0 + i]), "tree %d: leaf %d has a non-finite value", t, i);
        for (int i = 0; i < nint; ++i) {
            const int dt = (uint8_t)decision_type[n0 + i];
            OTTO_REQUIRE((dt & 1) == 0, "tree %d node %d: categorical split (decision_type %d)", t, i, dt);
            OTTO_REQUIRE(((dt >> 2) & 3) != 3 && (dt >> 4) == 0, "tree %d node %d: unknown decision_type %d", t, i, dt);
            OTTO_REQUIRE(split_feature[n0 + i] >= 0 && split_feature[n0 + i] < F, "tree %d node %d: split_feature %d outside [0, %d)", t,
                         i, split_feature[n0 + i], F);
            OTTO_REQUIRE(threshold[n0 + i] == threshold[n0 + i], "tree %d node %d: NaN threshold", t, i);
        }
        seen_node.assign(nint, 0);
        seen_leaf.assign(L, 0);
        stack.clear();
        if (nint == 0) seen_leaf[0] = 1;
        else { stack.push_back(0); seen_node[0] = 1; }
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            const int32_t kids[2] = {left_child[n0 + i], right_child[n0 + i]};
            for (int32_t c : kids) {
                if (c >= 0) {
                    OTTO_REQUIRE(c < nint, "tree %d node %d: child %d outside the tree", t, i, c);
                    OTTO_REQUIRE(!seen_node[c], "tree %d: internal node %d is reached twice (a cycle or a shared subtree)", t, c);
                    seen_node[c] = 1;
                    stack.push_back(c);
                } else {
                    OTTO_REQUIRE(~c < L, "tree %d node %d: leaf %d outside the tree", t, i, ~c);
                    OTTO_REQUIRE(!seen_leaf[~c], "tree %d: leaf %d is reached twice", t, ~c);
                    seen_leaf[~c] = 1;
                }
            }
        }
        for (int i = 0; i < nint; ++i) OTTO_REQUIRE(seen_node[i], "tree %d: internal node %d is unreachable", t, i);
        for (int i = 0; i < L; ++i) OTTO_REQUIRE(seen_leaf[i], "tree %d: leaf %d is unreachable", t, i);
    }

    char* img = (char*)out;
    memset(img, 0, (size_t)bytes);
    FHeader h;
    memset(&h, 0, sizeof h);
    h.magic = F_MAGIC; h.version = 1; h.T = T; h.F = F; h.total_nodes = (int32_t)total_nodes; h.total_leaves = (int32_t)total_leaves;
    h.total_bytes = bytes; h.off_trees = 64; h.off_groups = 64 + align16((int64_t)T * 8); h.off_blob = h.off_groups + (int64_t)T * 16;
    FTree* trees = (FTree*)(img + h.off_trees);
    FGroup* groups = (FGroup*)(img + h.off_groups);
    char* blob = img + h.off_blob;
    int64_t off16 = 0;
    int ng = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t n0 = node_off[t], l0 = leaf_off[t];
        const int L = (int)(leaf_off[t + 1] - l0);
        const int64_t u = tree_units(L);
        if (L > h.max_leaves) h.max_leaves = L;
        trees[t].off16 = (uint32_t)off16;
        trees[t].n_leaves = L;
        // a tree joins the open group while the group stays within the LDS budget; a tree above the budget stands alone
        const bool fits = u <= F_GROUP16;
        if (ng > 0 && fits && groups[ng - 1].len16 != 0 && groups[ng - 1].len16 + u <= F_GROUP16) {
            groups[ng - 1].n_trees += 1;
            groups[ng - 1].len16 += (uint32_t)u;
        } else {
            groups[ng].first_tree = t; groups[ng].n_trees = 1; groups[ng].off16 = (uint32_t)off16; groups[ng].len16 = fits ? (uint32_t)u : 0u;
            ++ng;
        }
        uint32_t* nd = (uint32_t*)(blob + off16 * 16);
        for (int i = 0; i < L - 1; ++i) {
            const int dt = (uint8_t)decision_type[n0 + i];
            const float t32 = floor_f32(threshold[n0 + i]);
            memcpy(&nd[4 * i], &t32, 4);
            nd[4 * i + 1] = (uint32_t)split_feature[n0 + i] | (uint32_t)((dt >> 2) & 3) << 16 | (uint32_t)((dt >> 1) & 1) << 18;
            nd[4 * i + 2] = (uint32_t)left_child[n0 + i];
            nd[4 * i + 3] = (uint32_t)right_child[n0 + i];
        }
        memcpy(blob + off16 * 16 + (int64_t)(L - 1) * 16, leaf_value + l0, (size_t)L * 8);
        off16 += u;
    }
    h.n_groups = ng;
    memcpy(img, &h, sizeof h);
    return 0;
}

extern "C" int otto_forest_predict(const void* d_packed, int64_t packed_bytes, const float* d_X, int64_t ld, int64_t n_rows,
                                   int32_t F, double* d_raw, double* d_acc, double divisor, void* stream) {
    OTTO_TRY(check_predict_args(d_packed, packed_bytes, d_X, ld, n_rows, F));
    OTTO_REQUIRE(d_acc == nullptr || (divisor == divisor && divisor != 0.0), "divisor must be a non-zero number");
    if (n_rows == 0) return 0;
    OTTO_REQUIRE(d_raw || d_acc, "neither d_raw nor d_acc given");
    ForestArgs a;
    memset(&a, 0, sizeof a);
    a.img = (const char*)d_packed; a.packed_bytes = packed_bytes; a.X = d_X; a.ld = ld; a.n_rows = n_rows; a.F = F;
    a.raw = d_raw; a.acc = d_acc; a.divisor = divisor;
    return run_forest(a, (hipStream_t)stream);
}

extern "C" int otto_forest_leaves(const void* d_packed, int64_t packed_bytes, const float* d_X, int64_t ld, int64_t n_rows,
                                  int32_t F, int32_t T, int32_t* d_leaf, void* stream) {
    OTTO_TRY(check_predict_args(d_packed, packed_bytes, d_X, ld, n_rows, F));
    OTTO_REQUIRE(T >= 1, "T = %d", T);
    if (n_rows == 0) return 0;
    OTTO_REQUIRE(d_leaf, "null d_leaf");
    ForestArgs a;
    memset(&a, 0, sizeof a);
    a.img = (const char*)d_packed; a.packed_bytes = packed_bytes; a.X = d_X; a.ld = ld; a.n_rows = n_rows; a.F = F; a.T = T;
    a.leaf = d_leaf;
    return run_forest(a, (hipStream_t)stream);
}

extern "C" int otto_forest_session_topk(const double* d_score, const int32_t* d_aid, const int64_t* d_row_off, int64_t S,
                                        int64_t n_rows, int32_t k, int32_t* d_top_aid, double* d_top_score, int32_t* d_n,
                                        void* stream) {
    OTTO_REQUIRE(k >= 1 && k <= OTTO_FOREST_MAX_K, "k must be in [1, %d] (got %d)", OTTO_FOREST_MAX_K, k);
    OTTO_REQUIRE(S >= 0 && S < ((int64_t)1 << 33), "S = %lld outside [0, 2^33)", (long long)S);
    OTTO_REQUIRE(n_rows >= 0, "n_rows = %lld", (long long)n_rows);
    if (S == 0) return 0;
    OTTO_REQUIRE(d_row_off && d_top_aid && d_top_score && d_n, "null argument");
    OTTO_REQUIRE((d_score && d_aid) || n_rows == 0, "null d_score or d_aid");
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_FOREST_TOPK, 256, &scratch, s));
    uint32_t* err = (uint32_t*)scratch;
    OTTO_HIP(hipMemsetAsync(err, 0, 4, s));
    k_session_topk<<<(unsigned)((S + 3) / 4), 256, 0, s>>>(d_score, d_aid, d_row_off, S, n_rows, k, d_top_aid, d_top_score, d_n, err);
    OTTO_HIP(hipGetLastError());
    uint32_t bad = 0;
    OTTO_HIP(hipMemcpyAsync(&bad, err, 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (bad) {
        set_error("%u session%s with row_off not in 0 <= row_off[s] <= row_off[s+1] <= n_rows = %lld: left empty", bad,
                  bad == 1 ? "" : "s", (long long)n_rows);
        return OTTO_EINVAL;
    }
    return 0;
}
