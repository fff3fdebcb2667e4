// XGBoost-style ranker family (SPEC-XGB; include/otto_xgb.h): the rank:pairwise objective and
// depth-wise tree growth. The ranking, the histogram, split-search and partition bodies are SPEC-GBDT's (gbdt_device.h).
//
// Device, on the caller's stream:
//   k_xgb_pairwise_short / _long   one workgroup per query (short: one wave and LDS for 128 rows, a launch over all
//                    queries; long: four waves and LDS for 1024 rows, 1024 workgroups that walk the queries and take the
//                    longer ones). rank_query ranks it in LDS; the label counts give every bucket's first
//                    record position, a row's place inside its bucket is the number of earlier ranks with its label; one
//                    thread per record position draws the partner and leaves the pair (ranks of high and low, g, 2h) in
//                    LDS; one thread per row then walks the pair list in ascending index and adds the pairs it is part
//                    of: no float atomics, the order of every sum is pinned. Both are templates on NDCG: true is
//                    rank:ndcg (SPEC-OBJ, include/otto_objective.h): thread 0 also adds the query's ideal DCG from the
//                    label counts, and the pair thread scales g and 2h by the pair's |delta NDCG|; false is rank:pairwise,
//                    with that code compiled out.
//   k_level_hist     grid = (row chunks of all nodes of the level, groups of 8 features). A workgroup finds its node by
//                    binary search over the nodes' first chunk, then is k_hist's body (hist_block) on that node's rows
//                    and histogram slot.
//   k_level_sub      larger sibling = parent - smaller sibling, all nodes of the level in one launch.
//   k_level_split    one workgroup per live node: best_split_block on the node's slot, records side by side.
//   k_level_part_count / _scan / _scatter   the stable partition of SPEC-GBDT, segmented: blocks of 2048 rows of every
//                    node that splits, one workgroup per node scans its own blocks, the scatter stays inside the node's
//                    range of the row list.
// Host: otto_xgb_grow_tree reads the level's split records with one copy and one synchronisation, decides the splits,
// numbers the nodes and uploads the descriptors of the next level's launches.
#include "gbdt_device.h"
#include "../../include/otto_xgb.h"

#include <math.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace otto {
namespace {

constexpr int MAX_LEVEL_NODES = 1 << OTTO_XGB_MAX_DEPTH;    // descriptors of one launch

// one node of a level launch; the host array of the level entry points has the same layout (word 4 ignored)
struct LevelNode {
    int32_t begin, cnt;             // its rows: [begin, begin + cnt) of the row list
    int32_t slot, slot2;            // histogram slots (hist: filled; sub: slot2 -= slot; split: searched)
    int32_t first;                  // the first work item (row chunk, partition block) of this node in the launch
    int32_t feature, bin, default_left;
};
static_assert(sizeof(LevelNode) == 32, "the level entry points read int32 [n_nodes, 8]");

// the node that owns work item `item`: the last one with first <= item (nodes without items share their successor's first)
__device__ __forceinline__ int find_node(const LevelNode* nodes, int n_nodes, int item) {
    int lo = 0, hi = n_nodes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (nodes[mid].first <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// rank:pairwise
// ---------------------------------------------------------------------------------------------------------------------
struct PairArgs {
    const double* score;
    const int32_t* label;
    const int64_t* query_off;
    int64_t n;
    const double* sigmoid;
    double sig_lo, sig_factor;
    uint64_t seed;
    const double* discount;   // LambdaMART weighting only
    double* grad;
    double* hess;
    uint32_t* err;
};

constexpr uint16_t NO_PAIR = 0xFFFF;
constexpr int SHORT_QUERY = 128;    // rows of a query the one-wave kernel takes
constexpr int LONG_BLOCKS = 1024;   // grid of the kernel that takes the longer ones

// the LDS of one query of at most CAP rows: rank_query's arrays (QueryLds without LambdaRank's extras), then the pairs
template <int CAP>
struct PairLds {
    uint64_t key[CAP];        // by position; after the ranking: 2h of a pair, as bits
    double score[CAP];        // by rank
    double disc[CAP];         // g of a pair
    uint16_t pos[CAP];        // by rank: the row's position in the query
    uint8_t label[CAP];       // by rank
    uint32_t lcnt[OTTO_GBDT_MAX_LABEL + 1];
    uint32_t start[OTTO_GBDT_MAX_LABEL + 1];    // first record position of a label's bucket
    uint16_t rec[CAP];        // record position -> rank
    uint16_t hi[CAP], lo[CAP];    // pair index -> rank of its high / low row
    double inv_idcg;          // LambdaMART weighting only
};

// one query, rows [lo, lo + cnt), by the whole workgroup; cnt >= 1. Ends without a barrier. NDCG: SPEC-OBJ's rank:ndcg, every
// pair weighted by the |delta NDCG| of swapping its two rows; false: rank:pairwise, the code the flag adds compiled out.
template <bool NDCG, int CAP>
__device__ __forceinline__ void pair_query(PairLds<CAP>& s, const PairArgs& a, int64_t lo, int cnt) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x;
    rank_query(s, a.score, a.label, lo, cnt, a.err);
    if (s.lcnt[s.label[0]] == (uint32_t)cnt) return;    // one bucket: m == 0 for every row, nothing is drawn
    if (tid == 0) {
        uint32_t at = 0;
        for (int lab = OTTO_GBDT_MAX_LABEL; lab >= 0; --lab) { s.start[lab] = at; at += s.lcnt[lab]; }
        if constexpr (NDCG) {
            double idcg = 0.0;
            int r = 0;
            for (int lab = OTTO_GBDT_MAX_LABEL; lab >= 0; --lab) {
                const double gain = (double)((1ull << lab) - 1ull);
                for (uint32_t c = s.lcnt[lab]; c > 0; --c, ++r) idcg = idcg + gain * a.discount[r];
            }
            s.inv_idcg = idcg == 0.0 ? 0.0 : 1.0 / idcg;
        }
    }
    __syncthreads();
    for (int r = tid; r < cnt; r += nt) {
        const uint8_t lab = s.label[r];
        uint32_t within = 0;
        for (int o = 0; o < r; ++o) within += s.label[o] == lab ? 1u : 0u;
        s.rec[s.start[lab] + within] = (uint16_t)r;
    }
    __syncthreads();
    const double top = (double)(OTTO_GBDT_SIGMOID_BINS - 1);
    for (int pid = tid; pid < cnt; pid += nt) {
        const int r = s.rec[pid];
        const int lab = s.label[r];
        const uint32_t i = s.start[lab], j = i + s.lcnt[lab];
        const uint64_t m = (uint64_t)i + (uint64_t)(cnt - (int)j);
        if (m == 0) { s.hi[pid] = NO_PAIR; s.lo[pid] = NO_PAIR; continue; }
        const uint64_t u = row_key(a.seed, (uint64_t)(lo + s.pos[r])) % m;
        int hi_r, lo_r;
        if (u < i) { hi_r = s.rec[u]; lo_r = r; }
        else { hi_r = r; lo_r = s.rec[u + (j - i)]; }
        const double d = s.score[lo_r] - s.score[hi_r];
        double x = (d - a.sig_lo) * a.sig_factor;
        x = x > 0.0 ? x : 0.0;                          // NaN -> 0
        x = x < top ? x : top;
        const double p = a.sigmoid[(size_t)x];
        const double g = p - 1.0;
        double h = p * (1.0 - p);
        h = h > 1e-16 ? h : 1e-16;
        s.hi[pid] = (uint16_t)hi_r;
        s.lo[pid] = (uint16_t)lo_r;
        if constexpr (NDCG) {
            const double dg = (double)((1ull << s.label[hi_r]) - 1ull) - (double)((1ull << s.label[lo_r]) - 1ull);
            const double delta = fabs(dg * (a.discount[hi_r] - a.discount[lo_r])) * s.inv_idcg;
            s.disc[pid] = g * delta;
            s.key[pid] = (uint64_t)__double_as_longlong(2.0 * h * delta);
        } else {
            s.disc[pid] = g;
            s.key[pid] = (uint64_t)__double_as_longlong(2.0 * h);
        }
    }
    __syncthreads();
    for (int r = tid; r < cnt; r += nt) {
        double g = 0.0, h = 0.0;
        for (int pid = 0; pid < cnt; ++pid) {
            const int hi_r = s.hi[pid], lo_r = s.lo[pid];
            if (hi_r == r) {
                g = g + s.disc[pid];
                h = h + __longlong_as_double((long long)s.key[pid]);
            } else if (lo_r == r) {
                g = g - s.disc[pid];
                h = h + __longlong_as_double((long long)s.key[pid]);
            }
        }
        const int64_t row = lo + s.pos[r];
        a.grad[row] = g;
        a.hess[row] = h;
    }
}

// one workgroup of one wave per query: the queries of at most SHORT_QUERY rows (4.7 KB of LDS, so that a CU holds its 32
// waves); it also counts the queries the spec refuses
template <bool NDCG>
__global__ __launch_bounds__(64) void k_xgb_pairwise_short(PairArgs a) {
    __shared__ PairLds<SHORT_QUERY> s;
    int64_t lo;
    int cnt;
    if (!query_range(a.query_off, blockIdx.x, a.n, &lo, &cnt, a.err)) return;   // grad / hess were zeroed
    if (cnt == 0 || cnt > SHORT_QUERY) return;
    pair_query<NDCG>(s, a, lo, cnt);
}

// the longer queries: workgroup b walks queries [b * per, (b + 1) * per) and works on those above SHORT_QUERY rows
template <bool NDCG>
__global__ __launch_bounds__(256) void k_xgb_pairwise_long(PairArgs a, int64_t Q, int64_t per) {
    __shared__ PairLds<MAXQ> s;
    const int64_t q1 = ((int64_t)blockIdx.x + 1) * per < Q ? ((int64_t)blockIdx.x + 1) * per : Q;
    for (int64_t q = (int64_t)blockIdx.x * per; q < q1; ++q) {
        const int64_t lo = a.query_off[q], hi = a.query_off[q + 1];
        if (!(lo >= 0 && lo <= hi && hi <= a.n && hi - lo <= MAXQ) || hi - lo <= SHORT_QUERY) continue;
        pair_query<NDCG>(s, a, lo, (int)(hi - lo));
        __syncthreads();                                // the next query reuses the LDS
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// level kernels
// ---------------------------------------------------------------------------------------------------------------------
template <bool LIST>
__global__ __launch_bounds__(HIST_THREADS) void k_level_hist(const uint8_t* bins, int64_t n, int F, const int2* gh, const int32_t* rows,
                                                             const LevelNode* nodes, int n_nodes, int64_t chunk,
                                                             unsigned long long* hist0, int64_t words, uint32_t* err,
                                                             const int32_t* feats, int n_list) {
    const LevelNode nd = nodes[find_node(nodes, n_nodes, (int)blockIdx.x)];
    auto range = [&](int64_t* i0, int64_t* i1) {
        const int64_t end = (int64_t)nd.begin + nd.cnt;
        *i0 = (int64_t)nd.begin + (int64_t)((int)blockIdx.x - nd.first) * chunk;
        *i1 = *i0 + chunk < end ? *i0 + chunk : end;
    };
    hist_block<LIST>(bins, n, F, gh, rows, range, blockIdx.y * HIST_FG, hist0 + (int64_t)nd.slot * words, err, feats, n_list);
}

__global__ __launch_bounds__(256) void k_level_sub(const LevelNode* nodes, int64_t* hist0, int64_t words) {
    const LevelNode nd = nodes[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (nd.slot2 >= 0 && i < words) hist0[(int64_t)nd.slot2 * words + i] -= hist0[(int64_t)nd.slot * words + i];
}

template <bool LIST>
__global__ __launch_bounds__(256) void k_level_split(const LevelNode* nodes, const int64_t* hist0, int64_t words, int F,
                                                     const int32_t* n_edges, const int32_t* exps, SplitParams p, const int32_t* feats,
                                                     int n_list, int64_t* out) {
    best_split_block<LIST>(hist0 + (int64_t)nodes[blockIdx.x].slot * words, out + (int64_t)blockIdx.x * SW, F, n_edges, exps, p, feats,
                           n_list);
}

__global__ __launch_bounds__(256) void k_level_part_count(const uint8_t* bins, int64_t n, const int32_t* rows, const LevelNode* nodes,
                                                          int n_nodes, uint32_t* block_left, uint32_t* err) {
    const LevelNode nd = nodes[find_node(nodes, n_nodes, (int)blockIdx.x)];
    part_count_block(bins + (int64_t)nd.feature * n, n, nd.bin, nd.default_left, rows + nd.begin, nd.cnt,
                     (int64_t)((int)blockIdx.x - nd.first) * PART_ROWS, block_left + blockIdx.x, err);
}

__global__ __launch_bounds__(256) void k_level_part_scan(const LevelNode* nodes, uint32_t* block_left, int64_t* n_left) {
    const LevelNode nd = nodes[blockIdx.x];
    part_scan_block(block_left + nd.first, (uint32_t)part_blocks(nd.cnt), n_left + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_level_part_scatter(const uint8_t* bins, int64_t n, const int32_t* rows, const LevelNode* nodes,
                                                            int n_nodes, const uint32_t* block_before, const int64_t* n_left,
                                                            int32_t* out) {
    const int d = find_node(nodes, n_nodes, (int)blockIdx.x);
    const LevelNode nd = nodes[d];
    part_scatter_block(bins + (int64_t)nd.feature * n, n, nd.bin, nd.default_left, rows + nd.begin, nd.cnt,
                       (int64_t)((int)blockIdx.x - nd.first) * PART_ROWS, block_before[blockIdx.x], n_left[d], out + nd.begin);
}

__global__ __launch_bounds__(256) void k_iota(int32_t* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------------------------------
// host: the level launches
// ---------------------------------------------------------------------------------------------------------------------
struct LevelWork {          // the part of the workspace a level launch needs
    int64_t nodes, block_left, n_left, bytes;
};
LevelWork level_work(int64_t n_rows) {
    LevelWork w;
    int64_t at = 0;
    w.nodes = at; at += align256((int64_t)3 * MAX_LEVEL_NODES * (int64_t)sizeof(LevelNode));   // split, partition, hist
    w.block_left = at; at += align256((part_blocks(n_rows) + MAX_LEVEL_NODES) * 4);            // a node ends in one partial block
    w.n_left = at; at += align256((int64_t)MAX_LEVEL_NODES * 8);
    w.bytes = at;
    return w;
}

struct WorkLayout {
    int64_t level, rows_a, rows_b, split, hist, total;
    int slots;
};
WorkLayout work_layout(int64_t n, int32_t F, int32_t max_depth) {
    WorkLayout w;
    int64_t at = 0;
    w.level = at; at += level_work(n).bytes;
    w.rows_a = at; at += align256(n * 4);
    w.rows_b = at; at += align256(n * 4);
    w.split = at; at += align256((int64_t)MAX_LEVEL_NODES * SW * 8);
    w.slots = 1 << (max_depth - 1);
    w.hist = at; at += (int64_t)w.slots * 3 * F * 256 * 8;
    w.total = at;
    return w;
}

// rows per histogram work item: about 512 items for the level, never below 2048 rows (launch_hist's rule)
int64_t level_chunk(int64_t total_rows) {
    const int64_t chunk = (total_rows + 511) / 512;
    return chunk < 2048 ? 2048 : (chunk + HIST_THREADS - 1) / HIST_THREADS * HIST_THREADS;
}

// uploads the descriptors (h must stay alive until the stream has passed the copy) with `first` set per `per` rows an item
int upload_nodes(std::vector<LevelNode>& h, int64_t per, LevelNode* d_nodes, int64_t* items, hipStream_t s) {
    int64_t at = 0;
    for (LevelNode& nd : h) {
        nd.first = (int32_t)at;
        if (per) at += (nd.cnt + per - 1) / per;
    }
    *items = at;
    OTTO_HIP(hipMemcpyAsync(d_nodes, h.data(), h.size() * sizeof(LevelNode), hipMemcpyHostToDevice, s));
    return 0;
}

// zeroes the slot of every node, fills it from the node's rows, then slot2 -= slot where slot2 >= 0
int launch_level_hist(const uint8_t* bins, int64_t n, int F, const int32_t* gh, const int32_t* rows, std::vector<LevelNode>& h,
                      LevelNode* d_nodes, int64_t* hist0, uint32_t* err, const int32_t* feats, int n_list, hipStream_t s) {
    const int64_t words = (int64_t)3 * F * 256;
    int64_t total = 0;
    bool any_sub = false;
    int run0 = 0, run1 = 0;                             // consecutive slots (a level's new ones are) are cleared at once
    for (const LevelNode& nd : h) {
        total += nd.cnt;
        any_sub |= nd.slot2 >= 0;
        if (nd.slot != run1) {
            if (run1 > run0) OTTO_HIP(hipMemsetAsync(hist0 + (int64_t)run0 * words, 0, (size_t)(run1 - run0) * words * 8, s));
            run0 = nd.slot;
        }
        run1 = nd.slot + 1;
    }
    if (run1 > run0) OTTO_HIP(hipMemsetAsync(hist0 + (int64_t)run0 * words, 0, (size_t)(run1 - run0) * words * 8, s));
    const int64_t chunk = level_chunk(total);
    int64_t items = 0;
    OTTO_TRY(upload_nodes(h, chunk, d_nodes, &items, s));
    if (items) {
        const dim3 grid((unsigned)items, (unsigned)(((feats ? n_list : F) + HIST_FG - 1) / HIST_FG));
        if (feats)
            k_level_hist<true><<<grid, HIST_THREADS, 0, s>>>(bins, n, F, (const int2*)gh, rows, d_nodes, (int)h.size(), chunk,
                                                             (unsigned long long*)hist0, words, err, feats, n_list);
        else
            k_level_hist<false><<<grid, HIST_THREADS, 0, s>>>(bins, n, F, (const int2*)gh, rows, d_nodes, (int)h.size(), chunk,
                                                              (unsigned long long*)hist0, words, err, nullptr, 0);
        OTTO_HIP(hipGetLastError());
    }
    if (any_sub) {
        k_level_sub<<<dim3((unsigned)((words + 255) / 256), (unsigned)h.size()), 256, 0, s>>>(d_nodes, hist0, words);
        OTTO_HIP(hipGetLastError());
    }
    return 0;
}

int launch_level_split(std::vector<LevelNode>& h, LevelNode* d_nodes, const int64_t* hist0, int F, const int32_t* n_edges,
                       const int32_t* exps, const SplitParams& p, const int32_t* feats, int n_list, int64_t* d_split, hipStream_t s) {
    const int64_t words = (int64_t)3 * F * 256;
    int64_t items = 0;
    OTTO_TRY(upload_nodes(h, 0, d_nodes, &items, s));
    if (feats) k_level_split<true><<<(unsigned)h.size(), 256, 0, s>>>(d_nodes, hist0, words, F, n_edges, exps, p, feats, n_list, d_split);
    else k_level_split<false><<<(unsigned)h.size(), 256, 0, s>>>(d_nodes, hist0, words, F, n_edges, exps, p, nullptr, 0, d_split);
    OTTO_HIP(hipGetLastError());
    return 0;
}

int launch_level_partition(const uint8_t* bins, int64_t n, const int32_t* rows, std::vector<LevelNode>& h, LevelNode* d_nodes,
                           int32_t* out, uint32_t* block_left, int64_t* n_left, uint32_t* err, hipStream_t s) {
    int64_t items = 0;
    OTTO_TRY(upload_nodes(h, PART_ROWS, d_nodes, &items, s));
    if (items) {
        k_level_part_count<<<(unsigned)items, 256, 0, s>>>(bins, n, rows, d_nodes, (int)h.size(), block_left, err);
        OTTO_HIP(hipGetLastError());
    }
    k_level_part_scan<<<(unsigned)h.size(), 256, 0, s>>>(d_nodes, block_left, n_left);
    OTTO_HIP(hipGetLastError());
    if (items) {
        k_level_part_scatter<<<(unsigned)items, 256, 0, s>>>(bins, n, rows, d_nodes, (int)h.size(), block_left, n_left, out);
        OTTO_HIP(hipGetLastError());
    }
    return 0;
}

// the descriptors of a level entry point: ranges inside [0, n_rows) that do not overlap, slots inside [0, n_slots)
int read_nodes(const int32_t* h_nodes, int32_t n_nodes, int64_t n_rows, int32_t n_slots, int32_t F, bool need_split,
               std::vector<LevelNode>* out) {
    OTTO_REQUIRE(h_nodes && n_nodes >= 1 && n_nodes <= MAX_LEVEL_NODES, "n_nodes = %d outside [1, %d]", n_nodes, MAX_LEVEL_NODES);
    out->resize(n_nodes);
    memcpy(out->data(), h_nodes, (size_t)n_nodes * sizeof(LevelNode));
    int64_t prev_end = 0;
    for (int i = 0; i < n_nodes; ++i) {
        const LevelNode& nd = (*out)[i];
        OTTO_REQUIRE(nd.begin >= prev_end && nd.cnt >= 0 && (int64_t)nd.begin + nd.cnt <= n_rows,
                     "node %d: rows [%d, %d + %d) must lie inside [0, %lld) behind the node before", i, nd.begin, nd.begin, nd.cnt,
                     (long long)n_rows);
        prev_end = (int64_t)nd.begin + nd.cnt;
        OTTO_REQUIRE(n_slots == 0 || (nd.slot >= 0 && nd.slot < n_slots && nd.slot2 < n_slots && nd.slot2 != nd.slot),
                     "node %d: slots %d, %d outside [0, %d)", i, nd.slot, nd.slot2, n_slots);
        OTTO_REQUIRE(!need_split || (nd.feature >= 0 && nd.feature < F && nd.bin >= 0 && nd.bin < OTTO_GBDT_MAX_EDGES),
                     "node %d: feature %d, bin %d", i, nd.feature, nd.bin);
    }
    return 0;
}

int check_xgb_params(double min_child_weight, double lambda, double gamma) {
    OTTO_REQUIRE(gamma >= 0.0, "gamma = %g below 0", gamma);
    return check_split_params(0, min_child_weight, lambda, gamma);
}

}  // namespace
}  // namespace otto

using namespace otto;

template <bool NDCG>
static int launch_pairs(const PairArgs& a, int64_t Q, hipStream_t s) {
    // OTTO's queries hold 50 to 100 candidates: one wave each; the second launch finds nothing to do there
    k_xgb_pairwise_short<NDCG><<<(unsigned)Q, 64, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    if (a.n > SHORT_QUERY) {
        const int64_t blocks = Q < LONG_BLOCKS ? Q : LONG_BLOCKS;
        k_xgb_pairwise_long<NDCG><<<(unsigned)blocks, 256, 0, s>>>(a, Q, (Q + blocks - 1) / blocks);
        OTTO_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int otto_xgb_lambdamart(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                                   const double* d_sigmoid, double sigmoid_lo, double sigmoid_factor, uint64_t seed_it, int32_t weighting,
                                   const double* d_discount, double* d_grad, double* d_hess, void* stream) {
    OTTO_TRY(check_query_args(d_score, d_label, d_query_off, Q, n));
    OTTO_REQUIRE(sigmoid_factor > 0.0 && sigmoid_lo == sigmoid_lo, "sigmoid_lo = %g, sigmoid_factor = %g", sigmoid_lo, sigmoid_factor);
    OTTO_REQUIRE(weighting == 0 || weighting == 1, "weighting = %d: 0 (rank:pairwise) or 1 (rank:ndcg)", weighting);
    OTTO_REQUIRE((d_grad && d_hess) || n == 0, "null d_grad or d_hess");
    hipStream_t s = (hipStream_t)stream;
    if (n) {
        OTTO_HIP(hipMemsetAsync(d_grad, 0, (size_t)n * 8, s));
        OTTO_HIP(hipMemsetAsync(d_hess, 0, (size_t)n * 8, s));
    }
    if (Q == 0) return 0;
    OTTO_REQUIRE(d_sigmoid, "null d_sigmoid");
    OTTO_REQUIRE(weighting == 0 || d_discount, "null d_discount");
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    PairArgs a{d_score, d_label, d_query_off, n, d_sigmoid, sigmoid_lo, sigmoid_factor, seed_it, d_discount, d_grad, d_hess, err};
    if (weighting) OTTO_TRY(launch_pairs<true>(a, Q, s));
    else OTTO_TRY(launch_pairs<false>(a, Q, s));
    return err_end(err, s);
}

extern "C" int64_t otto_xgb_workspace_bytes(int64_t n, int32_t F, int32_t max_depth) {
    if (n < 0 || n >= ((int64_t)1 << 31) || F < 1 || F > OTTO_FOREST_MAX_FEATURES || max_depth < 1 || max_depth > OTTO_XGB_MAX_DEPTH)
        return 0;
    return work_layout(n, F, max_depth).total;
}

extern "C" int otto_xgb_level_hist(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_rows,
                                   int64_t n_rows, const int32_t* h_nodes, int32_t n_nodes, const int32_t* d_features, int32_t n_used,
                                   int64_t* d_hist, int32_t n_slots, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows = %lld outside [0, 2^31)", (long long)n_rows);
    OTTO_REQUIRE(d_hist && n_slots >= 1, "null d_hist or n_slots = %d", n_slots);
    OTTO_REQUIRE((d_gh && d_rows) || n_rows == 0, "null d_gh or d_rows");
    const LevelWork w = level_work(n_rows);
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, a level launch needs %lld", (long long)work_bytes,
                 (long long)w.bytes);
    std::vector<LevelNode> h;
    OTTO_TRY(read_nodes(h_nodes, n_nodes, n_rows, n_slots, F, false, &h));
    hipStream_t s = (hipStream_t)stream;
    if (d_features) OTTO_TRY(check_feature_list(d_features, n_used, F, s));
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_TRY(launch_level_hist(d_bins, n, F, d_gh, d_rows, h, (LevelNode*)((char*)d_work + w.nodes), d_hist, err, d_features, n_used, s));
    return err_end(err, s);
}

extern "C" int otto_xgb_level_split(const int64_t* d_hist, int32_t n_slots, int32_t F, const int32_t* d_n_edges, const int32_t* d_exp,
                                    const int32_t* h_nodes, int32_t n_nodes, double min_child_weight, double lambda, double gamma,
                                    const int32_t* d_features, int32_t n_used, int64_t* d_split, void* d_work, int64_t work_bytes,
                                    void* stream) {
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    OTTO_REQUIRE(d_hist && d_n_edges && d_exp && d_split && n_slots >= 1, "null argument or n_slots = %d", n_slots);
    OTTO_TRY(check_xgb_params(min_child_weight, lambda, gamma));
    const LevelWork w = level_work(0);
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, a level launch needs %lld", (long long)work_bytes,
                 (long long)w.bytes);
    std::vector<LevelNode> h;
    OTTO_TRY(read_nodes(h_nodes, n_nodes, ((int64_t)1 << 31) - 1, n_slots, F, false, &h));
    hipStream_t s = (hipStream_t)stream;
    if (d_features) OTTO_TRY(check_feature_list(d_features, n_used, F, s));
    SplitParams p{0, min_child_weight, lambda, gamma};
    OTTO_TRY(launch_level_split(h, (LevelNode*)((char*)d_work + w.nodes), d_hist, F, d_n_edges, d_exp, p, d_features, n_used, d_split, s));
    OTTO_HIP(hipStreamSynchronize(s));               // the descriptors are the call's own: the copy must have read them
    return 0;
}

extern "C" int otto_xgb_level_partition(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_rows, int64_t n_rows,
                                        const int32_t* h_nodes, int32_t n_nodes, int32_t* d_out, int64_t* d_n_left, void* d_work,
                                        int64_t work_bytes, void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows = %lld outside [0, 2^31)", (long long)n_rows);
    OTTO_REQUIRE(d_n_left && ((d_rows && d_out) || n_rows == 0), "null argument");
    const LevelWork w = level_work(n_rows);
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, a level launch needs %lld", (long long)work_bytes,
                 (long long)w.bytes);
    std::vector<LevelNode> h;
    OTTO_TRY(read_nodes(h_nodes, n_nodes, n_rows, 0, F, true, &h));
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_work;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_TRY(launch_level_partition(d_bins, n, d_rows, h, (LevelNode*)(base + w.nodes), d_out, (uint32_t*)(base + w.block_left),
                                    (int64_t*)(base + w.n_left), err, s));
    OTTO_HIP(hipMemcpyAsync(d_n_left, base + w.n_left, (size_t)n_nodes * 8, hipMemcpyDeviceToDevice, s));
    return err_end(err, s);
}

extern "C" int otto_xgb_grow_tree(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_exp,
                                  const int32_t* d_n_edges, const float* h_edges, int32_t max_depth, double min_child_weight,
                                  double lambda, double gamma, double eta, const int32_t* d_bag, int64_t n_bag,
                                  const int32_t* d_features, int32_t n_used, otto_xgb_tree* tree, void* d_work, int64_t work_bytes,
                                  void* stream) {
    OTTO_TRY(check_bins_args(d_bins, n, F));
    OTTO_REQUIRE(!d_bag || (n_bag >= 1 && n_bag <= n), "n_bag = %lld outside [1, n = %lld]", (long long)n_bag, (long long)n);
    OTTO_REQUIRE(n >= 1, "n = 0: nothing to grow a tree on");
    OTTO_REQUIRE(max_depth >= 1 && max_depth <= OTTO_XGB_MAX_DEPTH, "max_depth = %d outside [1, %d]", max_depth, OTTO_XGB_MAX_DEPTH);
    OTTO_TRY(check_xgb_params(min_child_weight, lambda, gamma));
    OTTO_REQUIRE(eta == eta, "eta is NaN");
    OTTO_REQUIRE(d_gh && d_exp && d_n_edges && h_edges && tree, "null argument");
    otto_xgb_tree& T = *tree;
    OTTO_REQUIRE(T.split_feature && T.split_bin && T.threshold && T.decision_type && T.left_child && T.right_child && T.split_gain &&
                 T.cover && T.sum_grad && T.count && T.left_id && T.right_id && T.leaf_value && T.leaf_cover && T.leaf_sum_grad &&
                 T.leaf_count, "null array in otto_xgb_tree");
    const WorkLayout w = work_layout(n, F, max_depth);
    OTTO_REQUIRE(d_work && work_bytes >= w.total, "d_work holds %lld bytes, otto_xgb_workspace_bytes asks for %lld",
                 (long long)work_bytes, (long long)w.total);
    hipStream_t s = (hipStream_t)stream;
    int n_syncs = 0;
    T.n_leaves = 0; T.n_syncs = 0; T.hist_rows = 0;
    if (d_features) {
        OTTO_TRY(check_feature_list(d_features, n_used, F, s));
        ++n_syncs;
    }
    char* base = (char*)d_work;
    const LevelWork lw = level_work(n);
    LevelNode* d_nodes = (LevelNode*)(base + w.level + lw.nodes);      // three regions: split, partition, hist
    uint32_t* block_left = (uint32_t*)(base + w.level + lw.block_left);
    int64_t* d_n_left = (int64_t*)(base + w.level + lw.n_left);
    int32_t* rows[2] = {(int32_t*)(base + w.rows_a), (int32_t*)(base + w.rows_b)};
    int64_t* d_split = (int64_t*)(base + w.split);
    int64_t* hist0 = (int64_t*)(base + w.hist);
    SplitParams p{0, min_child_weight, lambda, gamma};
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    int32_t exps[2] = {0, 0};
    OTTO_HIP(hipMemcpyAsync(exps, d_exp, 8, hipMemcpyDeviceToHost, s));     // on the host after the first synchronisation

    struct Live {           // a live leaf of the level
        int leaf, xid;      // SPEC-GBDT's leaf index, XGBoost's node id
        int64_t begin, cnt;
        int slot;
        int parent, side;   // the internal node that points here (-1: the root), 0 left / 1 right
    };
    struct LeafSums { int64_t gq, hq, cnt; };
    const int64_t n_root = d_bag ? n_bag : n;
    // the root's row list: the bag, or every row
    if (d_bag) OTTO_HIP(hipMemcpyAsync(rows[0], d_bag, (size_t)n_bag * 4, hipMemcpyDeviceToDevice, s));
    else {
        k_iota<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(rows[0], n);
        OTTO_HIP(hipGetLastError());
    }
    std::vector<std::vector<LevelNode>> keep;   // every uploaded descriptor list stays alive until the call returns
    keep.reserve((size_t)3 * max_depth + 2);
    keep.emplace_back(1, LevelNode{0, (int32_t)n_root, 0, -1, 0, 0, 0, 0});
    OTTO_TRY(launch_level_hist(d_bins, n, F, d_gh, rows[0], keep.back(), d_nodes + 2 * MAX_LEVEL_NODES, hist0, err, d_features, n_used, s));
    int64_t hist_rows = n_root;
    std::vector<Live> level(1, Live{0, 0, 0, n_root, 0, -1, 0});
    std::vector<LeafSums> leaves(1, LeafSums{0, 0, n_root});
    std::vector<int64_t> rec((size_t)MAX_LEVEL_NODES * SW);
    int n_internal = 0, n_xgb = 1, next_slot = 1;
    for (int depth = 0; depth < max_depth && !level.empty(); ++depth) {
        const int n_live = (int)level.size();
        keep.emplace_back((size_t)n_live);
        for (int i = 0; i < n_live; ++i) keep.back()[i] = LevelNode{(int32_t)level[i].begin, (int32_t)level[i].cnt, level[i].slot, -1, 0, 0, 0, 0};
        OTTO_TRY(launch_level_split(keep.back(), d_nodes, hist0, F, d_n_edges, d_exp, p, d_features, n_used, d_split, s));
        uint32_t bad[ERR_WORDS] = {0, 0, 0, 0, 0};
        OTTO_HIP(hipMemcpyAsync(rec.data(), d_split, (size_t)n_live * SW * 8, hipMemcpyDeviceToHost, s));
        OTTO_HIP(hipMemcpyAsync(bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
        OTTO_HIP(hipStreamSynchronize(s));          // the one synchronisation of the level
        ++n_syncs;
        // a bag is the caller's: an entry outside [0, n) is reported here, before the counts it spoils are compared
        OTTO_TRY(err_code(bad));
        std::vector<Live> next;
        std::vector<LevelNode> part, hist;
        const bool children_split = depth + 1 < max_depth;      // the children of this level are searched in turn
        for (int i = 0; i < n_live; ++i) {
            const Live P = level[i];
            const int64_t* r = rec.data() + (int64_t)i * SW;
            OTTO_REQUIRE(r[8] == P.cnt, "the histogram of node %d counts %lld rows, its row range holds %lld", P.xid, (long long)r[8],
                         (long long)P.cnt);
            if (depth == 0) { leaves[0].gq = r[9]; leaves[0].hq = r[10]; }
            else OTTO_REQUIRE(r[9] == leaves[P.leaf].gq && r[10] == leaves[P.leaf].hq,
                              "the histogram of node %d disagrees with the split that made it", P.xid);
            if (!r[0]) continue;
            const int f = (int)r[1], b = (int)r[2], dl = (int)r[3];
            OTTO_REQUIRE(f >= 0 && f < F && b >= 0 && b < OTTO_GBDT_MAX_EDGES && r[5] >= 0 && r[5] <= P.cnt,
                         "the split search returned feature %d, bin %d, %lld of %lld rows left", f, b, (long long)r[5], (long long)P.cnt);
            const int node = n_internal++, right = (int)leaves.size();
            T.split_feature[node] = f;
            T.split_bin[node] = b;
            T.threshold[node] = (double)h_edges[(int64_t)f * OTTO_GBDT_MAX_EDGES + b];
            T.decision_type[node] = (int8_t)((2 << 2) | (dl ? 2 : 0));
            memcpy(&T.split_gain[node], &r[4], 8);
            T.cover[node] = ldexp((double)r[10], -exps[1]);
            T.sum_grad[node] = ldexp((double)r[9], -exps[0]);
            T.count[node] = r[8];
            T.left_child[node] = ~P.leaf;
            T.right_child[node] = ~right;
            T.left_id[node] = n_xgb;
            T.right_id[node] = n_xgb + 1;
            if (P.parent >= 0) (P.side ? T.right_child : T.left_child)[P.parent] = node;
            const int64_t cL = r[5], cR = P.cnt - cL;
            leaves[P.leaf] = LeafSums{r[6], r[7], cL};
            leaves.push_back(LeafSums{r[9] - r[6], r[10] - r[7], cR});
            if (children_split) {
                // the smaller child's histogram is built (ties: the left one), the larger one is the parent's minus that
                const bool left_small = cL <= cR;
                const int small_slot = next_slot++;
                OTTO_REQUIRE(small_slot < w.slots, "histogram slot %d of %d", small_slot, w.slots);
                next.push_back(Live{P.leaf, n_xgb, P.begin, cL, left_small ? small_slot : P.slot, node, 0});
                next.push_back(Live{right, n_xgb + 1, P.begin + cL, cR, left_small ? P.slot : small_slot, node, 1});
                part.push_back(LevelNode{(int32_t)P.begin, (int32_t)P.cnt, 0, -1, 0, f, b, dl});
                hist.push_back(LevelNode{(int32_t)(left_small ? P.begin : P.begin + cL), (int32_t)(left_small ? cL : cR), small_slot,
                                         P.slot, 0, 0, 0, 0});
                hist_rows += left_small ? cL : cR;
            }
            n_xgb += 2;
        }
        if (next.empty()) break;                    // nothing split, or the children are at max_depth: they stay leaves
        const int32_t* in = rows[depth & 1];
        int32_t* out = rows[(depth + 1) & 1];
        keep.push_back(std::move(part));
        OTTO_TRY(launch_level_partition(d_bins, n, in, keep.back(), d_nodes + MAX_LEVEL_NODES, out, block_left, d_n_left, err, s));
        keep.push_back(std::move(hist));
        OTTO_TRY(launch_level_hist(d_bins, n, F, d_gh, out, keep.back(), d_nodes + 2 * MAX_LEVEL_NODES, hist0, err, d_features, n_used, s));
        level.swap(next);
    }
    // every exit of the loop follows a synchronisation with nothing launched behind it
    for (int i = 0; i < (int)leaves.size(); ++i) {
        const double G = ldexp((double)leaves[i].gq, -exps[0]), H = ldexp((double)leaves[i].hq, -exps[1]);
        T.leaf_value[i] = (double)(float)(-(G / (H + lambda)) * eta);
        T.leaf_cover[i] = H;
        T.leaf_sum_grad[i] = G;
        T.leaf_count[i] = leaves[i].cnt;
    }
    T.n_leaves = (int32_t)leaves.size();
    T.n_syncs = n_syncs;
    T.hist_rows = hist_rows;
    return 0;
}
