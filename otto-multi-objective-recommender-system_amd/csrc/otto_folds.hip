// GroupKFold, the index sets of a fold with negative down-sampling, and the bin gather (SPEC-FOLDS, DESIGN.md section 3h;
// include/otto_folds.h). Integer work only: every output is pinned bit for bit.
//
// Device, on the caller's stream:
//   k_kf_hist      one wave per contiguous chunk of queries: checks the offsets and counts the chunk's queries per size
//                  (1025 bins in LDS) into its row of a [chunks, 1025] table.
//   k_kf_colscan   one thread per size walks the table's column from the last chunk to the first: the entry becomes the
//                  number of equal-sized queries in later chunks (they order first: q descending), the sum the size's total.
//   k_kf_start     start[s] = number of queries larger than s (one workgroup, LDS).
//   k_kf_place     the chunk again, from its last query to its first: rank among the equal-sized queries of the chunk by
//                  ballot, pos(q) = start + column + rank; writes size_at[pos] and pos_of_q[q].
//   k_kf_walk      ONE wave walks the Q positions. The fold totals are wave-uniform registers; the lanes fetch 64 sizes per
//                  coalesced load (the next 64 are in flight during the walk of the current ones) and write pos -> fold
//                  as one byte per lane. Sequential in Q by definition of the greedy assignment.
//   k_kf_scatter   fold_of_query[q] = fold_at[pos_of_q[q]].
//   k_classify     one wave per query (grid-stride): positives of the query by ballot, then the state byte of every row;
//                  N, P, Mv, Qt, Qv as per-wave sums and one integer atomic per wave and counter.
//   device_select  (select.h) radix select of the m-th smallest key among the eligible negatives; NegRows reads the state
//                  bytes, 4 per load.
//   k_query_counts one wave per query: kept rows of the query (validation rows, or positives + negatives with
//                  key <= threshold).
//   device_scan    (scan.h) twice over the queries: (kept queries << 32 | kept rows) of the training and validation side.
//   k_emit         one wave per query: row ids by ballot rank behind the query's scanned base; every write is checked
//                  against the sizes the caller allocated.
//   k_gather_u8    grid = (dwords of a feature row, F): a thread fetches four consecutive idx of one feature and stores one
//                  aligned dword; the bytes in front of the first aligned address and behind the last whole dword are
//                  single byte stores.
#include "common.h"
#include "wave.h"
#include "scan.h"
#include "select.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_forest.h"
#include "../../include/otto_gbdt.h"
#include "../../include/otto_folds.h"

namespace otto {
namespace {

constexpr int MAXQ = OTTO_GBDT_MAX_QUERY;
constexpr int KF_BINS = MAXQ + 1;           // sizes 0 .. 1024
constexpr int KF_CHUNK = 1024;              // queries per chunk until the chunk count reaches KF_MAX_CHUNKS
constexpr int KF_MAX_CHUNKS = 1024;
constexpr int GRID_WAVES_BLOCKS = 2048;     // fixed grid of the wave-per-query kernels (4 waves per workgroup)
constexpr int ST_OUT = OTTO_FOLDS_OUT, ST_VAL = OTTO_FOLDS_VAL, ST_POS = OTTO_FOLDS_POS, ST_NEG = OTTO_FOLDS_NEG;
constexpr int MODE_NONE = 0, MODE_THRESHOLD = 1, MODE_ALL = 2;
// error words of a call
constexpr int ERR_QUERY = 0, ERR_LABEL = 1, ERR_INDEX = 2, ERR_SIZE = 3, ERR_WORDS = 4;
constexpr int COUNT_WORDS = OTTO_FOLDS_COUNT_WORDS;
constexpr int CNT_N = 0, CNT_P = 1, CNT_MV = 2, CNT_QT = 3, CNT_QV = 4;

__device__ __forceinline__ bool query_ok(int64_t a, int64_t b, int64_t n) { return a >= 0 && a <= b && b <= n && b - a <= MAXQ; }

// ---------------------------------------------------------------------------------------------------------------------
// fold assignment
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_kf_hist(const int64_t* off, int64_t Q, int64_t n, int64_t per, uint32_t* table,
                                                uint32_t* err) {
    __shared__ uint32_t cnt[KF_BINS];
    const int lane = threadIdx.x;
    for (int s = lane; s < KF_BINS; s += 64) cnt[s] = 0;
    wave_lds_sync();
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < Q ? lo + per : Q;
    uint32_t bad = 0;
    for (int64_t q = lo + lane; q < hi; q += 64) {
        const int64_t a = off[q], b = off[q + 1];
        if (query_ok(a, b, n)) atomicAdd(&cnt[(int)(b - a)], 1u);
        else ++bad;
    }
    if (bad) atomicAdd(err + ERR_QUERY, bad);
    wave_lds_sync();
    uint32_t* row = table + (int64_t)blockIdx.x * KF_BINS;
    for (int s = lane; s < KF_BINS; s += 64) row[s] = cnt[s];
}

__global__ __launch_bounds__(256) void k_kf_colscan(uint32_t* table, int nb, uint32_t* total, const uint32_t* err) {
    if (err[ERR_QUERY]) return;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= KF_BINS) return;
    uint32_t run = 0;
    for (int b = nb - 1; b >= 0; --b) {
        uint32_t* p = table + (int64_t)b * KF_BINS + s;
        const uint32_t t = *p;
        *p = run;
        run += t;
    }
    total[s] = run;
}

__global__ __launch_bounds__(256) void k_kf_start(const uint32_t* total, uint32_t* start, const uint32_t* err) {
    __shared__ uint32_t sm[KF_BINS];
    if (err[ERR_QUERY]) return;
    for (int s = threadIdx.x; s < KF_BINS; s += 256) sm[s] = total[s];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int s = KF_BINS - 1; s >= 0; --s) {
            const uint32_t t = sm[s];
            sm[s] = run;
            run += t;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < KF_BINS; s += 256) start[s] = sm[s];
}

__global__ __launch_bounds__(64) void k_kf_place(const int64_t* off, int64_t Q, int64_t per, const uint32_t* table,
                                                 const uint32_t* start, uint16_t* size_at, int32_t* pos_of_q, const uint32_t* err) {
    __shared__ uint32_t cnt[KF_BINS];
    if (err[ERR_QUERY]) return;                       // a size outside 0..1024 would index outside the tables
    const int lane = threadIdx.x;
    for (int s = lane; s < KF_BINS; s += 64) cnt[s] = 0;
    wave_lds_sync();
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < Q ? lo + per : Q;
    const uint32_t* col = table + (int64_t)blockIdx.x * KF_BINS;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t top = hi; top > lo; top -= 64) {
        const int64_t q = top - 1 - lane;             // lane 0 holds the largest q: it orders first among equal sizes
        const bool active = q >= lo;
        const int c = active ? (int)(off[q + 1] - off[q]) : -1;
        uint64_t todo = __ballot(active);
        uint32_t rank = 0;
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int v = __shfl(c, leader, 64);
            const uint64_t same = __ballot(active && c == v);
            const uint32_t seen = cnt[v];
            if (active && c == v) rank = seen + (uint32_t)__popcll(same & below);
            wave_lds_sync();
            if (lane == leader) cnt[v] = seen + (uint32_t)__popcll(same);
            wave_lds_sync();
            todo &= ~same;
        }
        if (active) {
            const int64_t pos = (int64_t)start[c] + col[c] + rank;
            if (pos < Q) {                            // holds by construction
                size_at[pos] = (uint16_t)c;
                pos_of_q[q] = (int32_t)pos;
            }
        }
    }
}

template <int NS>
__global__ __launch_bounds__(64) void k_kf_walk(const uint16_t* size_at, int64_t Q, uint8_t* fold_at, int64_t* fold_rows,
                                                const uint32_t* err) {
    if (err[ERR_QUERY]) return;
    const int lane = threadIdx.x;
    uint32_t load[NS];                                // wave-uniform; the totals stay below 2^31 because n does
#pragma unroll
    for (int f = 0; f < NS; ++f) load[f] = 0;
    int cur = lane < Q ? size_at[lane] : 0;
    for (int64_t base = 0; base < Q; base += 64) {
        const int64_t ni = base + 64 + lane;
        const int nxt = ni < Q ? size_at[ni] : 0;
        const int cnt = Q - base < 64 ? (int)(Q - base) : 64;
        int mine = 0;
        for (int j = 0; j < cnt; ++j) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(cur, j);
            uint32_t best = load[0];
            int bf = 0;
#pragma unroll
            for (int f = 1; f < NS; ++f)
                if (load[f] < best) {                 // strict: a tie stays with the lowest fold index
                    best = load[f];
                    bf = f;
                }
#pragma unroll
            for (int f = 0; f < NS; ++f) load[f] += f == bf ? c : 0u;
            mine = lane == j ? bf : mine;
        }
        if (base + lane < Q) fold_at[base + lane] = (uint8_t)mine;
        cur = nxt;
    }
#pragma unroll
    for (int f = 0; f < NS; ++f)
        if (lane == 0) fold_rows[f] = (int64_t)load[f];
}

__global__ __launch_bounds__(256) void k_kf_scatter(const int32_t* pos_of_q, const uint8_t* fold_at, int64_t Q, int32_t* fold_of_query,
                                                    const uint32_t* err) {
    if (err[ERR_QUERY]) return;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
        const int32_t pos = pos_of_q[q];
        if (pos >= 0 && pos < Q) fold_of_query[q] = fold_at[pos];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// index sets
// ---------------------------------------------------------------------------------------------------------------------
template <typename L>
__global__ __launch_bounds__(256) void k_classify(const L* label, const int64_t* off, int64_t Q, int64_t n, const int32_t* fold_of_query,
                                                  int fold, uint8_t* state, unsigned long long* counts, uint32_t* err) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    unsigned long long cN = 0, cP = 0, cV = 0, cQt = 0, cQv = 0;      // wave-uniform
    for (int64_t q = wid; q < Q; q += nw) {
        const int64_t a = off[q], b = off[q + 1];
        if (!query_ok(a, b, n)) {
            if (lane == 0) atomicAdd(err + ERR_QUERY, 1u);
            continue;
        }
        if (fold_of_query[q] == fold) {
            for (int64_t r = a + lane; r < b; r += 64) state[r] = ST_VAL;
            cV += (unsigned long long)(b - a);
            cQv += b > a;
            continue;
        }
        int npos = 0;
        bool bad = false;
        for (int64_t r0 = a; r0 < b; r0 += 64) {
            const int64_t r = r0 + lane;
            const L l = r < b ? label[r] : (L)0;
            bad |= l < 0;
            npos += __popcll(__ballot(l > 0));
        }
        if (__ballot(bad)) {
            if (lane == 0) atomicOr(err + ERR_LABEL, 1u);
            continue;
        }
        if (npos == 0) continue;                                       // the rows stay ST_OUT
        for (int64_t r = a + lane; r < b; r += 64) state[r] = label[r] > 0 ? ST_POS : ST_NEG;
        cP += npos;
        cN += (unsigned long long)(b - a) - npos;
        cQt += 1;
    }
    if (lane == 0) {
        if (cN) atomicAdd(counts + CNT_N, cN);
        if (cP) atomicAdd(counts + CNT_P, cP);
        if (cV) atomicAdd(counts + CNT_MV, cV);
        if (cQt) atomicAdd(counts + CNT_QT, cQt);
        if (cQv) atomicAdd(counts + CNT_QV, cQv);
    }
}

// row source of the select: the eligible negatives; an item is four state bytes, one load
struct NegRows {
    const uint32_t* state4;
    template <typename F>
    __device__ void operator()(int64_t i, F count) const {
        const uint32_t w = state4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (((w >> (8 * k)) & 255u) == (uint32_t)ST_NEG) count(i * 4 + k);
    }
};

__device__ __forceinline__ bool row_kept(uint32_t st, uint64_t seed, int64_t r, int mode, uint64_t threshold) {
    if (st == (uint32_t)ST_VAL || st == (uint32_t)ST_POS) return true;
    if (st != (uint32_t)ST_NEG) return false;
    return mode == MODE_ALL || (mode == MODE_THRESHOLD && row_key(seed, (uint64_t)r) <= threshold);
}

// qcnt[q] = kept rows | validation query << 31
__global__ __launch_bounds__(256) void k_query_counts(const uint8_t* state, const int64_t* off, int64_t Q, int64_t n, uint64_t seed,
                                                      int mode, const uint64_t* sel, uint32_t* qcnt, uint32_t* err) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const uint64_t threshold = mode == MODE_THRESHOLD ? sel[0] : 0ull;
    for (int64_t q = wid; q < Q; q += nw) {
        const int64_t a = off[q], b = off[q + 1];
        uint32_t kept = 0, val = 0;
        if (!query_ok(a, b, n)) {
            if (lane == 0) atomicAdd(err + ERR_QUERY, 1u);
        } else {
            for (int64_t r0 = a; r0 < b; r0 += 64) {
                const int64_t r = r0 + lane;
                const uint32_t st = r < b ? state[r] : (uint32_t)ST_OUT;
                kept += (uint32_t)__popcll(__ballot(row_kept(st, seed, r, mode, threshold)));
                val += (uint32_t)__popcll(__ballot(st == (uint32_t)ST_VAL));
            }
        }
        if (lane == 0) qcnt[q] = kept | (val ? 0x80000000u : 0u);
    }
}

struct TrainPacked {
    const uint32_t* qcnt;
    __device__ uint64_t operator()(int64_t q) const {
        const uint32_t v = qcnt[q];
        return (v >> 31) == 0 && v ? (1ull << 32) + v : 0ull;
    }
};
struct ValPacked {
    const uint32_t* qcnt;
    __device__ uint64_t operator()(int64_t q) const {
        const uint32_t v = qcnt[q];
        return (v >> 31) && (v & 0x7fffffffu) ? (1ull << 32) + (v & 0x7fffffffu) : 0ull;
    }
};

struct EmitSide {
    int32_t* idx;
    int64_t* query_off;
    int32_t* query;
    int64_t M, Qn;
    const uint64_t* scan;    // [Q+1]: kept queries << 32 | kept rows in front of query q
};

__global__ __launch_bounds__(256) void k_emit(const uint8_t* state, const int64_t* off, int64_t Q, uint64_t seed, int mode,
                                              const uint64_t* sel, const uint32_t* qcnt, EmitSide train, EmitSide val, uint32_t* err) {
    if (err[ERR_QUERY]) return;
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
    const uint64_t threshold = mode == MODE_THRESHOLD ? sel[0] : 0ull;
    const uint64_t below = (1ull << lane) - 1ull;
    if (wid == 0 && lane == 0) {
        const uint64_t tt = train.scan[Q], vt = val.scan[Q];
        if ((int64_t)(tt >> 32) != train.Qn || (int64_t)(tt & 0xffffffffull) != train.M || (int64_t)(vt >> 32) != val.Qn ||
            (int64_t)(vt & 0xffffffffull) != val.M)
            atomicOr(err + ERR_SIZE, 1u);
        train.query_off[train.Qn] = train.M;
        val.query_off[val.Qn] = val.M;
    }
    for (int64_t q = wid; q < Q; q += nw) {
        const uint32_t v = qcnt[q];
        const int64_t cnt = v & 0x7fffffffu;
        if (cnt == 0) continue;
        const EmitSide& side = (v >> 31) ? val : train;
        const uint64_t packed = side.scan[q];
        const int64_t j = (int64_t)(packed >> 32), base = (int64_t)(packed & 0xffffffffull);
        if (j >= side.Qn || base + cnt > side.M) {
            if (lane == 0) atomicOr(err + ERR_SIZE, 1u);
            continue;
        }
        if (lane == 0) {
            side.query[j] = (int32_t)q;
            side.query_off[j] = base;
        }
        const int64_t a = off[q], b = off[q + 1];       // checked by k_query_counts (cnt != 0)
        int64_t at = base;
        for (int64_t r0 = a; r0 < b; r0 += 64) {
            const int64_t r = r0 + lane;
            const uint32_t st = r < b ? state[r] : (uint32_t)ST_OUT;
            const bool keep = row_kept(st, seed, r, mode, threshold);
            const uint64_t mask = __ballot(keep);
            const int64_t pos = at + __popcll(mask & below);
            if (keep && pos < base + cnt) side.idx[pos] = (int32_t)r;
            at += __popcll(mask);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_u8(const uint8_t* bins, int64_t n, const int32_t* idx, int64_t m, uint8_t* out,
                                                   uint32_t* err) {
    const uint8_t* src = bins + (int64_t)blockIdx.y * n;
    uint8_t* dst = out + (int64_t)blockIdx.y * m;
    int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3);         // bytes in front of the row's first aligned dword
    if (head > m) head = m;
    const int64_t nd = (m - head + 3) / 4;                             // dwords of the row, a partial last one included
    bool bad = false;
    auto fetch = [&](int64_t i) -> uint32_t {
        const int32_t x = idx[i];
        if (x < 0 || x >= n) {
            bad = true;
            return 0u;
        }
        return src[x];
    };
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < head) dst[threadIdx.x] = (uint8_t)fetch(threadIdx.x);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nd; j += (int64_t)gridDim.x * 256) {
        const int64_t i0 = head + 4 * j;
        if (i0 + 4 <= m) {
            const uint32_t b0 = fetch(i0), b1 = fetch(i0 + 1), b2 = fetch(i0 + 2), b3 = fetch(i0 + 3);
            *reinterpret_cast<uint32_t*>(dst + i0) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        } else {
            for (int64_t i = i0; i < m; ++i) dst[i] = (uint8_t)fetch(i);
        }
    }
    if (bad) atomicOr(err + ERR_INDEX, 1u);
}

// ---------------------------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------------------------
// scratch: error words at 0, the classify counters at 64
int err_begin(uint32_t** err, hipStream_t s) {
    void* scratch = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_FOLDS, 256, &scratch, s));
    *err = (uint32_t*)scratch;
    OTTO_HIP(hipMemsetAsync(scratch, 0, 128, s));
    return 0;
}

int err_code(const uint32_t* bad) {
    if (bad[ERR_QUERY]) {
        set_error("%u quer%s with query_off not in 0 <= query_off[q] <= query_off[q+1] <= n or with more than %d rows: the "
                  "outputs are not written", bad[ERR_QUERY], bad[ERR_QUERY] == 1 ? "y" : "ies", MAXQ);
        return OTTO_EINVAL;
    }
    if (bad[ERR_LABEL]) {
        set_error("a label below 0");
        return OTTO_EINVAL;
    }
    if (bad[ERR_INDEX]) {
        set_error("an index outside [0, n): its byte is written as 0");
        return OTTO_EINVAL;
    }
    if (bad[ERR_SIZE]) {
        set_error("d_state does not give the sizes Mt, Qt, Mv, Qv the caller passed");
        return OTTO_EINVAL;
    }
    return 0;
}

// drains the stream and turns the error words into a return code
int err_end(uint32_t* err, hipStream_t s) {
    uint32_t bad[ERR_WORDS] = {0, 0, 0, 0};
    OTTO_HIP(hipMemcpyAsync(bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    return err_code(bad);
}


struct KfPlan {
    int nb;
    int64_t per;
};
KfPlan kf_plan(int64_t Q) {
    int64_t nb = (Q + KF_CHUNK - 1) / KF_CHUNK;
    if (nb < 1) nb = 1;
    if (nb > KF_MAX_CHUNKS) nb = KF_MAX_CHUNKS;
    return KfPlan{(int)nb, (Q + nb - 1) / nb};
}

struct KfLayout {
    int64_t table, total, start, size_at, fold_at, pos_of_q, bytes;
};
KfLayout kf_layout(int64_t Q) {
    KfLayout w;
    int64_t at = 0;
    w.table = at; at += align256((int64_t)kf_plan(Q).nb * KF_BINS * 4);
    w.total = at; at += align256(KF_BINS * 4);
    w.start = at; at += align256(KF_BINS * 4);
    w.size_at = at; at += align256(Q * 2);
    w.fold_at = at; at += align256(Q);
    w.pos_of_q = at; at += align256(Q * 4);
    w.bytes = at;
    return w;
}

struct EmitLayout {
    int64_t qcnt, tscan, vscan, partial, hist, sel, bytes;
};
EmitLayout emit_layout(int64_t Q) {
    EmitLayout w;
    int64_t at = 0;
    w.qcnt = at; at += align256(Q * 4);
    w.tscan = at; at += align256((Q + 1) * 8);
    w.vscan = at; at += align256((Q + 1) * 8);
    w.partial = at; at += align256((int64_t)scan_partial_bytes(Q));
    w.hist = at; at += SELECT_HIST_BYTES;
    w.sel = at; at += SELECT_SEL_BYTES;
    w.bytes = at;
    return w;
}

template <int NS>
int launch_walk(int32_t n_splits, const uint16_t* size_at, int64_t Q, uint8_t* fold_at, int64_t* fold_rows, const uint32_t* err,
                hipStream_t s) {
    if constexpr (NS > OTTO_FOLDS_MAX_SPLITS) {
        set_error("n_splits = %d", n_splits);
        return OTTO_EINVAL;
    } else {
        if (n_splits != NS) return launch_walk<NS + 1>(n_splits, size_at, Q, fold_at, fold_rows, err, s);
        k_kf_walk<NS><<<1, 64, 0, s>>>(size_at, Q, fold_at, fold_rows, err);
        OTTO_HIP(hipGetLastError());
        return 0;
    }
}

bool range_ok(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_folds_kfold_workspace(int64_t Q) {
    if (!range_ok(Q)) return 0;
    return kf_layout(Q).bytes;
}

extern "C" int otto_folds_group_kfold(const int64_t* d_query_off, int64_t Q, int64_t n, int32_t n_splits, int32_t* d_fold_of_query,
                                      int64_t* d_fold_rows, float* h_walk_ms, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(range_ok(n), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(range_ok(Q), "Q = %lld outside [0, 2^31)", (long long)Q);
    OTTO_REQUIRE(n_splits >= 2 && n_splits <= OTTO_FOLDS_MAX_SPLITS, "n_splits must be in [2, %d] (got %d)", OTTO_FOLDS_MAX_SPLITS,
                 n_splits);
    OTTO_REQUIRE(Q >= n_splits, "Q = %lld queries for %d folds", (long long)Q, n_splits);
    OTTO_REQUIRE(d_query_off && d_fold_of_query && d_fold_rows, "null argument");
    const KfLayout w = kf_layout(Q);
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, the fold assignment needs %lld", (long long)work_bytes,
                 (long long)w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_work;
    uint32_t* table = (uint32_t*)(base + w.table);
    uint32_t* total = (uint32_t*)(base + w.total);
    uint32_t* start = (uint32_t*)(base + w.start);
    uint16_t* size_at = (uint16_t*)(base + w.size_at);
    uint8_t* fold_at = (uint8_t*)(base + w.fold_at);
    int32_t* pos_of_q = (int32_t*)(base + w.pos_of_q);
    const KfPlan plan = kf_plan(Q);
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    OTTO_HIP(hipMemsetAsync(pos_of_q, 0xff, (size_t)Q * 4, s));
    k_kf_hist<<<plan.nb, 64, 0, s>>>(d_query_off, Q, n, plan.per, table, err);
    OTTO_HIP(hipGetLastError());
    k_kf_colscan<<<(KF_BINS + 255) / 256, 256, 0, s>>>(table, plan.nb, total, err);
    OTTO_HIP(hipGetLastError());
    k_kf_start<<<1, 256, 0, s>>>(total, start, err);
    OTTO_HIP(hipGetLastError());
    k_kf_place<<<plan.nb, 64, 0, s>>>(d_query_off, Q, plan.per, table, start, size_at, pos_of_q, err);
    OTTO_HIP(hipGetLastError());
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (h_walk_ms) {
        OTTO_HIP(hipEventCreate(&ev[0]));
        OTTO_HIP(hipEventCreate(&ev[1]));
        OTTO_HIP(hipEventRecord(ev[0], s));
    }
    int rc = launch_walk<2>(n_splits, size_at, Q, fold_at, d_fold_rows, err, s);
    if (rc == 0 && h_walk_ms && hipEventRecord(ev[1], s) != hipSuccess) {
        set_error("hipEventRecord failed");
        rc = OTTO_EHIP;
    }
    if (rc == 0) {
        const unsigned grid = (unsigned)((Q + 255) / 256 < 2048 ? (Q + 255) / 256 : 2048);
        k_kf_scatter<<<grid, 256, 0, s>>>(pos_of_q, fold_at, Q, d_fold_of_query, err);
        if (hipGetLastError() != hipSuccess) {
            set_error("k_kf_scatter launch failed");
            rc = OTTO_EHIP;
        }
    }
    if (rc == 0) rc = err_end(err, s);
    if (h_walk_ms) {
        *h_walk_ms = 0.f;
        if (rc == 0 && hipEventElapsedTime(h_walk_ms, ev[0], ev[1]) != hipSuccess) {
            set_error("hipEventElapsedTime failed");
            rc = OTTO_EHIP;
        }
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    return rc;
}

extern "C" int64_t otto_folds_state_bytes(int64_t n) {
    if (!range_ok(n)) return 0;
    return (n + 15) / 16 * 16 + 16;
}

extern "C" int otto_folds_classify(const void* d_label, int32_t label_bytes, const int64_t* d_query_off, int64_t Q, int64_t n,
                                   const int32_t* d_fold_of_query, int32_t fold, uint8_t* d_state, int64_t* h_counts, void* stream) {
    OTTO_REQUIRE(range_ok(n), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(range_ok(Q), "Q = %lld outside [0, 2^31)", (long long)Q);
    OTTO_REQUIRE(label_bytes == 1 || label_bytes == 4, "label_bytes must be 1 (uint8) or 4 (int32), got %d", label_bytes);
    OTTO_REQUIRE(fold >= 0 && fold < OTTO_FOLDS_MAX_SPLITS, "fold = %d outside [0, %d)", fold, OTTO_FOLDS_MAX_SPLITS);
    OTTO_REQUIRE(d_query_off && d_state && h_counts, "null argument");
    OTTO_REQUIRE((d_label || n == 0) && (d_fold_of_query || Q == 0), "null d_label or d_fold_of_query");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    unsigned long long* counts = (unsigned long long*)((char*)err + 64);
    OTTO_HIP(hipMemsetAsync(d_state, ST_OUT, (size_t)otto_folds_state_bytes(n), s));
    if (Q) {
        const unsigned grid = (unsigned)((Q + 3) / 4 < GRID_WAVES_BLOCKS ? (Q + 3) / 4 : GRID_WAVES_BLOCKS);
        if (label_bytes == 1)
            k_classify<uint8_t><<<grid, 256, 0, s>>>((const uint8_t*)d_label, d_query_off, Q, n, d_fold_of_query, fold, d_state, counts, err);
        else
            k_classify<int32_t><<<grid, 256, 0, s>>>((const int32_t*)d_label, d_query_off, Q, n, d_fold_of_query, fold, d_state, counts, err);
        OTTO_HIP(hipGetLastError());
    }
    unsigned long long got[COUNT_WORDS] = {0, 0, 0, 0, 0};
    OTTO_HIP(hipMemcpyAsync(got, counts, sizeof(got), hipMemcpyDeviceToHost, s));
    OTTO_TRY(err_end(err, s));
    for (int i = 0; i < COUNT_WORDS; ++i) h_counts[i] = (int64_t)got[i];
    return 0;
}

extern "C" int64_t otto_folds_emit_workspace(int64_t Q) {
    if (!range_ok(Q)) return 0;
    return emit_layout(Q).bytes;
}

extern "C" int otto_folds_emit(const uint8_t* d_state, const int64_t* d_query_off, int64_t Q, int64_t n, int64_t n_eligible, int64_t m,
                               uint64_t seed, int64_t Mt, int64_t Qt, int64_t Mv, int64_t Qv, int32_t* d_train_idx,
                               int64_t* d_train_query_off, int32_t* d_train_query, int32_t* d_val_idx, int64_t* d_val_query_off,
                               int32_t* d_val_query, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(range_ok(n), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(range_ok(Q), "Q = %lld outside [0, 2^31)", (long long)Q);
    OTTO_REQUIRE(n_eligible >= 0 && n_eligible <= n && m >= 0 && m <= n_eligible, "m = %lld of %lld eligible negatives of %lld rows",
                 (long long)m, (long long)n_eligible, (long long)n);
    OTTO_REQUIRE(Mt >= m && Mt <= n && Mv >= 0 && Mv <= n && Qt >= 0 && Qt <= Q && Qv >= 0 && Qv <= Q,
                 "Mt = %lld, Qt = %lld, Mv = %lld, Qv = %lld do not fit n = %lld, Q = %lld, m = %lld", (long long)Mt, (long long)Qt,
                 (long long)Mv, (long long)Qv, (long long)n, (long long)Q, (long long)m);
    OTTO_REQUIRE(d_state && d_query_off && d_train_query_off && d_val_query_off, "null argument");
    OTTO_REQUIRE((d_train_idx || Mt == 0) && (d_train_query || Qt == 0) && (d_val_idx || Mv == 0) && (d_val_query || Qv == 0),
                 "null output");
    const EmitLayout w = emit_layout(Q);
    OTTO_REQUIRE(d_work && work_bytes >= w.bytes, "d_work holds %lld bytes, the index sets need %lld", (long long)work_bytes,
                 (long long)w.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)d_work;
    uint32_t* qcnt = (uint32_t*)(base + w.qcnt);
    uint64_t* tscan = (uint64_t*)(base + w.tscan);
    uint64_t* vscan = (uint64_t*)(base + w.vscan);
    uint64_t* partial = (uint64_t*)(base + w.partial);
    uint32_t* hist = (uint32_t*)(base + w.hist);
    uint64_t* sel = (uint64_t*)(base + w.sel);
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    const int mode = m == 0 ? MODE_NONE : m == n_eligible ? MODE_ALL : MODE_THRESHOLD;
    if (mode == MODE_THRESHOLD)     // d_state is padded with ST_OUT to whole dwords (otto_folds_state_bytes)
        OTTO_TRY(device_select(NegRows{(const uint32_t*)d_state}, (n + 3) / 4, m, seed, hist, sel, s));
    const unsigned qgrid = (unsigned)(Q == 0 ? 1 : (Q + 3) / 4 < GRID_WAVES_BLOCKS ? (Q + 3) / 4 : GRID_WAVES_BLOCKS);
    k_query_counts<<<qgrid, 256, 0, s>>>(d_state, d_query_off, Q, n, seed, mode, sel, qcnt, err);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(TrainPacked{qcnt}, Q, tscan, partial, s));
    OTTO_TRY(device_scan(ValPacked{qcnt}, Q, vscan, partial, s));
    EmitSide train{d_train_idx, d_train_query_off, d_train_query, Mt, Qt, tscan};
    EmitSide val{d_val_idx, d_val_query_off, d_val_query, Mv, Qv, vscan};
    k_emit<<<qgrid, 256, 0, s>>>(d_state, d_query_off, Q, seed, mode, sel, qcnt, train, val, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}

extern "C" int otto_folds_gather_u8(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_idx, int64_t m, uint8_t* d_out,
                                    void* stream) {
    OTTO_REQUIRE(range_ok(n), "n = %lld outside [0, 2^31)", (long long)n);
    OTTO_REQUIRE(range_ok(m), "m = %lld outside [0, 2^31)", (long long)m);
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FOREST_MAX_FEATURES, "F must be in [1, %d] (got %d)", OTTO_FOREST_MAX_FEATURES, F);
    if (m == 0) return 0;
    OTTO_REQUIRE(d_idx && d_out, "null d_idx or d_out");
    OTTO_REQUIRE(d_bins || n == 0, "null d_bins");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = nullptr;
    OTTO_TRY(err_begin(&err, s));
    const int64_t blocks = (m / 4 + 1 + 255) / 256;
    k_gather_u8<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)F), 256, 0, s>>>(d_bins, n, d_idx, m, d_out, err);
    OTTO_HIP(hipGetLastError());
    return err_end(err, s);
}
