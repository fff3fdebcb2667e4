// Validation split, ground-truth labels and recall@20 hit counts on the device (SPEC-EVAL: include/otto_eval.h,
// DESIGN.md section 3f). gfx950 only.
//
// Split. Sessions are binned by LENGTH, since the tail is never longer than the session:
//   n <= EVAL_SHORT (8)   an 8-lane group per session, eight sessions per wave. This kernel visits every session, checks
//                         its cutoff and appends the longer ones to two task lists (one atomic per wave and list).
//   n <= EVAL_WAVE (64)   one wave per listed session.
//   longer                one 256-thread workgroup per listed session.
// In a group every lane holds one event; "first occurrence of (typ, aid) in the tail" and "number of distinct smaller
// aids of my typ" are two all-pairs loops over the group's lanes (ds_bpermute), which give the distinct-ascending lists
// without a sort. A workgroup stages the cart / order events of the tail as (typ, aid) keys, sorts them with a bitonic
// network of ascending compare-exchanges and emits the keys that differ from their left neighbour. Up to EVAL_LDS_KEYS
// (2048) keys are staged in LDS; more go to the session's own slice of the caller's workspace (one key per event), where
// the same network runs in global memory: a pair whose upper index is past the end is skipped, which equals padding
// with +infinity, so any length is exact.
// The count pass and the emit pass run the same code; the emit pass is told the offsets the scans made in between.
//
// Hits. Padded rows (k <= 64): an 8-lane group per label session, one lane per label, no cross-lane traffic inside the
// loops. CSR rows: one wave per label session, lanes strided over the row, a ballot per label.
#include "common.h"
#include "wave.h"
#include "scan.h"
#include "../../include/otto_covis.h"
#include "../../include/otto_eval.h"

#include <stddef.h>
#include <string.h>

namespace otto {
namespace {

constexpr int EVAL_SHORT = 8;         // sessions of up to 8 events: an 8-lane group
constexpr int EVAL_WAVE = 64;         // up to 64 events: a wave
constexpr int EVAL_THREADS = 256;
constexpr int EVAL_LDS_KEYS = 2048;   // cart / order tail events a workgroup sorts in LDS (16 KiB)
constexpr int EVAL_DENOM_CAP = 20;

struct EvalScratch {                  // 256-byte per-device scratch
    uint32_t bad_typ, bad_cutoff, n_without_click, foreign, unsorted;
    uint32_t n_med, n_long, pad;
    unsigned long long tot[4];
};

struct SplitArgs {
    const int32_t* aid;
    const int32_t* ts;
    const uint8_t* typ;
    const int64_t* sess_off;
    int64_t S;
    const int32_t* cutoff;
    // count pass: per-session counts; emit pass: the scanned offsets
    int32_t* cnt[4];                  // kept, click, cart, order  [S] each
    const int64_t* off[4];
    int32_t* out_aid;
    int32_t* out_ts;
    uint8_t* out_typ;
    int32_t* lab[3];                  // click, cart, order aids
    int32_t* list_med;
    int32_t* list_long;
    uint64_t* gkeys;                  // one key per event: the slice of a session is its own events' range
    EvalScratch* sc;
};

__global__ __launch_bounds__(256) void k_check_typ(const uint8_t* typ, int64_t E, EvalScratch* sc) {
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < E; i += (int64_t)gridDim.x * 256) bad += typ[i] > 2;
    if (bad) atomicAdd(&sc->bad_typ, bad);
}

// one 8-lane group per session; every lane walks the session with stride 8 and keeps its own last click
template <bool CUTOFF>
__global__ __launch_bounds__(256) void k_last_click(const uint8_t* typ, const int64_t* sess_off, int64_t S, uint64_t seed,
                                                    int32_t* out, EvalScratch* sc) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int gl = threadIdx.x & 7;
    const bool valid = s < S;
    int64_t b = 0, n = 0;
    if (valid) { b = sess_off[s]; n = sess_off[s + 1] - b; }
    int64_t last = -1;
    uint32_t bad = 0;
    for (int64_t i = gl; i < n; i += 8) {
        const int t = typ[b + i];
        if (t == 0) last = i;
        bad += t > 2;
    }
    if (bad) atomicAdd(&sc->bad_typ, bad);
    for (int d = 1; d < 8; d <<= 1) {
        const int64_t o = __shfl_xor(last, d, 8);
        last = o > last ? o : last;
    }
    if (!valid || gl) return;
    if (!CUTOFF) { out[s] = (int32_t)last; return; }
    int32_t cut = 0;
    if (n != 2 && last > 0) {
        const uint64_t h = mix64(mix64(seed) ^ ((uint64_t)s * 0xA0761D6478BD642Full));
        cut = (int32_t)(((h >> 32) * (uint64_t)last) >> 32);
    }
    if (n != 2 && last < 0) atomicAdd(&sc->n_without_click, 1u);
    out[s] = cut;
}

// append to a task list: one atomic per wave
__device__ __forceinline__ void list_append(bool want, uint32_t* counter, int32_t* list, int32_t value) {
    const uint64_t m = __ballot(want);
    if (!m) return;
    const unsigned l = lane_id();
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0;
    if ((int)l == leader) base = atomicAdd(counter, (uint32_t)__builtin_popcountll(m));
    base = __shfl(base, leader, 64);
    if (want) list[base + __builtin_popcountll(m & ((1ull << l) - 1ull))] = value;
}

// Session s (n <= G events, valid cutoff) on a G-lane group; `active` is false for a group without work. All 64 lanes of
// the wave must arrive here together.
template <int G, bool EMIT>
__device__ __forceinline__ void split_group(const SplitArgs& A, int64_t s, bool active, int gl) {
    int64_t b = 0;
    int n = 0, cut = 0;
    if (active) {
        b = A.sess_off[s];
        n = (int)(A.sess_off[s + 1] - b);
        cut = A.cutoff[s];
    }
    const bool have = gl < n;
    const int32_t a = have ? A.aid[b + gl] : 0;
    const int t = have ? A.typ[b + gl] : 255;
    const bool in_tail = have && gl > cut;
    const int mine = in_tail && (t == 1 || t == 2) ? t : -1;     // my label list, -1: none
    bool dup = false;
#pragma unroll 8
    for (int j = 0; j < G; ++j) {
        const int32_t aj = __shfl(a, j, G);
        const int tj = __shfl(mine, j, G);
        dup |= j < gl && tj == mine && aj == a;
    }
    const int first = mine >= 0 && !dup ? mine : -2;             // first occurrence of (typ, aid) in the tail
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < G; ++j) {
        const int32_t aj = __shfl(a, j, G);
        const int fj = __shfl(first, j, G);
        rank += fj == mine && aj < a;
    }
    const unsigned shift = lane_id() & ~(unsigned)(G - 1);
    const uint64_t gm = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull) << shift;
    const uint64_t m_click = __ballot(in_tail && t == 0) & gm;
    const uint64_t m_cart = __ballot(first == 1) & gm;
    const uint64_t m_order = __ballot(first == 2) & gm;
    if (!active) return;
    if (!EMIT) {
        if (gl == 0) {
            A.cnt[0][s] = n ? cut + 1 : 0;
            A.cnt[1][s] = m_click ? 1 : 0;
            A.cnt[2][s] = __builtin_popcountll(m_cart);
            A.cnt[3][s] = __builtin_popcountll(m_order);
        }
        return;
    }
    if (have && gl <= cut) {
        const int64_t o = A.off[0][s] + gl;
        A.out_aid[o] = a;
        A.out_ts[o] = A.ts[b + gl];
        A.out_typ[o] = (uint8_t)t;
    }
    if (m_click && (int)(__builtin_ctzll(m_click) - shift) == gl) A.lab[0][A.off[1][s]] = a;
    if (first >= 0) A.lab[first][A.off[first + 1][s] + rank] = a;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_split_short(SplitArgs A) {
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int gl = threadIdx.x & 7;
    const bool valid = s < A.S;
    int64_t n = 0;
    int cut = 0;
    if (valid) {
        n = A.sess_off[s + 1] - A.sess_off[s];
        cut = A.cutoff[s];
    }
    const bool bad = valid && (cut < 0 || (int64_t)cut >= (n > 1 ? n : 1));
    const bool ok = valid && !bad;
    if (bad && gl == 0) {
        atomicAdd(&A.sc->bad_cutoff, 1u);
        if (!EMIT) A.cnt[0][s] = A.cnt[1][s] = A.cnt[2][s] = A.cnt[3][s] = 0;
    }
    list_append(ok && gl == 0 && n > EVAL_SHORT && n <= EVAL_WAVE, &A.sc->n_med, A.list_med, (int32_t)s);
    list_append(ok && gl == 0 && n > EVAL_WAVE, &A.sc->n_long, A.list_long, (int32_t)s);
    split_group<8, EMIT>(A, s, ok && n <= EVAL_SHORT, gl);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_split_wave(SplitArgs A) {
    const uint32_t n_items = A.sc->n_med;
    const uint32_t n_waves = gridDim.x * (256 / 64);
    for (uint32_t it = blockIdx.x * (256 / 64) + (threadIdx.x >> 6); it < n_items; it += n_waves)
        split_group<64, EMIT>(A, A.list_med[it], true, (int)lane_id());
}

// ascending bitonic network over K[0, m); a pair whose upper index is >= m is skipped (the pad is +infinity)
__device__ __forceinline__ void block_bitonic(uint64_t* K, int64_t m) {
    int64_t P = 1;
    int lgP = 0;
    while (P < m) { P <<= 1; ++lgP; }
    for (int lk = 1; lk <= lgP; ++lk) {
        const int64_t k = (int64_t)1 << lk, h = k >> 1;
        for (int64_t i = threadIdx.x; i < (P >> 1); i += EVAL_THREADS) {      // mirror step
            const int64_t q = i & (h - 1), lo = ((i >> (lk - 1)) << lk) + q, hi = lo + (k - 1 - 2 * q);
            if (lo >= m) break;
            if (hi < m) {
                const uint64_t x = K[lo], y = K[hi];
                if (x > y) { K[lo] = y; K[hi] = x; }
            }
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; --lj) {
            const int64_t j = (int64_t)1 << lj;
            for (int64_t i = threadIdx.x; i < (P >> 1); i += EVAL_THREADS) {
                const int64_t lo = ((i >> lj) << (lj + 1)) + (i & (j - 1)), hi = lo + j;
                if (lo >= m) break;
                if (hi < m) {
                    const uint64_t x = K[lo], y = K[hi];
                    if (x > y) { K[lo] = y; K[hi] = x; }
                }
            }
            __syncthreads();
        }
    }
}

struct BlockShared {
    unsigned long long m, click, fill;
    uint32_t n_cart;
    uint32_t scan[EVAL_THREADS / 64 + 1];
};

// stage the cart / order keys of the tail in K, sort, count or emit the distinct ones
template <bool EMIT>
__device__ __forceinline__ void block_labels(const SplitArgs& A, int64_t s, int64_t tail0, int64_t L, int64_t m, uint64_t* K,
                                             BlockShared& sh) {
    for (int64_t i = threadIdx.x; i < L; i += EVAL_THREADS) {
        const int t = A.typ[tail0 + i];
        if (t == 1 || t == 2) {
            const unsigned long long p = atomicAdd(&sh.fill, 1ull);
            K[p] = ((uint64_t)(t - 1) << 32) | (uint32_t)A.aid[tail0 + i];
        }
    }
    __syncthreads();
    block_bitonic(K, m);
    const int64_t n_cart = EMIT ? A.off[2][s + 1] - A.off[2][s] : 0;
    int64_t run = 0;
    uint32_t my_carts = 0;
    for (int64_t base = 0; base < m; base += EVAL_THREADS) {
        const int64_t i = base + threadIdx.x;
        uint64_t key = 0;
        uint32_t f = 0;
        if (i < m) {
            key = K[i];
            f = i == 0 || K[i - 1] != key;
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan<uint32_t, EVAL_THREADS>(f, sh.scan, &tot);
        if (f) {
            const int64_t pos = run + ex;
            const int list = (int)(key >> 32);        // 0 carts, 1 orders; the carts sort first
            if (EMIT) A.lab[1 + list][A.off[2 + list][s] + (list ? pos - n_cart : pos)] = (int32_t)(uint32_t)key;
            else my_carts += list == 0;
        }
        run += tot;
    }
    if (!EMIT) {
        if (my_carts) atomicAdd(&sh.n_cart, my_carts);
        __syncthreads();
        if (threadIdx.x == 0) {
            A.cnt[2][s] = (int32_t)sh.n_cart;
            A.cnt[3][s] = (int32_t)(run - sh.n_cart);
        }
    }
}

template <bool EMIT>
__global__ __launch_bounds__(EVAL_THREADS) void k_split_block(SplitArgs A) {
    __shared__ uint64_t keys[EVAL_LDS_KEYS];
    __shared__ BlockShared sh;
    const uint32_t n_items = A.sc->n_long;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = A.list_long[it];
        const int64_t b = A.sess_off[s], n = A.sess_off[s + 1] - b;
        const int64_t cut = A.cutoff[s];
        const int64_t tail0 = b + cut + 1, L = n - cut - 1;
        __syncthreads();                               // the previous item is done with sh
        if (threadIdx.x == 0) { sh.m = 0; sh.click = ~0ull; sh.fill = 0; sh.n_cart = 0; }
        __syncthreads();
        unsigned long long my_m = 0, my_click = ~0ull;
        for (int64_t i = threadIdx.x; i < L; i += EVAL_THREADS) {
            const int t = A.typ[tail0 + i];
            if (t == 0) my_click = my_click < (unsigned long long)i ? my_click : (unsigned long long)i;
            my_m += t == 1 || t == 2;
        }
        if (my_m) atomicAdd(&sh.m, my_m);
        if (my_click != ~0ull) atomicMin(&sh.click, my_click);
        __syncthreads();
        const int64_t m = (int64_t)sh.m;
        const unsigned long long click = sh.click;
        if (EMIT) {
            for (int64_t i = threadIdx.x; i <= cut; i += EVAL_THREADS) {
                const int64_t o = A.off[0][s] + i;
                A.out_aid[o] = A.aid[b + i];
                A.out_ts[o] = A.ts[b + i];
                A.out_typ[o] = A.typ[b + i];
            }
            if (threadIdx.x == 0 && click != ~0ull) A.lab[0][A.off[1][s]] = A.aid[tail0 + (int64_t)click];
        } else if (threadIdx.x == 0) {
            A.cnt[0][s] = (int32_t)(cut + 1);
            A.cnt[1][s] = click != ~0ull;
        }
        if (m <= EVAL_LDS_KEYS) block_labels<EMIT>(A, s, tail0, L, m, keys, sh);
        else block_labels<EMIT>(A, s, tail0, L, m, A.gkeys + tail0, sh);
    }
}

// the last entry of each of the four offset arrays = its total: into the scratch, so the host reads one block
__global__ void k_split_totals(const int64_t* o0, const int64_t* o1, const int64_t* o2, const int64_t* o3, int64_t S, EvalScratch* sc) {
    const int64_t* o[4] = {o0, o1, o2, o3};
    if (threadIdx.x < 4) sc->tot[threadIdx.x] = (unsigned long long)o[threadIdx.x][S];
}

struct CntAt {
    const int32_t* c;
    __device__ uint64_t operator()(int64_t i) const { return (uint64_t)(uint32_t)c[i]; }
};

struct SplitWs {
    int32_t* cnt[4];
    int32_t* list_med;
    int32_t* list_long;
    uint64_t* partial;
    uint64_t* gkeys;
};
size_t split_ws_layout(int64_t S, int64_t E, char* base, SplitWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    SplitWs t;
    for (int i = 0; i < 4; ++i) t.cnt[i] = (int32_t*)take((size_t)S * 4);
    t.list_med = (int32_t*)take((size_t)S * 4);
    t.list_long = (int32_t*)take((size_t)S * 4);
    t.partial = (uint64_t*)take(scan_partial_bytes(S));
    t.gkeys = (uint64_t*)take((size_t)E * 8);
    if (w) *w = t;
    return o < 256 ? 256 : o;
}

int grid_for(int64_t n, int per_block) {
    int64_t g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : g);
}
int capped_grid(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

int get_scratch(EvalScratch** sc, hipStream_t s) {
    void* p = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_EVAL, 256, &p, s));
    *sc = (EvalScratch*)p;
    OTTO_HIP(hipMemsetAsync(p, 0, sizeof(EvalScratch), s));
    return 0;
}

int read_scratch(EvalScratch* sc, EvalScratch* h, hipStream_t s) {
    OTTO_HIP(hipMemcpyAsync(h, sc, sizeof *h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    return 0;
}

template <bool EMIT>
int launch_split(const SplitArgs& a, hipStream_t s) {
    k_split_short<EMIT><<<grid_for(a.S, 256 / 8), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    // fixed grids that walk the task lists: the list lengths stay on the device
    const int64_t by_wave = (a.S + 3) / 4, by_block = a.S;
    k_split_wave<EMIT><<<(int)(by_wave < 2048 ? by_wave : 2048), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    k_split_block<EMIT><<<(int)(by_block < 1024 ? by_block : 1024), EVAL_THREADS, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    return 0;
}

int last_click_common(bool cutoff, const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, uint64_t seed, int32_t* d_out,
                      int64_t* h_n_without_click, const char* who, hipStream_t s) {
    OTTO_REQUIRE(S >= 0 && S < (1ll << 31), "%s: S must be in [0, 2^31) (got %lld)", who, (long long)S);
    if (h_n_without_click) *h_n_without_click = 0;
    if (S == 0) return 0;
    OTTO_REQUIRE(d_sess_off && d_out, "%s: null argument", who);
    EvalScratch* sc = nullptr;
    OTTO_TRY(get_scratch(&sc, s));
    if (cutoff) k_last_click<true><<<grid_for(S, 256 / 8), 256, 0, s>>>(d_typ, d_sess_off, S, seed, d_out, sc);
    else k_last_click<false><<<grid_for(S, 256 / 8), 256, 0, s>>>(d_typ, d_sess_off, S, seed, d_out, sc);
    OTTO_HIP(hipGetLastError());
    EvalScratch h;
    OTTO_TRY(read_scratch(sc, &h, s));
    if (h.bad_typ) {
        set_error("%s: %u events with a typ outside 0..2", who, h.bad_typ);
        return OTTO_EINVAL;
    }
    if (h_n_without_click) *h_n_without_click = (int64_t)h.n_without_click;
    return 0;
}

// ---------------------------------------------------------------------------
// hits
// ---------------------------------------------------------------------------
struct HitsArgs {
    const int32_t* label_session;
    const int64_t* label_off;
    const int32_t* label_aid;
    int64_t S;
    const int32_t* pred_aid;
    const int32_t* pred_n;
    const int64_t* pred_off;
    int32_t k;
    int64_t P;
    const int32_t* pred_session;
    int32_t cap;
    const uint8_t* mask;
    int32_t* row_of;                  // label session -> prediction row, -1: none (only with pred_session)
    int32_t* hits;
    int32_t* denom;
    EvalScratch* sc;
};

// ids ascending and distinct; every prediction session found among the label sessions
__global__ __launch_bounds__(256) void k_hits_map(HitsArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (A.label_session && i > 0 && i < A.S && A.label_session[i] <= A.label_session[i - 1]) atomicAdd(&A.sc->unsorted, 1u);
    if (!A.pred_session || i >= A.P) return;
    const int32_t v = A.pred_session[i];
    if (i > 0 && v <= A.pred_session[i - 1]) atomicAdd(&A.sc->unsorted, 1u);
    int64_t at = -1;
    if (!A.label_session) {
        at = v >= 0 && v < A.S ? v : -1;
    } else {
        int64_t lo = 0, hi = A.S;                      // first label session >= v
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A.label_session[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        if (lo < A.S && A.label_session[lo] == v) at = lo;
    }
    if (at < 0) atomicAdd(&A.sc->foreign, 1u);
    else A.row_of[at] = (int32_t)i;
}

// the counted part of the prediction row of label session j
__device__ __forceinline__ void row_span(const HitsArgs& A, int64_t j, const int32_t** row, int64_t* len) {
    const int64_t p = A.pred_session ? (int64_t)A.row_of[j] : j;
    *row = A.pred_aid;
    *len = 0;
    if (p < 0) return;
    int64_t n;
    if (A.pred_off) {
        const int64_t o = A.pred_off[p];
        *row = A.pred_aid + o;
        n = A.pred_off[p + 1] - o;
    } else {
        *row = A.pred_aid + p * A.k;
        n = A.k;
        if (A.pred_n) n = A.pred_n[p] < n ? A.pred_n[p] : n;
    }
    if (A.cap > 0 && n > A.cap) n = A.cap;
    *len = n > 0 ? n : 0;
}

// 8-lane group per label session, one lane per label: is it the first of its value, and is it in the row
__global__ __launch_bounds__(256) void k_hits_group(HitsArgs A) {
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int gl = threadIdx.x & 7;
    const bool valid = j < A.S;
    int64_t lb = 0, nl = 0, len = 0;
    const int32_t* row = A.pred_aid;
    if (valid) {
        lb = A.label_off[j];
        nl = A.label_off[j + 1] - lb;
        row_span(A, j, &row, &len);
    }
    int32_t h = 0;
    for (int64_t q = gl; q < nl; q += 8) {
        const int32_t v = A.label_aid[lb + q];
        if (v < 0) continue;
        bool dup = false;
        for (int64_t r = 0; r < q && !dup; ++r) dup = A.label_aid[lb + r] == v;
        if (dup) continue;
        bool in = false;
        for (int64_t r = 0; r < len && !in; ++r) in = row[r] == v;
        h += in;
    }
    for (int d = 1; d < 8; d <<= 1) h += __shfl_xor(h, d, 8);
    if (valid && gl == 0) {
        A.hits[j] = h;
        A.denom[j] = (int32_t)(nl < EVAL_DENOM_CAP ? nl : EVAL_DENOM_CAP);
    }
}

// one wave per label session: per label, the lanes stride over the earlier labels and over the row
__global__ __launch_bounds__(256) void k_hits_wave(HitsArgs A) {
    const int64_t n_waves = (int64_t)gridDim.x * (256 / 64);
    const int l = (int)lane_id();
    for (int64_t j = (int64_t)blockIdx.x * (256 / 64) + (threadIdx.x >> 6); j < A.S; j += n_waves) {
        const int64_t lb = A.label_off[j], nl = A.label_off[j + 1] - lb;
        const int32_t* row;
        int64_t len;
        row_span(A, j, &row, &len);
        int32_t h = 0;
        for (int64_t q = 0; q < nl; ++q) {
            const int32_t v = A.label_aid[lb + q];
            if (v < 0) continue;
            bool dup = false;
            for (int64_t r = l; r < q; r += 64) dup |= A.label_aid[lb + r] == v;
            if (__ballot(dup)) continue;
            bool in = false;
            for (int64_t r0 = 0; r0 < len; r0 += 64) {
                in = r0 + l < len && row[r0 + l] == v;
                if (__ballot(in)) { in = true; break; }
            }
            h += in;
        }
        if (l == 0) {
            A.hits[j] = h;
            A.denom[j] = (int32_t)(nl < EVAL_DENOM_CAP ? nl : EVAL_DENOM_CAP);
        }
    }
}

__global__ __launch_bounds__(256) void k_hits_totals(HitsArgs A) {
    __shared__ unsigned long long sm[4][256 / 64];
    unsigned long long t[4] = {0, 0, 0, 0};
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < A.S; j += (int64_t)gridDim.x * 256) {
        const unsigned long long h = (unsigned long long)A.hits[j], d = (unsigned long long)A.denom[j];
        t[0] += h;
        t[1] += d;
        if (A.mask && A.mask[j]) { t[2] += h; t[3] += d; }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        t[c] = wave_reduce<Sum>(t[c]);
        if (lane_id() == 0) sm[c][threadIdx.x >> 6] = t[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long v = 0;
        for (int w = 0; w < 256 / 64; ++w) v += sm[threadIdx.x][w];
        if (v) atomicAdd(&A.sc->tot[threadIdx.x], v);
    }
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int otto_eval_last_click(const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, int32_t* d_last_click, void* stream) {
    return last_click_common(false, d_typ, d_sess_off, S, 0, d_last_click, nullptr, "otto_eval_last_click", (hipStream_t)stream);
}

extern "C" int otto_eval_cutoffs(const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, uint64_t seed, int32_t* d_cutoff,
                                 int64_t* h_n_without_click, void* stream) {
    return last_click_common(true, d_typ, d_sess_off, S, seed, d_cutoff, h_n_without_click, "otto_eval_cutoffs", (hipStream_t)stream);
}

extern "C" int64_t otto_eval_split_workspace(int64_t S, int64_t n_events) {
    if (S < 0 || n_events < 0) return 256;
    return (int64_t)split_ws_layout(S, n_events, nullptr, nullptr);
}

static int split_args(const char* who, const int32_t* d_aid, const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S,
                      int64_t n_events, const int32_t* d_cutoff, void* d_ws, int64_t ws_bytes, SplitArgs* a, SplitWs* w,
                      hipStream_t s) {
    OTTO_REQUIRE(S > 0 && S < (1ll << 31), "%s: S must be in (0, 2^31) (got %lld)", who, (long long)S);
    OTTO_REQUIRE(n_events >= 0, "%s: n_events = %lld", who, (long long)n_events);
    OTTO_REQUIRE(d_sess_off && d_cutoff && d_ws && (n_events == 0 || (d_aid && d_typ)), "%s: null argument", who);
    OTTO_REQUIRE(((uintptr_t)d_ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    OTTO_REQUIRE(ws_bytes >= otto_eval_split_workspace(S, n_events), "%s: workspace too small (%lld < %lld)", who,
                 (long long)ws_bytes, (long long)otto_eval_split_workspace(S, n_events));
    split_ws_layout(S, n_events, (char*)d_ws, w);
    memset(a, 0, sizeof *a);
    a->aid = d_aid; a->typ = d_typ; a->sess_off = d_sess_off; a->S = S; a->cutoff = d_cutoff;
    a->list_med = w->list_med; a->list_long = w->list_long; a->gkeys = w->gkeys;
    OTTO_TRY(get_scratch(&a->sc, s));
    return 0;
}

extern "C" int otto_eval_split_count(const int32_t* d_aid, const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S,
                                     int64_t n_events, const int32_t* d_cutoff, int64_t* d_out_sess_off, int64_t* d_click_off,
                                     int64_t* d_cart_off, int64_t* d_order_off, int64_t* h_counts, void* d_ws, int64_t ws_bytes,
                                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int64_t* offs[4] = {d_out_sess_off, d_click_off, d_cart_off, d_order_off};
    OTTO_REQUIRE(h_counts && offs[0] && offs[1] && offs[2] && offs[3], "otto_eval_split_count: null argument");
    if (S == 0) {
        for (int i = 0; i < 4; ++i) {
            h_counts[i] = 0;
            OTTO_HIP(hipMemsetAsync(offs[i], 0, 8, s));
        }
        return 0;
    }
    SplitArgs a;
    SplitWs w;
    OTTO_TRY(split_args("otto_eval_split_count", d_aid, d_typ, d_sess_off, S, n_events, d_cutoff, d_ws, ws_bytes, &a, &w, s));
    for (int i = 0; i < 4; ++i) a.cnt[i] = w.cnt[i];
    if (n_events) {
        k_check_typ<<<capped_grid(n_events), 256, 0, s>>>(d_typ, n_events, a.sc);
        OTTO_HIP(hipGetLastError());
    }
    OTTO_TRY(launch_split<false>(a, s));
    for (int i = 0; i < 4; ++i) OTTO_TRY(device_scan(CntAt{w.cnt[i]}, S, (uint64_t*)offs[i], w.partial, s));
    k_split_totals<<<1, 64, 0, s>>>(offs[0], offs[1], offs[2], offs[3], S, a.sc);
    OTTO_HIP(hipGetLastError());
    EvalScratch h;
    OTTO_TRY(read_scratch(a.sc, &h, s));
    if (h.bad_typ) {
        set_error("otto_eval_split_count: %u events with a typ outside 0..2", h.bad_typ);
        return OTTO_EINVAL;
    }
    if (h.bad_cutoff) {
        set_error("otto_eval_split_count: %u sessions with a cutoff outside [0, max(n, 1))", h.bad_cutoff);
        return OTTO_EINVAL;
    }
    for (int i = 0; i < 4; ++i) h_counts[i] = (int64_t)h.tot[i];
    return 0;
}

extern "C" int otto_eval_split(const int32_t* d_aid, const int32_t* d_ts, const uint8_t* d_typ, const int64_t* d_sess_off,
                               int64_t S, int64_t n_events, const int32_t* d_cutoff, const int64_t* d_out_sess_off,
                               const int64_t* d_click_off, const int64_t* d_cart_off, const int64_t* d_order_off,
                               int32_t* d_out_aid, int32_t* d_out_ts, uint8_t* d_out_typ, int32_t* d_click_aid,
                               int32_t* d_cart_aid, int32_t* d_order_aid, void* d_ws, int64_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (S == 0) return 0;
    OTTO_REQUIRE(d_out_sess_off && d_click_off && d_cart_off && d_order_off, "otto_eval_split: null offsets");
    OTTO_REQUIRE(n_events == 0 || d_ts, "otto_eval_split: null argument");
    SplitArgs a;
    SplitWs w;
    OTTO_TRY(split_args("otto_eval_split", d_aid, d_typ, d_sess_off, S, n_events, d_cutoff, d_ws, ws_bytes, &a, &w, s));
    a.ts = d_ts;
    a.off[0] = d_out_sess_off; a.off[1] = d_click_off; a.off[2] = d_cart_off; a.off[3] = d_order_off;
    a.out_aid = d_out_aid; a.out_ts = d_out_ts; a.out_typ = d_out_typ;
    a.lab[0] = d_click_aid; a.lab[1] = d_cart_aid; a.lab[2] = d_order_aid;
    return launch_split<true>(a, s);
}

extern "C" int64_t otto_eval_hits_workspace(int64_t S) {
    return S <= 0 ? 256 : (int64_t)align256((size_t)S * 4);
}

extern "C" int otto_eval_hits(const int32_t* d_label_session, const int64_t* d_label_off, const int32_t* d_label_aid, int64_t S,
                              const int32_t* d_pred_aid, const int32_t* d_pred_n, const int64_t* d_pred_off, int32_t k, int64_t P,
                              const int32_t* d_pred_session, int32_t cap, const uint8_t* d_mask, int32_t* d_hits,
                              int32_t* d_denom, int64_t* h_totals, void* d_ws, int64_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    OTTO_REQUIRE(h_totals, "otto_eval_hits: null h_totals");
    OTTO_REQUIRE(S >= 0 && S < (1ll << 31) && P >= 0 && P < (1ll << 31), "otto_eval_hits: S and P must be in [0, 2^31)");
    OTTO_REQUIRE(d_pred_off || (k >= 1 && k <= 64), "otto_eval_hits: padded rows need 1 <= k <= 64 (got %d)", k);
    OTTO_REQUIRE(d_pred_session || P == S, "otto_eval_hits: without d_pred_session the rows are position-aligned: P (%lld) must equal S (%lld)",
                 (long long)P, (long long)S);
    for (int i = 0; i < 4; ++i) h_totals[i] = 0;
    if (S == 0) {
        OTTO_REQUIRE(P == 0, "otto_eval_hits: %lld prediction sessions are not among the label sessions", (long long)P);
        return 0;
    }
    OTTO_REQUIRE(d_label_off && d_hits && d_denom && d_ws && (P == 0 || d_pred_off || d_pred_aid), "otto_eval_hits: null argument");
    OTTO_REQUIRE(((uintptr_t)d_ws & 255) == 0, "otto_eval_hits: the workspace must be 256-byte aligned");
    OTTO_REQUIRE(ws_bytes >= otto_eval_hits_workspace(S), "otto_eval_hits: workspace too small (%lld < %lld)", (long long)ws_bytes,
                 (long long)otto_eval_hits_workspace(S));
    HitsArgs a;
    memset(&a, 0, sizeof a);
    a.label_session = d_label_session; a.label_off = d_label_off; a.label_aid = d_label_aid; a.S = S;
    a.pred_aid = d_pred_aid; a.pred_n = d_pred_off ? nullptr : d_pred_n; a.pred_off = d_pred_off; a.k = d_pred_off ? 0 : k; a.P = P;
    a.pred_session = d_pred_session; a.cap = cap; a.mask = d_mask;
    a.row_of = (int32_t*)d_ws; a.hits = d_hits; a.denom = d_denom;
    OTTO_TRY(get_scratch(&a.sc, s));
    if (d_pred_session) OTTO_HIP(hipMemsetAsync(a.row_of, 0xFF, (size_t)S * 4, s));
    if (d_pred_session || d_label_session) {
        k_hits_map<<<grid_for(S > P ? S : P, 256), 256, 0, s>>>(a);
        OTTO_HIP(hipGetLastError());
    }
    if (d_pred_off) k_hits_wave<<<(int)((S + 3) / 4 < 8192 ? (S + 3) / 4 : 8192), 256, 0, s>>>(a);
    else k_hits_group<<<grid_for(S, 256 / 8), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    k_hits_totals<<<capped_grid(S), 256, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    EvalScratch h;
    OTTO_TRY(read_scratch(a.sc, &h, s));
    if (h.unsorted) {
        set_error("otto_eval_hits: session ids are not ascending and distinct (%u places)", h.unsorted);
        return OTTO_EINVAL;
    }
    if (h.foreign) {
        set_error("otto_eval_hits: %u prediction sessions are not among the label sessions", h.foreign);
        return OTTO_EINVAL;
    }
    for (int i = 0; i < 4; ++i) h_totals[i] = (int64_t)h.tot[i];
    return 0;
}
