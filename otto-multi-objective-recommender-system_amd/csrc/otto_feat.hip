// Per-aid and per-session ranker columns and the feature matrix on the device (include/otto_feat.h, SPEC-FEAT, DESIGN.md
// section 3e; reference: src/ranker/aid_feature_engineering.py, src/ranker/session_feature_engineering.py and the joins of
// src/ranker/lgb_trainer.py:34-47).
//
// Aid table: one record per event (ts, session | type | start | end), one stable radix sort of the event indices by aid
// (the sort of otto_events.hip; the input is session-sorted, so an aid's segment arrives in (session, ts) order), a
// segmented reduce with one wave per aid segment and a workgroup per hot aid, exact integer sums, float64 finalisation by
// one lane; then one sort of every (rank column, value) key and two binary searches per (aid, column) for the rank columns.
// No global atomic on the per-event path: counts are ballots, sums are wave reductions.
// Session table: one wave per session, the aid-table columns summed in event order.
// Matrix: lanes run along the flattened (row, column) index of a tile, so every wave writes whole lines.
#include "common.h"
#include "sort.h"
#include "wave.h"
#include "../../include/otto_events.h"
#include "../../include/otto_feat.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace otto {

constexpr int FEAT_RANKED = 13;             // rank sources: count, days, type counts, type sessions, type days, last-week count, sessions
constexpr uint32_t FEAT_NULL = 0xFFFFFFFFu;
constexpr uint32_t FEAT_SESS_MASK = 0x0FFFFFFFu;
constexpr int64_t FEAT_HOT = 1024;          // events above which an aid segment gets a workgroup
constexpr uint32_t FEAT_EXACT = 1u << 24;   // integers up to here are float32 values
constexpr int FEAT_TILE = 256;              // matrix rows per workgroup

__constant__ const int c_rank_column[FEAT_RANKED] = {8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 29};

struct FeatCal {          // per day of the table
    uint8_t dow[OTTO_FEAT_MAX_DAYS];
    uint8_t slot[OTTO_FEAT_MAX_DAYS];      // week slot of the day's week
    uint8_t last_week[OTTO_FEAT_MAX_DAYS]; // 1: the day's week is the maximum week present
    int32_t day_min, n_days, n_slots, pad;
};

struct FeatProgram {      // one matrix column
    const void* base;
    int32_t sel;          // row index: 0 the row, 1 its session, 2 its candidate
    int32_t stride, col, kind;   // kind 0 float32, 1 uint16, 2 uint16 with 0 -> NaN
};

// wave-uniform totals of an aid segment (or of one wave's share of it)
struct AidTot {
    uint32_t tcnt[3], starts, ends, sess, tsess[3], lw_cnt, lw_sess;
    uint32_t ts_min, ts_max, lw_ts_min, lw_ts_max, pad;
    unsigned long long hour, hour2, dow, dow2, lw_dow;
    unsigned long long days, tdays[3];
    uint32_t slot[OTTO_FEAT_MAX_WEEK_SLOTS][3];
};

__device__ __forceinline__ uint32_t count_lanes(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// the session that owns event / row e: the largest s in [lo, hi] with off[s] <= e
__device__ __forceinline__ int64_t owner_of(const int64_t* off, int64_t lo, int64_t hi, int64_t e) {
    ++hi;                                   // first s in (lo, hi] with off[s] > e, minus one
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Per event: the sort key (aid), its index, the record the reduce gathers, and the first event index of every day.
__global__ __launch_bounds__(256) void k_feat_prep(const uint32_t* aid, const int32_t* ts, const uint8_t* type, const int64_t* off,
                                                   int64_t n_sess, int64_t n, uint32_t n_aids, int32_t day_min, int32_t n_days,
                                                   uint64_t* key, uint32_t* idx, uint2* rec, uint32_t* day_first, uint32_t* err) {
    __shared__ int64_t s_range[2];
    __shared__ uint32_t s_first[OTTO_FEAT_MAX_DAYS];
    const int64_t base = (int64_t)blockIdx.x * 1024;
    const int64_t last = (base + 1024 < n ? base + 1024 : n) - 1;
    if (threadIdx.x < OTTO_FEAT_MAX_DAYS) s_first[threadIdx.x] = FEAT_NULL;
    if (threadIdx.x < 2) s_range[threadIdx.x] = owner_of(off, 0, n_sess - 1, threadIdx.x == 0 ? base : last);
    __syncthreads();
    const int64_t s_lo = s_range[0], s_hi = s_range[1];
    const unsigned lane = lane_id();
    for (int c = 0; c < 4; ++c) {
        const int64_t i = base + (int64_t)c * 256 + threadIdx.x;
        int d = -1;
        if (i < n) {
            const int64_t s = s_lo >= 0 && s_hi >= s_lo ? owner_of(off, s_lo, s_hi, i) : -1;
            const uint32_t a = aid[i], ty = type[i];
            const int32_t t = ts[i];
            const int64_t day = t >= 0 ? ((int64_t)t + 7200) / 86400 - day_min : -1;
            const bool ok = s >= 0 && s < n_sess && a < n_aids && ty < 3 && day >= 0 && day < n_days;
            if (!ok) atomicAdd(err, 1u);
            else d = (int)day;
            const uint32_t start = ok && off[s] == i, end = ok && off[s + 1] == i + 1;
            key[i] = ok ? a : 0u;
            idx[i] = (uint32_t)i;
            rec[i] = make_uint2((uint32_t)t, ((uint32_t)(ok ? s : 0) & FEAT_SESS_MASK) | ((ty & 3u) << 28) | (start << 30) | (end << 31));
        }
        // lanes hold ascending event indices: the lowest lane of a day holds the wave's first event of that day
        unsigned long long todo = __ballot(d >= 0);
        while (todo) {
            const int leader = __ffsll(todo) - 1;
            const int dl = __shfl(d, leader, 64);
            if ((int)lane == leader) atomicMin(&s_first[dl], (uint32_t)i);
            todo &= ~__ballot(d == dl);
        }
    }
    __syncthreads();
    if (threadIdx.x < OTTO_FEAT_MAX_DAYS && s_first[threadIdx.x] != FEAT_NULL) atomicMin(&day_first[threadIdx.x], s_first[threadIdx.x]);
}

// aid_off[a] = the first sorted position whose aid is >= a, a in [0, n_aids]
__global__ void k_feat_bounds(const uint64_t* key, int64_t n, uint32_t n_aids, uint32_t* aid_off) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    const int64_t prev = p == 0 ? -1 : (int64_t)key[p - 1], cur = p == n ? (int64_t)n_aids : (int64_t)key[p];
    for (int64_t a = prev + 1; a <= cur; ++a) aid_off[a] = (uint32_t)p;
}

// One wave's share of the segment [lo, hi) of the sorted event indices: chunks wave, wave + n_waves, ... of 64 events.
__device__ void feat_scan(const uint32_t* order, const uint2* rec, const FeatCal* cal, int64_t lo, int64_t hi, int wave, int n_waves,
                          AidTot& t) {
    const unsigned lane = lane_id();
    const int n_slots = cal->n_slots, day_min = cal->day_min;
    unsigned long long hour = 0, hour2 = 0, dow = 0, dow2 = 0, lw_dow = 0, days = 0, tdays[3] = {0, 0, 0};
    uint32_t ts_min = FEAT_NULL, ts_max = 0, lw_ts_min = FEAT_NULL, lw_ts_max = 0;
    t = AidTot{};
    for (int64_t c = lo + (int64_t)wave * 64; c < hi; c += (int64_t)n_waves * 64) {
        const int64_t p = c + lane;
        const bool valid = p < hi;
        const uint2 r = valid ? rec[order[p]] : make_uint2(0u, 0u);
        const uint32_t sess = r.y & FEAT_SESS_MASK, ty = (r.y >> 28) & 3u;
        const uint32_t tt = r.x + 7200u, day = valid ? tt / 86400u - (uint32_t)day_min : 0u, hr = (tt % 86400u) / 3600u;
        const uint32_t dw = cal->dow[day], slot = cal->slot[day];
        const bool lw = valid && cal->last_week[day];
        // the head of a run of same-session events; same-session events of an aid are contiguous in its segment
        uint32_t before = (uint32_t)__shfl_up((int)sess, 1, 64);
        if (lane == 0 && c > lo) before = rec[order[c - 1]].y & FEAT_SESS_MASK;
        const bool head = valid && (p == lo || before != sess);
        uint32_t seen = 1u << ty;          // types (bits 0-2) and last-week membership (bit 3) anywhere in the head's run
        seen |= lw ? 8u : 0u;
        const uint32_t next_sess = (uint32_t)__shfl_down((int)sess, 1, 64);
        if (head && p + 1 < hi && (lane == 63 || next_sess == sess)) {
            for (int64_t q = p + 1; q < hi; ++q) {
                const uint2 r2 = rec[order[q]];
                if ((r2.y & FEAT_SESS_MASK) != sess) break;
                seen |= 1u << ((r2.y >> 28) & 3u);
                seen |= cal->last_week[(r2.x + 7200u) / 86400u - (uint32_t)day_min] ? 8u : 0u;
            }
        }
        t.starts += count_lanes(valid && ((r.y >> 30) & 1u));
        t.ends += count_lanes(valid && (r.y >> 31));
        t.sess += count_lanes(head);
        t.lw_cnt += count_lanes(lw);
        t.lw_sess += count_lanes(head && (seen & 8u));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t.tcnt[k] += count_lanes(valid && ty == (uint32_t)k);
            t.tsess[k] += count_lanes(head && ((seen >> k) & 1u));
        }
#pragma unroll
        for (int sl = 0; sl < OTTO_FEAT_MAX_WEEK_SLOTS; ++sl) {
            if (sl < n_slots) {
#pragma unroll
                for (int k = 0; k < 3; ++k) t.slot[sl][k] += count_lanes(valid && slot == (uint32_t)sl && ty == (uint32_t)k);
            }
        }
        if (valid) {
            hour += hr; hour2 += hr * hr; dow += dw; dow2 += dw * dw;
            days |= 1ull << day;
#pragma unroll
            for (int k = 0; k < 3; ++k) tdays[k] |= ty == (uint32_t)k ? 1ull << day : 0ull;
            ts_min = r.x < ts_min ? r.x : ts_min; ts_max = r.x > ts_max ? r.x : ts_max;
            if (lw) {
                lw_dow += dw;
                lw_ts_min = r.x < lw_ts_min ? r.x : lw_ts_min; lw_ts_max = r.x > lw_ts_max ? r.x : lw_ts_max;
            }
        }
    }
    t.hour = wave_reduce<Sum>(hour); t.hour2 = wave_reduce<Sum>(hour2); t.dow = wave_reduce<Sum>(dow); t.dow2 = wave_reduce<Sum>(dow2);
    t.lw_dow = wave_reduce<Sum>(lw_dow);
    t.days = wave_reduce<Or>(days);
#pragma unroll
    for (int k = 0; k < 3; ++k) t.tdays[k] = wave_reduce<Or>(tdays[k]);
    t.ts_min = wave_reduce<Min>(ts_min); t.ts_max = wave_reduce<Max>(ts_max);
    t.lw_ts_min = wave_reduce<Min>(lw_ts_min); t.lw_ts_max = wave_reduce<Max>(lw_ts_max);
}

__device__ void feat_merge(AidTot& a, const AidTot& b) {
    for (int k = 0; k < 3; ++k) { a.tcnt[k] += b.tcnt[k]; a.tsess[k] += b.tsess[k]; a.tdays[k] |= b.tdays[k]; }
    a.starts += b.starts; a.ends += b.ends; a.sess += b.sess; a.lw_cnt += b.lw_cnt; a.lw_sess += b.lw_sess;
    a.ts_min = b.ts_min < a.ts_min ? b.ts_min : a.ts_min; a.ts_max = b.ts_max > a.ts_max ? b.ts_max : a.ts_max;
    a.lw_ts_min = b.lw_ts_min < a.lw_ts_min ? b.lw_ts_min : a.lw_ts_min;
    a.lw_ts_max = b.lw_ts_max > a.lw_ts_max ? b.lw_ts_max : a.lw_ts_max;
    a.hour += b.hour; a.hour2 += b.hour2; a.dow += b.dow; a.dow2 += b.dow2; a.lw_dow += b.lw_dow; a.days |= b.days;
    for (int sl = 0; sl < OTTO_FEAT_MAX_WEEK_SLOTS; ++sl)
        for (int k = 0; k < 3; ++k) a.slot[sl][k] += b.slot[sl][k];
}

// sample std of n integers with sum s and sum of squares q; the integers of the quotient stay below 2^53 or the error word is set
__device__ float feat_std(unsigned long long n, unsigned long long s, unsigned long long q, uint32_t* err) {
    if (n < 2) return __builtin_nanf("");
    if (n >= (1ull << 26) || q >= (1ull << 53) / n) { atomicAdd(err, 1u); return __builtin_nanf(""); }
    return (float)sqrt((double)(n * q - s * s) / (double)(n * (n - 1)));
}

// One lane turns the totals of aid a into its row (the rank columns come later) and its rank sources.
__device__ void feat_finalize(const AidTot& t, int n_slots, uint32_t a, uint32_t n_aids, float* out, uint32_t* rank_val, uint32_t* err) {
    float* o = out + (size_t)a * OTTO_FEAT_AID_COLUMNS;
    const float nanf_ = __builtin_nanf("");
    const unsigned long long n = (unsigned long long)t.tcnt[0] + t.tcnt[1] + t.tcnt[2];
    uint32_t rv[FEAT_RANKED];
    for (int k = 0; k < FEAT_RANKED; ++k) rv[k] = FEAT_NULL;
    if (n == 0) {
        for (int q = 0; q < OTTO_FEAT_AID_COLUMNS; ++q) o[q] = nanf_;
    } else {
        if (n > FEAT_EXACT) atomicAdd(err, 1u);
        const double dn = (double)n;
        o[0] = (float)((double)(t.tcnt[1] + 2ull * t.tcnt[2]) / dn);
        o[1] = (float)((double)t.hour / dn);
        o[2] = feat_std(n, t.hour, t.hour2, err);
        o[3] = (float)((double)t.dow / dn);
        o[4] = feat_std(n, t.dow, t.dow2, err);
        o[5] = (float)((double)t.ts_max / (double)t.ts_min);
        o[6] = (float)((double)t.starts / dn);
        o[7] = (float)((double)t.ends / dn);
        rv[0] = (uint32_t)n; rv[1] = (uint32_t)__popcll(t.days); rv[12] = t.sess;
        for (int k = 0; k < 3; ++k) {
            if (t.tcnt[k]) { rv[2 + k] = t.tcnt[k]; rv[5 + k] = t.tsess[k]; rv[8 + k] = (uint32_t)__popcll(t.tdays[k]); }
        }
        if (t.lw_cnt) {
            rv[11] = t.lw_cnt;
            o[20] = (float)((double)t.lw_ts_max / (double)t.lw_ts_min);
            o[21] = (float)((double)t.lw_dow / (double)t.lw_cnt);
            o[30] = (float)t.lw_sess;
        } else {
            o[20] = o[21] = o[30] = nanf_;
        }
        for (int k = 0; k < 3; ++k) {
            double pct = (double)nanf_;
            uint32_t before = 0, last = 0;
            for (int sl = 0; sl < OTTO_FEAT_MAX_WEEK_SLOTS; ++sl) {
                if (sl >= n_slots) break;
                last = t.slot[sl][k];
                if (sl > 0) {
                    const double p = (double)last / (double)before - 1.0;     // pandas: filled / shifted - 1
                    if (p == p) pct = p;
                }
                before = last;
            }
            o[22 + k] = t.tcnt[k] ? (float)((double)last / (double)t.tcnt[k]) : 0.f;
            o[25 + k] = isinf(pct) ? nanf_ : (float)pct;
        }
        o[28] = (float)n;
    }
    for (int k = 0; k < FEAT_RANKED; ++k) rank_val[(size_t)k * n_aids + a] = rv[k];
}

__global__ __launch_bounds__(256) void k_feat_aid_wave(const uint32_t* order, const uint2* rec, const FeatCal* g_cal, const uint32_t* aid_off,
                                                       uint32_t n_aids, float* out, uint32_t* rank_val, uint32_t* hot, uint32_t* n_hot,
                                                       uint32_t* err) {
    __shared__ FeatCal s_cal;
    if (threadIdx.x < sizeof(FeatCal) / 4) reinterpret_cast<uint32_t*>(&s_cal)[threadIdx.x] = reinterpret_cast<const uint32_t*>(g_cal)[threadIdx.x];
    __syncthreads();
    const unsigned lane = lane_id();
    for (int64_t a = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); a < (int64_t)n_aids; a += (int64_t)gridDim.x * 4) {
        const int64_t lo = aid_off[a], hi = aid_off[a + 1];
        if (hi - lo > FEAT_HOT) {
            if (lane == 0) hot[atomicAdd(n_hot, 1u)] = (uint32_t)a;      // one atomic per hot aid
            continue;
        }
        AidTot t;
        feat_scan(order, rec, &s_cal, lo, hi, 0, 1, t);
        if (lane == 0) feat_finalize(t, s_cal.n_slots, (uint32_t)a, n_aids, out, rank_val, err);
    }
}

__global__ __launch_bounds__(256) void k_feat_aid_hot(const uint32_t* order, const uint2* rec, const FeatCal* g_cal, const uint32_t* aid_off,
                                                      uint32_t n_aids, float* out, uint32_t* rank_val, const uint32_t* hot,
                                                      const uint32_t* n_hot, uint32_t* err) {
    __shared__ FeatCal s_cal;
    __shared__ AidTot s_tot[4];
    if (threadIdx.x < sizeof(FeatCal) / 4) reinterpret_cast<uint32_t*>(&s_cal)[threadIdx.x] = reinterpret_cast<const uint32_t*>(g_cal)[threadIdx.x];
    __syncthreads();
    const int w = threadIdx.x >> 6;
    const uint32_t todo = *n_hot;
    for (uint32_t h = blockIdx.x; h < todo; h += gridDim.x) {
        const uint32_t a = hot[h];
        AidTot t;
        feat_scan(order, rec, &s_cal, aid_off[a], aid_off[a + 1], w, 4, t);
        if (lane_id() == 0) s_tot[w] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < 4; ++q) feat_merge(t, s_tot[q]);
            feat_finalize(t, s_cal.n_slots, a, n_aids, out, rank_val, err);
        }
        __syncthreads();
    }
}

__global__ void k_feat_rank_keys(const uint32_t* rank_val, int64_t n, uint32_t n_aids, uint64_t* key, uint32_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = ((uint64_t)(i / n_aids) << 32) | rank_val[i];
    idx[i] = (uint32_t)i;
}

__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t* v, int64_t n, uint64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// rank(pct=True), average method, of column c over its non-null aids: (less + (equal + 1) / 2) / N
__global__ void k_feat_rank_write(const uint32_t* rank_val, const uint64_t* sorted, int64_t n, uint32_t n_aids, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = (uint64_t)(i / n_aids);
    const uint32_t a = (uint32_t)(i % n_aids), v = rank_val[i];
    float r = __builtin_nanf("");
    if (v != FEAT_NULL) {
        const int64_t first = lower_bound_u64(sorted, n, c << 32), stop = lower_bound_u64(sorted, n, (c << 32) | FEAT_NULL);
        const int64_t less = lower_bound_u64(sorted, n, (c << 32) | v) - first;
        const int64_t equal = lower_bound_u64(sorted, n, ((c << 32) | v) + 1) - first - less;
        r = (float)(((double)less + (double)(equal + 1) * 0.5) / (double)(stop - first));
    }
    out[(size_t)a * OTTO_FEAT_AID_COLUMNS + c_rank_column[c]] = r;
}

// One wave per session: its aids sit in LDS for the distinct count, the aid-table columns are added in event order.
__global__ __launch_bounds__(256) void k_feat_session(const uint32_t* aid, const int32_t* ts, const uint8_t* type, const int64_t* off,
                                                      int64_t n_sess, const float* table, uint32_t n_aids, const FeatCal* g_cal, float* out,
                                                      uint32_t* err) {
    __shared__ uint32_t s_aid[4][OTTO_FEAT_MAX_SESSION];
    __shared__ FeatCal s_cal;
    if (threadIdx.x < sizeof(FeatCal) / 4) reinterpret_cast<uint32_t*>(&s_cal)[threadIdx.x] = reinterpret_cast<const uint32_t*>(g_cal)[threadIdx.x];
    __syncthreads();
    const int w = threadIdx.x >> 6;
    const unsigned lane = lane_id();
    const float nanf_ = __builtin_nanf("");
    const int cols[5] = {28, 0, 1, 29, 30};        // aid_count, aid_type_mean, aid_hour_mean, session rank, last-week sessions
    for (int64_t s = (int64_t)blockIdx.x * 4 + w; s < n_sess; s += (int64_t)gridDim.x * 4) {
        const int64_t lo = off[s];
        int64_t n64 = off[s + 1] - lo;
        if (n64 < 0 || n64 > OTTO_FEAT_MAX_SESSION) {
            if (lane == 0) atomicAdd(err, 1u);
            n64 = n64 < 0 ? 0 : OTTO_FEAT_MAX_SESSION;
        }
        const int n = (int)n64;
        for (int i = (int)lane; i < n; i += 64) s_aid[w][i] = aid[lo + i];
        wave_lds_sync();
        uint32_t uniq = 0;
        for (int i = (int)lane; i < n; i += 64) {
            const uint32_t a = s_aid[w][i];
            bool first = true;
            for (int j = 0; j < i; ++j) first = first && s_aid[w][j] != a;
            uniq += first ? 1u : 0u;
        }
        uniq = wave_reduce<Sum>(uniq);
        double sum[5] = {0, 0, 0, 0, 0};
        uint32_t cnt[5] = {0, 0, 0, 0, 0};
        float last[5] = {nanf_, nanf_, nanf_, nanf_, nanf_}, cmin = nanf_, cmax = nanf_;
        for (int b = 0; b < n; b += 64) {
            const int i = b + (int)lane;
            float v[5] = {nanf_, nanf_, nanf_, nanf_, nanf_};
            if (i < n) {
                const uint32_t a = s_aid[w][i];
                if (a < n_aids) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) v[k] = table[(size_t)a * OTTO_FEAT_AID_COLUMNS + cols[k]];
                } else {
                    atomicAdd(err, 1u);
                }
            }
            const int m = n - b < 64 ? n - b : 64;
            for (int j = 0; j < m; ++j) {             // event order; every lane keeps the same sums
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), j));
                    if (x == x) {
                        sum[k] += (double)x; ++cnt[k]; last[k] = x;
                        if (k == 0) { cmin = cmin == cmin && cmin < x ? cmin : x; cmax = cmax == cmax && cmax > x ? cmax : x; }
                    }
                }
            }
        }
        if (lane == 0) {
            float* o = out + (size_t)s * OTTO_FEAT_SESSION_COLUMNS;
            for (int q = 0; q < OTTO_FEAT_SESSION_COLUMNS; ++q) o[q] = nanf_;
            o[0] = (float)n;
            o[1] = (float)(uniq & 255u);
            if (n > 0) {
                const uint32_t a = s_aid[w][n - 1];
                const int32_t t = ts[lo + n - 1];
                const int64_t day = t >= 0 ? ((int64_t)t + 7200) / 86400 - s_cal.day_min : -1;
                if (a > FEAT_EXACT || day < 0 || day >= s_cal.n_days) atomicAdd(err, 1u);
                o[2] = (float)a;
                o[3] = (float)type[lo + n - 1];
                o[4] = day >= 0 && day < s_cal.n_days ? (float)s_cal.dow[day] : nanf_;
                o[5] = cnt[0] ? (float)(sum[0] / (double)cnt[0]) : nanf_;
                o[6] = cmin; o[7] = cmax; o[8] = last[0];
                o[9] = cnt[1] ? (float)(sum[1] / (double)cnt[1]) : nanf_;
                o[10] = cnt[2] ? (float)(sum[2] / (double)cnt[2]) : nanf_;
                o[11] = cnt[3] ? (float)(sum[3] / (double)cnt[3]) : nanf_;
                o[12] = last[3];
                o[13] = cnt[4] ? (float)(sum[4] / (double)cnt[4]) : nanf_;
                o[14] = last[4];
            }
        }
        wave_lds_sync();
    }
}

// A workgroup per tile of FEAT_TILE rows. Lanes run along the flattened (row, column) index, so a wave-instruction writes
// 256 consecutive bytes of the matrix and reads the columns one source holds for a row from one line of that source.
__global__ __launch_bounds__(256) void k_feat_matrix(const int64_t* row_off, int64_t n_sess, const int32_t* cand, int64_t n_rows,
                                                     uint32_t n_aids, const FeatProgram* g_prog, int F, float* out, uint32_t* err) {
    __shared__ FeatProgram s_prog[OTTO_FEAT_MAX_COLUMNS];
    __shared__ int64_t s_range[2];
    __shared__ int64_t s_index[3][FEAT_TILE];       // per row of the tile: the row, its session, its candidate (-1: none)
    const int64_t row0 = (int64_t)blockIdx.x * FEAT_TILE;
    const int rows = (int)(n_rows - row0 < FEAT_TILE ? n_rows - row0 : FEAT_TILE);
    if ((int)threadIdx.x < F) s_prog[threadIdx.x] = g_prog[threadIdx.x];
    if (threadIdx.x < 2) s_range[threadIdx.x] = owner_of(row_off, 0, n_sess - 1, threadIdx.x == 0 ? row0 : row0 + rows - 1);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        const int64_t r = row0 + threadIdx.x;
        const int64_t s = s_range[0] >= 0 && s_range[1] >= s_range[0] ? owner_of(row_off, s_range[0], s_range[1], r) : -1;
        const int32_t y = cand[r];
        const bool ok = y >= 0 && (uint32_t)y < n_aids && s >= 0 && s < n_sess && row_off[s + 1] > r;
        if (!ok) atomicAdd(err, 1u);
        s_index[0][threadIdx.x] = r;
        s_index[1][threadIdx.x] = ok ? s : -1;
        s_index[2][threadIdx.x] = ok ? y : -1;
    }
    __syncthreads();
    const int total = rows * F, step_r = 256 / F, step_f = 256 % F;
    int r = (int)threadIdx.x / F, f = (int)threadIdx.x % F;
    float* o = out + (size_t)row0 * F;
    for (int i = threadIdx.x; i < total; i += 256) {
        const FeatProgram p = s_prog[f];
        const int64_t at = s_index[p.sel][r];
        float v = __builtin_nanf("");
        if (at >= 0) {
            const size_t e = (size_t)at * p.stride + p.col;
            if (p.kind == 0) {
                v = reinterpret_cast<const float*>(p.base)[e];
            } else {
                const uint16_t u = reinterpret_cast<const uint16_t*>(p.base)[e];
                v = p.kind == 2 && u == 0 ? v : (float)u;
            }
        }
        o[i] = v;
        r += step_r; f += step_f;
        if (f >= F) { f -= F; ++r; }
    }
}


struct AidWs {
    uint32_t* err;          // [0] error word, [1] hot aids
    FeatCal* cal;
    uint32_t* day_first;    // [64]
    uint32_t* aid_off;      // [n_aids + 1]
    uint2* rec;             // [n]
    uint32_t* rank_val;     // [13][n_aids]
    uint32_t* hot;          // [n / FEAT_HOT + 1]
    char* sort;
};

static size_t aid_ws_layout(int64_t n, uint32_t n_aids, char* base, AidWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    char* e = take(256); char* c = take(sizeof(FeatCal)); char* d = take(OTTO_FEAT_MAX_DAYS * 4);
    char* a = take(((size_t)n_aids + 1) * 4); char* r = take((size_t)n * 8); char* v = take((size_t)FEAT_RANKED * n_aids * 4);
    char* h = take(((size_t)n / FEAT_HOT + 1) * 4);
    const int64_t n_rank = (int64_t)FEAT_RANKED * n_aids;
    char* s = take((size_t)otto_events_sort_workspace(n > n_rank ? n : n_rank));
    if (w) {
        w->err = (uint32_t*)e; w->cal = (FeatCal*)c; w->day_first = (uint32_t*)d; w->aid_off = (uint32_t*)a; w->rec = (uint2*)r;
        w->rank_val = (uint32_t*)v; w->hot = (uint32_t*)h; w->sort = s;
    }
    return o;
}

// the day table -> per-day day_of_week; present days in order of their first event -> week slots and the last week
static int make_calendar(int32_t day_min, int32_t n_days, const int32_t* h_days, const uint32_t* first, FeatCal* cal) {
    *cal = FeatCal{};
    cal->day_min = day_min; cal->n_days = n_days;
    for (int d = 0; d < n_days; ++d) {
        OTTO_REQUIRE(h_days[3 * d] >= 0 && h_days[3 * d] < 7 && h_days[3 * d + 2] >= 1 && h_days[3 * d + 2] <= 53,
                     "day table row %d: day_of_week %d / week_of_year %d out of range", d, h_days[3 * d], h_days[3 * d + 2]);
        cal->dow[d] = (uint8_t)h_days[3 * d];
    }
    if (!first) return 0;
    std::vector<int> present;
    for (int d = 0; d < n_days; ++d)
        if (first[d] != FEAT_NULL) present.push_back(d);
    std::sort(present.begin(), present.end(), [&](int x, int y) { return first[x] < first[y]; });
    std::vector<int> slots;
    int last_week = 0;
    for (int d : present) {
        const int wk = h_days[3 * d + 2];
        if (std::find(slots.begin(), slots.end(), wk) == slots.end()) slots.push_back(wk);
        last_week = wk > last_week ? wk : last_week;
    }
    OTTO_REQUIRE((int)slots.size() <= OTTO_FEAT_MAX_WEEK_SLOTS, "%d distinct weeks, at most %d", (int)slots.size(), OTTO_FEAT_MAX_WEEK_SLOTS);
    cal->n_slots = (int)slots.size();
    for (int d = 0; d < n_days; ++d) {
        const int wk = h_days[3 * d + 2];
        const auto it = std::find(slots.begin(), slots.end(), wk);
        cal->slot[d] = it == slots.end() ? 255 : (uint8_t)(it - slots.begin());
        cal->last_week[d] = wk == last_week;
    }
    return 0;
}

static int read_error(uint32_t* d_err, hipStream_t s, const char* what) {
    uint32_t herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(herr == 0, "%s: %u bad inputs (%s)", what, herr,
                 "index outside its table, day outside the day table, type > 2, ts < 0, session too long, or an integer above 2^24");
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_feat_aid_table_workspace(int64_t n_events, uint32_t n_aids) {
    if (n_events < 0) return 0;
    return (int64_t)aid_ws_layout(n_events, n_aids, nullptr, nullptr);
}

extern "C" int otto_feat_aid_table(const uint32_t* d_aid, const int32_t* d_ts, const uint8_t* d_type, const int64_t* d_sess_off,
                                   int64_t n_sess, int64_t n, uint32_t n_aids, int32_t day_min, int32_t n_days, const int32_t* h_days,
                                   float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    OTTO_REQUIRE(n_days >= 1 && n_days <= OTTO_FEAT_MAX_DAYS, "the day table spans %d days, expected 1 to %d", n_days, OTTO_FEAT_MAX_DAYS);
    OTTO_REQUIRE(n >= 0 && n < (1ll << 32) && n_sess >= 0 && n_sess < (1ll << 28), "n_events must be below 2^32, n_sess below 2^28");
    OTTO_REQUIRE(n_aids > 0 && n_aids < (1u << 28) && h_days && d_out && d_ws, "otto_feat_aid_table: bad argument");
    OTTO_REQUIRE(n == 0 || (n_sess > 0 && d_aid && d_ts && d_type && d_sess_off), "otto_feat_aid_table: null argument");
    OTTO_REQUIRE(ws_bytes >= otto_feat_aid_table_workspace(n, n_aids), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    AidWs w;
    aid_ws_layout(n, n_aids, (char*)d_ws, &w);
    FeatCal cal;
    OTTO_TRY(make_calendar(day_min, n_days, h_days, nullptr, &cal));
    OTTO_HIP(hipMemsetAsync(w.err, 0, 256, s));
    OTTO_HIP(hipMemsetAsync(w.day_first, 0xFF, OTTO_FEAT_MAX_DAYS * 4, s));
    uint64_t *key0, *scan_out, *scan_partial, *sorted_key = nullptr;
    uint32_t *val0, *order = nullptr;
    if (n > 0) {
        otto_sort_ws_buffers(n, w.sort, &key0, &val0, &scan_out, &scan_partial);
        k_feat_prep<<<(unsigned)((n + 1023) / 1024), 256, 0, s>>>(d_aid, d_ts, d_type, d_sess_off, n_sess, n, n_aids, day_min, n_days, key0, val0,
                                                                w.rec, w.day_first, w.err);
        OTTO_HIP(hipGetLastError());
    }
    uint32_t first[OTTO_FEAT_MAX_DAYS];
    OTTO_HIP(hipMemcpyAsync(first, w.day_first, sizeof first, hipMemcpyDeviceToHost, s));
    OTTO_TRY(read_error(w.err, s, "otto_feat_aid_table"));
    OTTO_TRY(make_calendar(day_min, n_days, h_days, first, &cal));
    OTTO_HIP(hipMemcpyAsync(w.cal, &cal, sizeof cal, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipStreamSynchronize(s));          // cal is a stack variable
    if (n > 0) OTTO_TRY(otto_sort_pairs_in_ws(key0, n, w.sort, &sorted_key, &order, s));
    k_feat_bounds<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(sorted_key, n, n_aids, w.aid_off);
    OTTO_HIP(hipGetLastError());
    const int64_t blocks = ((int64_t)n_aids + 3) / 4;
    k_feat_aid_wave<<<(unsigned)(blocks < 256 * 16 ? blocks : 256 * 16), 256, 0, s>>>(order, w.rec, w.cal, w.aid_off, n_aids, d_out, w.rank_val,
                                                                                      w.hot, w.err + 1, w.err);
    OTTO_HIP(hipGetLastError());
    k_feat_aid_hot<<<1024, 256, 0, s>>>(order, w.rec, w.cal, w.aid_off, n_aids, d_out, w.rank_val, w.hot, w.err + 1, w.err);
    OTTO_HIP(hipGetLastError());
    // the event sort's buffers are free now: one sort of every (rank column, value)
    const int64_t n_rank = (int64_t)FEAT_RANKED * n_aids;
    otto_sort_ws_buffers(n_rank, w.sort, &key0, &val0, &scan_out, &scan_partial);
    k_feat_rank_keys<<<(unsigned)((n_rank + 255) / 256), 256, 0, s>>>(w.rank_val, n_rank, n_aids, key0, val0);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(otto_sort_pairs_in_ws(key0, n_rank, w.sort, &sorted_key, &order, s));
    k_feat_rank_write<<<(unsigned)((n_rank + 255) / 256), 256, 0, s>>>(w.rank_val, sorted_key, n_rank, n_aids, d_out);
    OTTO_HIP(hipGetLastError());
    return read_error(w.err, s, "otto_feat_aid_table");
}

extern "C" int64_t otto_feat_session_table_workspace(int64_t n_sess) { return n_sess < 0 ? 0 : 256 + (int64_t)align256(sizeof(FeatCal)); }

extern "C" int otto_feat_session_table(const uint32_t* d_aid, const int32_t* d_ts, const uint8_t* d_type, const int64_t* d_sess_off,
                                       int64_t n_sess, const float* d_aid_table, uint32_t n_aids, int32_t day_min, int32_t n_days,
                                       const int32_t* h_days, float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    OTTO_REQUIRE(n_days >= 1 && n_days <= OTTO_FEAT_MAX_DAYS, "the day table spans %d days, expected 1 to %d", n_days, OTTO_FEAT_MAX_DAYS);
    OTTO_REQUIRE(n_sess >= 0 && n_aids > 0 && h_days && d_ws, "otto_feat_session_table: bad argument");
    OTTO_REQUIRE(ws_bytes >= otto_feat_session_table_workspace(n_sess), "workspace too small");
    if (n_sess == 0) return 0;
    OTTO_REQUIRE(d_aid && d_ts && d_type && d_sess_off && d_aid_table && d_out, "otto_feat_session_table: null argument");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = (uint32_t*)d_ws;
    FeatCal* d_cal = (FeatCal*)((char*)d_ws + 256);
    FeatCal cal;
    OTTO_TRY(make_calendar(day_min, n_days, h_days, nullptr, &cal));
    OTTO_HIP(hipMemsetAsync(err, 0, 256, s));
    OTTO_HIP(hipMemcpyAsync(d_cal, &cal, sizeof cal, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipStreamSynchronize(s));          // cal is a stack variable
    const int64_t blocks = (n_sess + 3) / 4;
    k_feat_session<<<(unsigned)(blocks < 256 * 16 ? blocks : 256 * 16), 256, 0, s>>>(d_aid, d_ts, d_type, d_sess_off, n_sess, d_aid_table, n_aids,
                                                                                     d_cal, d_out, err);
    OTTO_HIP(hipGetLastError());
    return read_error(err, s, "otto_feat_session_table");
}

extern "C" int64_t otto_feat_matrix_workspace(int64_t n_rows) {
    return n_rows < 0 ? 0 : 256 + (int64_t)align256(sizeof(FeatProgram) * OTTO_FEAT_MAX_COLUMNS);
}

extern "C" int otto_feat_matrix(const int64_t* d_row_off, int64_t n_sess, const int32_t* d_cand, const float* d_score, int64_t n_rows,
                                const uint16_t* d_inter_row, const float* d_inter_sess, const float* d_inter_aid,
                                const float* d_aid_table, const float* d_sess_table, uint32_t n_aids, const int32_t* h_program, int32_t F,
                                float* d_out, void* d_ws, int64_t ws_bytes, void* stream) {
    OTTO_REQUIRE(F >= 1 && F <= OTTO_FEAT_MAX_COLUMNS && h_program, "F must be in [1, %d]", OTTO_FEAT_MAX_COLUMNS);
    OTTO_REQUIRE(n_rows >= 0 && n_sess >= 0 && n_aids > 0 && d_ws, "otto_feat_matrix: bad argument");
    OTTO_REQUIRE(ws_bytes >= otto_feat_matrix_workspace(n_rows), "workspace too small");
    const struct { const void* base; int sel, width; } src[6] = {
        {d_score, 0, 1}, {d_inter_row, 0, 5}, {d_inter_sess, 1, 10}, {d_inter_aid, 2, 9},
        {d_aid_table, 2, OTTO_FEAT_AID_COLUMNS}, {d_sess_table, 1, OTTO_FEAT_SESSION_COLUMNS}};
    FeatProgram prog[OTTO_FEAT_MAX_COLUMNS] = {};
    for (int f = 0; f < F; ++f) {
        const int sc = h_program[2 * f], col = h_program[2 * f + 1];
        OTTO_REQUIRE(sc >= 0 && sc < 6, "column %d: source %d is none of 0..5", f, sc);
        OTTO_REQUIRE(col >= 0 && col < src[sc].width, "column %d: source %d has no column %d", f, sc, col);
        OTTO_REQUIRE(n_rows == 0 || src[sc].base, "column %d: source %d is NULL", f, sc);
        prog[f].base = src[sc].base; prog[f].sel = src[sc].sel; prog[f].stride = src[sc].width; prog[f].col = col;
        prog[f].kind = sc == OTTO_FEAT_SRC_INTER_ROW ? (col == 1 ? 2 : 1) : 0;
    }
    if (n_rows == 0) return 0;
    OTTO_REQUIRE(n_sess > 0 && d_row_off && d_cand && d_out, "otto_feat_matrix: null argument");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* err = (uint32_t*)d_ws;
    FeatProgram* d_prog = (FeatProgram*)((char*)d_ws + 256);
    OTTO_HIP(hipMemsetAsync(err, 0, 256, s));
    OTTO_HIP(hipMemcpyAsync(d_prog, prog, sizeof(FeatProgram) * F, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipStreamSynchronize(s));          // prog is a stack variable
    k_feat_matrix<<<(unsigned)((n_rows + FEAT_TILE - 1) / FEAT_TILE), 256, 0, s>>>(d_row_off, n_sess, d_cand, n_rows, n_aids, d_prog, F, d_out, err);
    OTTO_HIP(hipGetLastError());
    return read_error(err, s, "otto_feat_matrix");
}
