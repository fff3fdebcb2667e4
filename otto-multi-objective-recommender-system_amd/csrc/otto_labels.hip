// Label assembly for MI355X (gfx950): the (session, type, list of aids) rows of val_labels.parquet -> three CSR label lists
// aligned to a session list. C-ABI and SPEC-LABELS in include/otto_labels.h.
//
//   k_lab_claim   one lane per row: range checks, a binary search of the session list, atomicMin(owner[3 pos + type], row);
//                 the rows without a label session are counted with one atomic per wave.
//   k_lab_check   one lane per row: a kept row that is not the owner of its (session, type) is the duplicate.
//   k_lab_values  one lane per value: the range check; only a bad value looks up its row.
//   scan.h        per type an exclusive scan over the sessions of the owner's list length -> out_off[t].
//   k_lab_fill    one lane per value: its row by an upper bound over off, its slot from out_off; coalesced reads.
#include "common.h"
#include "wave.h"
#include "scan.h"
#include "../../include/otto_labels.h"

namespace otto {

constexpr int LAB_THREADS = 256;
constexpr unsigned long long LAB_NONE = ~0ull;

struct LabWs {
    unsigned long long* err;      // row << 8 | reason of the smallest offending row, ~0 without one
    unsigned long long* dropped;
    int32_t* pos;                 // [n_rows]  the row's position in the session list, -1: dropped
    unsigned long long* owner;    // [3 * n_sessions]
    uint64_t* partial;            // scan.h
};

static size_t lab_layout(int64_t n_rows, int64_t n_sessions, char* base, LabWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    LabWs t;
    t.err = (unsigned long long*)take(8);
    t.dropped = (unsigned long long*)take(8);
    t.pos = (int32_t*)take((size_t)n_rows * 4);
    t.owner = (unsigned long long*)take((size_t)n_sessions * 24);
    t.partial = (uint64_t*)take(scan_partial_bytes(n_sessions));
    if (w) *w = t;
    return o;
}

static const char* lab_reason(int64_t r) {
    static const char* const names[] = {"no violation", "a session outside int32", "a type code above 2", "list offsets that descend or leave the values",
                                        "the same (session, type) as an earlier row", "a value outside [0, n_aids)"};
    return r >= 0 && r <= OTTO_LABELS_E_VALUE ? names[r] : "?";
}

// the last row r in [0, n_rows) with off[r] <= i, or -1
__device__ __forceinline__ int64_t lab_row_of(const int64_t* __restrict__ off, int64_t n_rows, int64_t i) {
    int64_t lo = 0, hi = n_rows;                             // first r with off[r] > i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__global__ __launch_bounds__(LAB_THREADS) void k_lab_claim(const int64_t* __restrict__ session, const uint8_t* __restrict__ type,
                                                           const int64_t* __restrict__ off, int64_t n_rows, int64_t n_values,
                                                           const int32_t* __restrict__ lsess, int64_t n_sessions, int32_t* __restrict__ pos,
                                                           unsigned long long* owner, unsigned long long* dropped, unsigned long long* err) {
    const int64_t r = (int64_t)blockIdx.x * LAB_THREADS + threadIdx.x;
    const bool live = r < n_rows;
    int bad = 0;
    int64_t p = -1;
    if (live) {
        const int64_t s = session[r], a = off[r], z = off[r + 1];
        const int t = type[r];
        if (s < -2147483648ll || s > 2147483647ll) bad = OTTO_LABELS_E_SESSION;
        else if (t > 2) bad = OTTO_LABELS_E_TYPE;
        else if (a < 0 || z < a || z > n_values) bad = OTTO_LABELS_E_OFFSETS;
        if (!bad) {
            int64_t lo = 0, hi = n_sessions;                 // first position with lsess >= s
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)lsess[mid] < s) lo = mid + 1; else hi = mid;
            }
            if (lo < n_sessions && (int64_t)lsess[lo] == s) {
                p = lo;
                atomicMin(&owner[3 * p + t], (unsigned long long)r);
            }
        } else {
            atomicMin(err, (unsigned long long)r << 8 | (unsigned long long)bad);
        }
        pos[r] = (int32_t)p;
    }
    const unsigned long long m = __ballot(live && !bad && p < 0);
    if (lane_id() == 0 && m) atomicAdd(dropped, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(LAB_THREADS) void k_lab_check(const uint8_t* __restrict__ type, int64_t n_rows, const int32_t* __restrict__ pos,
                                                           const unsigned long long* __restrict__ owner, unsigned long long* err) {
    const int64_t r = (int64_t)blockIdx.x * LAB_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p = pos[r];
    if (p >= 0 && owner[3 * p + type[r]] != (unsigned long long)r) atomicMin(err, (unsigned long long)r << 8 | (unsigned long long)OTTO_LABELS_E_DUP);
}

__global__ __launch_bounds__(LAB_THREADS) void k_lab_values(const int64_t* __restrict__ value, int64_t n_values, const int64_t* __restrict__ off,
                                                            int64_t n_rows, int64_t n_aids, unsigned long long* err) {
    const int64_t i = (int64_t)blockIdx.x * LAB_THREADS + threadIdx.x;
    if (i >= n_values) return;
    const int64_t v = value[i];
    if (v >= 0 && v < n_aids) return;
    const int64_t r = lab_row_of(off, n_rows, i);
    if (r >= 0 && i < off[r + 1]) atomicMin(err, (unsigned long long)r << 8 | (unsigned long long)OTTO_LABELS_E_VALUE);
}

struct LabLen {                                              // the list length of (session position, type)
    const unsigned long long* owner;
    const int64_t* off;
    const uint8_t* null;
    int t;
    __device__ uint64_t operator()(int64_t p) const {
        const unsigned long long o = owner[3 * p + t];
        if (o == LAB_NONE || null[o]) return 0;
        const int64_t n = off[o + 1] - off[o];
        return n > 0 ? (uint64_t)n : 0;
    }
};

struct LabOut {
    const int64_t* off[3];
    int32_t* aid[3];
};

__global__ __launch_bounds__(LAB_THREADS) void k_lab_fill(const int64_t* __restrict__ value, int64_t n_values, const int64_t* __restrict__ off,
                                                          const uint8_t* __restrict__ type, const uint8_t* __restrict__ null, int64_t n_rows,
                                                          const int32_t* __restrict__ pos, const unsigned long long* __restrict__ owner, LabOut out) {
    const int64_t i = (int64_t)blockIdx.x * LAB_THREADS + threadIdx.x;
    if (i >= n_values) return;
    const int64_t r = lab_row_of(off, n_rows, i);
    if (r < 0 || i >= off[r + 1]) return;                    // a value of no row
    const int64_t p = pos[r];
    if (p < 0 || null[r]) return;
    const int t = type[r];
    if (owner[3 * p + t] != (unsigned long long)r) return;   // only the owner's length was scanned
    out.aid[t][out.off[t][p] + (i - off[r])] = (int32_t)value[i];
}

static int lab_check(const otto_labels_job* j) {
    OTTO_REQUIRE(j, "otto_labels: null job");
    OTTO_REQUIRE(j->n_rows >= 0 && j->n_rows < (1ll << 40), "otto_labels: n_rows must be in [0, 2^40) (got %lld)", (long long)j->n_rows);
    OTTO_REQUIRE(j->n_values >= 0 && j->n_values < (1ll << 40), "otto_labels: n_values must be in [0, 2^40) (got %lld)", (long long)j->n_values);
    OTTO_REQUIRE(j->n_sessions >= 0 && j->n_sessions < (1ll << 31), "otto_labels: n_sessions must be in [0, 2^31) (got %lld)", (long long)j->n_sessions);
    OTTO_REQUIRE(j->n_aids >= 0 && j->n_aids < (1ll << 31), "otto_labels: n_aids must be in [0, 2^31) (got %lld)", (long long)j->n_aids);
    return 0;
}

static int lab_args(const otto_labels_job& j, LabWs* w) {
    OTTO_REQUIRE(j.d_off && (j.n_rows == 0 || (j.d_session && j.d_type && j.d_null)) && (j.n_values == 0 || j.d_value), "otto_labels: null input");
    OTTO_REQUIRE(j.n_sessions == 0 || j.d_label_session, "otto_labels: null session list");
    OTTO_REQUIRE(j.d_out_off[0] && j.d_out_off[1] && j.d_out_off[2], "otto_labels: null output offsets");
    const int64_t need = (int64_t)lab_layout(j.n_rows, j.n_sessions, (char*)j.d_work, w);
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0 && j.work_bytes >= need, "otto_labels: workspace of %lld 256-byte aligned bytes needed",
                 (long long)need);
    return 0;
}

static inline unsigned lab_grid(int64_t n) { return (unsigned)((n + LAB_THREADS - 1) / LAB_THREADS); }

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_labels_workspace(const otto_labels_job* job) {
    if (lab_check(job) != 0) return -22;
    return (int64_t)lab_layout(job->n_rows, job->n_sessions, nullptr, nullptr);
}

extern "C" int otto_labels_count(const otto_labels_job* job, int64_t* h_counts, int64_t* h_err) {
    OTTO_REQUIRE(h_err && h_counts, "otto_labels_count: null h_counts or h_err");
    h_err[0] = -1;
    h_err[1] = 0;
    h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
    OTTO_TRY(lab_check(job));
    const otto_labels_job& j = *job;
    LabWs w;
    OTTO_TRY(lab_args(j, &w));
    hipStream_t s = (hipStream_t)j.stream;
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    OTTO_HIP(hipMemsetAsync(w.dropped, 0, 8, s));
    if (j.n_sessions > 0) OTTO_HIP(hipMemsetAsync(w.owner, 0xFF, (size_t)j.n_sessions * 24, s));
    if (j.n_rows > 0) {
        k_lab_claim<<<lab_grid(j.n_rows), LAB_THREADS, 0, s>>>(j.d_session, j.d_type, j.d_off, j.n_rows, j.n_values, j.d_label_session, j.n_sessions,
                                                                 w.pos, w.owner, w.dropped, w.err);
        k_lab_check<<<lab_grid(j.n_rows), LAB_THREADS, 0, s>>>(j.d_type, j.n_rows, w.pos, w.owner, w.err);
        OTTO_HIP(hipGetLastError());
    }
    if (j.n_values > 0 && j.n_rows > 0) {
        k_lab_values<<<lab_grid(j.n_values), LAB_THREADS, 0, s>>>(j.d_value, j.n_values, j.d_off, j.n_rows, j.n_aids, w.err);
        OTTO_HIP(hipGetLastError());
    }
    for (int t = 0; t < 3; ++t)
        OTTO_TRY(device_scan(LabLen{w.owner, j.d_off, j.d_null, t}, j.n_sessions, (uint64_t*)j.d_out_off[t], w.partial, s));
    unsigned long long herr = 0, dropped = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipMemcpyAsync(&dropped, w.dropped, 8, hipMemcpyDeviceToHost, s));
    for (int t = 0; t < 3; ++t) OTTO_HIP(hipMemcpyAsync(h_counts + t, j.d_out_off[t] + j.n_sessions, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != LAB_NONE) {
        h_err[0] = (int64_t)(herr >> 8);
        h_err[1] = (int64_t)(herr & 0xFF);
        h_counts[0] = h_counts[1] = h_counts[2] = 0;
        OTTO_REQUIRE(false, "otto_labels_count: row %lld: %s", (long long)h_err[0], lab_reason(h_err[1]));
    }
    h_counts[3] = (int64_t)dropped;
    return 0;
}

extern "C" int otto_labels_fill(const otto_labels_job* job) {
    OTTO_TRY(lab_check(job));
    const otto_labels_job& j = *job;
    LabWs w;
    OTTO_TRY(lab_args(j, &w));
    if (j.n_values == 0 || j.n_rows == 0 || j.n_sessions == 0) return 0;
    OTTO_REQUIRE(j.d_out_aid[0] && j.d_out_aid[1] && j.d_out_aid[2], "otto_labels_fill: null output lists");
    LabOut out;
    for (int t = 0; t < 3; ++t) {
        out.off[t] = j.d_out_off[t];
        out.aid[t] = j.d_out_aid[t];
    }
    k_lab_fill<<<lab_grid(j.n_values), LAB_THREADS, 0, (hipStream_t)j.stream>>>(j.d_value, j.n_values, j.d_off, j.d_type, j.d_null, j.n_rows, w.pos,
                                                                                w.owner, out);
    OTTO_HIP(hipGetLastError());
    return 0;
}
