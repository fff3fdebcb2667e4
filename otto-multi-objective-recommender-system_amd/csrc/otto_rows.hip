// Rows -> resident top-k for MI355X (gfx950): the (aid_x, aid_y, wgt) rows of the covisitation part files back into the padded
// [n_aids, k] arrays the candidate lookup takes. C-ABI and SPEC-ROWS in include/otto_rows.h.
//
//   k_rows_topk  one wave per 64 consecutive rows. Every lane loads its row and its two neighbours' aid_x; a ballot of the
//                head flags (aid_x differs from the previous row's) gives the lane its run's start inside the wave. Only
//                the run that began before the wave's first row looks back, wave-uniformly and at most k rows. The lane at
//                a run's last row writes n. The padding (y = -1, w = 0, n = 0) is three fills in front of the kernel.
#include "common.h"
#include "../../include/otto_rows.h"

namespace otto {

constexpr int ROWS_THREADS = 256;
constexpr int ROWS_WAVES = ROWS_THREADS / WAVE;

static const char* rows_reason(int64_t r) {
    static const char* const names[] = {"no violation", "aid_x outside [0, n_aids)", "aid_y outside [0, n_aids)",
                                        "aid_x below the previous row's", "a run longer than k"};
    return r >= 0 && r <= OTTO_ROWS_E_RUN ? names[r] : "?";
}

__global__ __launch_bounds__(ROWS_THREADS) void k_rows_topk(const int32_t* __restrict__ aid_x, const int32_t* __restrict__ aid_y,
                                                            const float* __restrict__ wgt, int64_t n_rows, int64_t n_aids, int k,
                                                            int32_t* __restrict__ y, float* __restrict__ w, int32_t* __restrict__ n,
                                                            unsigned long long* err) {
    const int64_t r0 = ((int64_t)blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6)) * WAVE;
    if (r0 >= n_rows) return;                                // wave-uniform
    const int lane = (int)lane_id();
    const int64_t r = r0 + lane;
    const bool live = r < n_rows;
    const int32_t x = live ? aid_x[r] : 0, ay = live ? aid_y[r] : 0;
    const int32_t prev = live && r > 0 ? aid_x[r - 1] : -1;
    const bool head = live && (r == 0 || x != prev);
    const bool last = live && (r + 1 == n_rows || aid_x[r + 1] != x);
    const unsigned long long heads = __ballot(head);
    // rows of the wave's first aid in front of the wave: only looked for when the wave's first row is no head
    const int32_t x0 = __builtin_amdgcn_readfirstlane(x);
    int back = 0;
    if (!(heads & 1ull)) {
        while (back < k && r0 - 1 - back >= 0 && aid_x[r0 - 1 - back] == x0) ++back;      // back == k: the run is too long
    }
    const unsigned long long mine = heads & (~0ull >> (63 - lane));                       // the heads at or below this lane
    const int pos = mine ? lane - (63 - __builtin_clzll(mine)) : lane + back;
    if (!live) return;
    int bad = 0;
    if (x < 0 || x >= n_aids) bad = OTTO_ROWS_E_AID_X;
    else if (ay < 0 || ay >= n_aids) bad = OTTO_ROWS_E_AID_Y;
    else if (r > 0 && x < prev) bad = OTTO_ROWS_E_ORDER;
    else if (pos >= k) bad = OTTO_ROWS_E_RUN;
    if (bad) {
        atomicMin(err, (unsigned long long)r << 8 | (unsigned long long)bad);
        return;
    }
    y[(int64_t)x * k + pos] = ay;                            // 0 <= x < n_aids and pos < k here: the slot lies inside the outputs
    w[(int64_t)x * k + pos] = wgt[r];
    if (last) n[x] = pos + 1;
}

static int rows_check(const otto_rows_job* j) {
    OTTO_REQUIRE(j, "otto_rows: null job");
    OTTO_REQUIRE(j->n_rows >= 0 && j->n_rows < (1ll << 40), "otto_rows: n_rows must be in [0, 2^40) (got %lld)", (long long)j->n_rows);
    OTTO_REQUIRE(j->n_aids >= 0 && j->n_aids < (1ll << 31), "otto_rows: n_aids must be in [0, 2^31) (got %lld)", (long long)j->n_aids);
    OTTO_REQUIRE(j->k >= 1 && j->k <= OTTO_ROWS_MAX_K, "otto_rows: k must be in [1, %d] (got %d)", OTTO_ROWS_MAX_K, j->k);
    OTTO_REQUIRE(j->reserved == 0, "otto_rows: reserved must be 0");
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_rows_workspace(const otto_rows_job* job) {
    if (rows_check(job) != 0) return -22;
    return 256;                                              // the error word
}

extern "C" int otto_rows_topk(const otto_rows_job* job, int64_t* h_err) {
    OTTO_REQUIRE(h_err, "otto_rows_topk: null h_err");
    h_err[0] = -1;
    h_err[1] = 0;
    OTTO_TRY(rows_check(job));
    const otto_rows_job& j = *job;
    OTTO_REQUIRE(j.n_rows == 0 || (j.d_aid_x && j.d_aid_y && j.d_wgt), "otto_rows_topk: null input column");
    OTTO_REQUIRE(j.n_aids == 0 || (j.d_y && j.d_w && j.d_n), "otto_rows_topk: null output");
    OTTO_REQUIRE(j.n_aids > 0 || j.n_rows == 0 || j.d_work, "otto_rows_topk: null workspace");
    if (j.n_aids == 0 && j.n_rows == 0) return 0;
    OTTO_REQUIRE(j.d_work && j.work_bytes >= 256 && ((uintptr_t)j.d_work & 7) == 0, "otto_rows_topk: workspace of 256 aligned bytes needed");
    hipStream_t s = (hipStream_t)j.stream;
    unsigned long long* err = (unsigned long long*)j.d_work;
    OTTO_HIP(hipMemsetAsync(err, 0xFF, 8, s));
    if (j.n_aids > 0) {
        OTTO_HIP(hipMemsetAsync(j.d_y, 0xFF, (size_t)j.n_aids * j.k * 4, s));
        OTTO_HIP(hipMemsetAsync(j.d_w, 0, (size_t)j.n_aids * j.k * 4, s));
        OTTO_HIP(hipMemsetAsync(j.d_n, 0, (size_t)j.n_aids * 4, s));
    }
    if (j.n_rows > 0) {
        const int64_t waves = (j.n_rows + WAVE - 1) / WAVE;
        k_rows_topk<<<(unsigned)((waves + ROWS_WAVES - 1) / ROWS_WAVES), ROWS_THREADS, 0, s>>>(j.d_aid_x, j.d_aid_y, j.d_wgt, j.n_rows, j.n_aids,
                                                                                            j.k, j.d_y, j.d_w, j.d_n, err);
        OTTO_HIP(hipGetLastError());
    }
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != ~0ull) {
        h_err[0] = (int64_t)(herr >> 8);
        h_err[1] = (int64_t)(herr & 0xFF);
        OTTO_REQUIRE(false, "otto_rows_topk: row %lld: %s", (long long)h_err[0], rows_reason(h_err[1]));
    }
    return 0;
}
