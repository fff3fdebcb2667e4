// Keyed radix select, shared by the row bag of the LambdaRank trainer and the negative sampler of the fold trainer: every
// row r has the key row_key(seed, r); device_select leaves the m-th smallest key among the eligible rows on the device.
// 8 digits of 8 bits from the top. A pass recomputes the keys from the row indices (no key array is stored) and counts the
// digit of the keys that carry the prefix found so far; one wave then picks the digit that holds the wanted rank.
#pragma once
#include "common.h"

namespace otto {

constexpr int SELECT_BLOCKS = 1024;                     // grid cap of the histogram kernel (4 waves per workgroup)
// workspace of a select: hist, then sel; a layout embeds both behind a 256-byte boundary
constexpr int64_t SELECT_HIST_BYTES = 8 * 256 * 4;      // one 256-bin histogram per pass
constexpr int64_t SELECT_SEL_BYTES = 256;               // { prefix, k } and padding
static_assert(SELECT_HIST_BYTES % 256 == 0 && SELECT_SEL_BYTES % 256 == 0, "the pieces keep a layout's 256-byte alignment");

// sel = { prefix: the digits found so far, k: the rank (1-based) still wanted among the keys that carry the prefix }
// Rows: operator()(int64_t i, F count) calls count(r) for every eligible row r of item i; the items [0, items) cover the
// rows once. Wave-private LDS histograms, merged once per workgroup; one integer global atomic per touched bin.
template <typename Rows>
__global__ __launch_bounds__(256) void k_select_hist(Rows rows, int64_t items, uint64_t seed, const uint64_t* sel, int pass,
                                                     uint32_t* hist) {
    __shared__ uint32_t h[4][256];
    for (int i = threadIdx.x; i < 4 * 256; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    const uint64_t prefix = pass == 0 ? 0ull : sel[0];
    const int shift = 56 - 8 * pass;
    uint32_t* mine = h[threadIdx.x >> 6];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        rows(i, [&](int64_t r) {
            const uint64_t key = row_key(seed, (uint64_t)r);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&mine[(key >> shift) & 255u], 1u);
        });
    }
    __syncthreads();
    const uint32_t t = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
    if (t) atomicAdd(hist + threadIdx.x, t);
}

static __global__ __launch_bounds__(64) void k_select_pick(const uint32_t* hist, uint64_t* sel, int pass, uint64_t m) {
    __shared__ uint32_t sm[256];
    for (int i = threadIdx.x; i < 256; i += 64) sm[i] = hist[i];
    wave_lds_sync();
    if (threadIdx.x == 0) {
        const uint64_t prefix = pass == 0 ? 0ull : sel[0];
        uint64_t k = pass == 0 ? m : sel[1];
        int d = 0;
        for (; d < 255; ++d) {                         // the last digit takes what is left: no index past the table
            if (sm[d] >= k) break;
            k -= sm[d];
        }
        sel[0] = (prefix << 8) | (uint64_t)d;
        sel[1] = k;
    }
}

// sel[0] = the m-th smallest key (1 <= m <= eligible rows) among the rows of `rows`, on the stream: no copy, no wait
template <typename Rows>
static int device_select(Rows rows, int64_t items, int64_t m, uint64_t seed, uint32_t* hist, uint64_t* sel, hipStream_t s) {
    OTTO_HIP(hipMemsetAsync(hist, 0, SELECT_HIST_BYTES, s));
    const unsigned grid = (unsigned)((items + 255) / 256 < SELECT_BLOCKS ? (items + 255) / 256 : SELECT_BLOCKS);
    for (int pass = 0; pass < 8; ++pass) {
        k_select_hist<Rows><<<grid, 256, 0, s>>>(rows, items, seed, sel, pass, hist + pass * 256);
        OTTO_HIP(hipGetLastError());
        k_select_pick<<<1, 64, 0, s>>>(hist + pass * 256, sel, pass, (uint64_t)m);
        OTTO_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace otto
