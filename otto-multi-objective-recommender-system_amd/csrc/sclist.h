// Per-row sorted top-k lists shared by the MFMA scoring kernels (k_score in otto_mf.hip, k_knn in otto_knn.hip):
// the in-LDS insertion and the exact merge of partial lists. One wave lane per slot, so k <= 64 here; the callers
// set their own limits (otto_mf_score_topk keeps k <= 32).
#pragma once
#include "common.h"

#include <math.h>

namespace otto {

// insert (score, id) into the sorted (desc) k-list of one row in LDS; the whole wave cooperates.
// Returns the new k-th score (threshold).
__device__ __forceinline__ float list_insert(volatile float* ls, volatile int32_t* li, int k, float sc, int32_t id) {
    const unsigned l = lane_id();
    const float cur = l < (unsigned)k ? ls[l] : -INFINITY;
    // entries that stay ahead of the newcomer: higher score (ids arrive in ascending order, so on a
    // tie the resident entry has the smaller id and stays ahead)
    const bool ahead = l < (unsigned)k && cur >= sc;
    const int pos = __popcll(__ballot(ahead));
    const int32_t curi = l < (unsigned)k ? li[l] : 0;
    __builtin_amdgcn_wave_barrier();
    if ((int)l >= pos && (int)l + 1 < k) { ls[l + 1] = cur; li[l + 1] = curi; }
    if ((int)l == pos && pos < k) { ls[l] = sc; li[l] = id; }
    __builtin_amdgcn_wave_barrier();
    return ls[k - 1];
}

// merge the nsplit partial k-lists of one row ([nsplit][Bpad][k], id -1 or 0x7FFFFFFF = empty slot) in one wave:
// on return lane l < k holds the l-th entry by (score desc, id asc); an empty slot has id 0x7FFFFFFF, score -inf.
__device__ __forceinline__ void merge_row_lists(const float* part_s, const int32_t* part_i, int nsplit, int64_t Bpad,
                                                int64_t row, int k, float& bs, int32_t& bi) {
    const unsigned l = lane_id();
    bs = -INFINITY;
    bi = 0x7FFFFFFF;
    const int total = nsplit * k;
    for (int c0 = 0; c0 < total; c0 += 64) {
        const int c = c0 + (int)l;
        float cs = -INFINITY;
        int32_t ci = 0x7FFFFFFF;
        if (c < total) {
            const int64_t o = ((int64_t)(c / k) * Bpad + row) * k + (c % k);
            cs = part_s[o];
            ci = part_i[o];
            if (ci < 0) ci = 0x7FFFFFFF;          // -1: an empty slot of a gathered partial list
        }
        auto better = [](float s1, int32_t i1, float s2, int32_t i2) { return s1 > s2 || (s1 == s2 && i1 < i2); };
        float ts = __shfl(bs, k - 1, 64);
        int32_t ti = __shfl(bi, k - 1, 64);
        uint64_t m = __ballot(ci != 0x7FFFFFFF && better(cs, ci, ts, ti));
        while (m) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const float s = __shfl(cs, src, 64);
            const int32_t id = __shfl(ci, src, 64);
            const float us = __shfl_up(bs, 1, 64);
            const int32_t ui = __shfl_up(bi, 1, 64);
            if (better(s, id, bs, bi)) {
                if (l > 0 && better(s, id, us, ui)) { bs = us; bi = ui; }
                else { bs = s; bi = id; }
            }
            ts = __shfl(bs, k - 1, 64);
            ti = __shfl(bi, k - 1, 64);
            m &= m - 1;
            m &= __ballot(ci != 0x7FFFFFFF && better(cs, ci, ts, ti));
        }
    }
}

}  // namespace otto
