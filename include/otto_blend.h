/*
 * otto_blend.h -- C-ABI of the robust scaling and the outer-join blend of ranker scores (SPEC-BLEND, DESIGN.md
 * section 3d).
 *
 * What this replaces in the reference: src/ranker/inference.py -- read_predictions (:14-55: RobustScaler().fit_transform
 * on the concatenated score column of one model family, cast to Float32), the left / outer / outer join of the
 * families on (session, aid) with nulls filled by 0 (:160-163, :227-231, :297-301), the weighted sum (:167-176) and,
 * through otto_forest_session_topk, "sort by (session, predictions desc), head(20)".
 *
 * Conventions of otto_forest.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; the caller
 * supplies the workspace, sized by the *_workspace function; no allocation per call (the error words and the counts
 * live in a 256-byte per-device scratch the library keeps); all device work on the caller's stream; a call
 * synchronises the stream at most once (otto_blend_scale: never).
 * The functions without a stream parameter (the two *_workspace sizes) run on the host and enqueue nothing.
 *
 * SPEC-BLEND.
 *
 * Robust statistics of one score column x[n], float64. NaN entries are ignored for the statistics and stay NaN in the
 * output (scikit-learn's behaviour). Any +-inf, n == 0 or an all-NaN column is refused with OTTO_EINVAL (scikit-learn
 * raises on inf). Let v be the nv non-NaN values in ascending order, -0.0 and +0.0 equal. All ranks are integers:
 *     median = v[nv>>1] for odd nv, else (v[(nv-1)>>1] + v[nv>>1]) / 2
 *     25th / 75th percentile:  p = num * (nv - 1) with num = 1 / 3,  lo = p >> 2,  hi = min(lo + 1, nv - 1),
 *                              t = (p & 3) / 4
 *     value = NumPy's linear interpolation of a = v[lo], b = v[hi] at t:  a + (b - a) * t,  replaced by
 *             b - (b - a) * (1 - t) when t >= 0.5,  replaced by a when b == a
 *     center = median;  scale = q75 - q25, replaced by 1.0 when scale < 10 * DBL_EPSILON
 *     scaled[i] = (float)((x[i] - center) / scale)      two float64 operations and one rounding
 * The device selects only nv and the six order statistics (otto_blend_robust_stats); the interpolation is a handful
 * of float64 scalar operations the caller does on the host; otto_blend_scale applies center and scale.
 * h_stats order: v[(nv-1)>>1], v[nv>>1], then v[lo], v[hi] of the 25th and v[lo], v[hi] of the 75th percentile.
 * A selected zero comes back as +0.0 whatever signs the tied zeros carried.
 *
 * Join. M <= OTTO_BLEND_MAX_MODELS models; model m supplies n_m >= 0 rows (session int32 >= 0, aid int32 >= 0, scaled
 * float32); the total row count is < 2^31. A negative id is refused with OTTO_EINVAL. A (session, aid) that occurs
 * twice within one model is refused with OTTO_EINVAL, detected on the device (the reference's join would multiply
 * such rows). Model 0 is the base and always outer. Every other model carries a flag left_of_base: a flagged model
 * creates no output row and contributes only at keys model 0 has. The output holds one row for each distinct key of
 * the un-flagged models, in ascending (session, aid) order, and the CSR of its sessions.
 *
 * Prediction.  p = ((s_0 * w_0 + s_1 * w_1) + s_2 * w_2) + ...  in the caller's model order; an absent model
 * contributes s_m = 0.0f (its product is still added); w_m = (float)weight_m; every product and every sum is rounded
 * to float32 separately -- no fused multiply-add (contraction is switched off for the kernel that computes p; HIP's
 * __fmul_rn / __fadd_rn are plain operators that hipcc would fuse). This is a CHOICE, not a pin: polars, which
 * evaluates the reference's expression, is not available to compare against. Had it evaluated in Float64 the
 * difference is a few float32 ulps and matters only at near-ties.
 *
 * Selection. Per session by (p descending, aid ascending), NaN last, -0.0 and +0.0 tie, the first k <= 64: the
 * existing otto_forest_session_topk over d_out_pred64 = (double)p, d_out_aid and d_out_row_off -- the joined rows are
 * in aid order, so its "row position ascending" is "aid ascending".
 */
#ifndef OTTO_BLEND_H
#define OTTO_BLEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_BLEND_MAX_MODELS 8

/* bytes of workspace otto_blend_robust_stats needs (independent of n today; n is part of the contract) */
int64_t otto_blend_select_workspace(int64_t n);

/* d_x float64 [n] (read only). *h_nv = number of non-NaN entries, h_stats[6] as above (host pointers).
 * OTTO_EINVAL for n <= 0, an all-NaN column or any +-inf. Synchronises the stream once. */
int otto_blend_robust_stats(const double* d_x, int64_t n, int64_t* h_nv, double* h_stats, void* d_workspace,
                            int64_t workspace_bytes, void* stream);

/* d_out[i] = (float)((d_x[i] - center) / scale). No synchronisation. */
int otto_blend_scale(const double* d_x, int64_t n, double center, double scale, float* d_out, void* stream);

/* bytes of workspace otto_blend_join needs for n_total rows over M models */
int64_t otto_blend_join_workspace(int64_t n_total, int32_t M);

/* HOST arrays of length M: d_session / d_aid / d_score (device pointers int32 / int32 / float32 [n[m]], may be NULL
 * where n[m] == 0), n, weight, left_of_base (left_of_base[0] must be 0).
 * Outputs, device, every one with capacity for n_total = sum n[m] rows (d_out_row_off: n_total + 1):
 *   d_out_session_id int32   the distinct sessions, ascending (first *h_n_sessions valid)
 *   d_out_row_off    int64   CSR: rows of session j are [row_off[j], row_off[j+1])  (first *h_n_sessions + 1 valid)
 *   d_out_aid        int32,  d_out_pred float32,  d_out_pred64 float64 or NULL: (double)pred  (first *h_n_out valid)
 * OTTO_EINVAL (outputs undefined) for a negative id or a key twice in one model. Synchronises the stream once. */
int otto_blend_join(int32_t M, const int32_t* const* d_session, const int32_t* const* d_aid, const float* const* d_score,
                    const int64_t* n, const double* weight, const int32_t* left_of_base, int32_t* d_out_session_id,
                    int64_t* d_out_row_off, int32_t* d_out_aid, float* d_out_pred, double* d_out_pred64, int64_t* h_n_out,
                    int64_t* h_n_sessions, void* d_workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
