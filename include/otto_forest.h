/*
 * otto_forest.h -- C-ABI of the gradient-boosted forest scorer and the per-session top-k (SPEC-FOREST, DESIGN.md
 * section 3c).
 *
 * What this replaces in the reference: lgb.Booster.predict over every (session, candidate) row and the fold average
 * (src/ranker/lgb_trainer.py:181, 248-266), then "sort by (session, score desc), head(20)" (lgb_trainer.py:183-189,
 * src/ranker/inference.py:175-176, 245-246, 314-315).
 *
 * Conventions of otto_knn.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; all device work on
 * the caller's stream; no buffer is allocated per call (the error words live in a 256-byte per-device scratch the library
 * keeps, as the candidate entry points do). A device call synchronises the stream once to read its error words.
 * The functions without a stream parameter (otto_forest_packed_bytes, otto_forest_pack) work on host arrays alone and enqueue nothing.
 *
 * SPEC-FOREST. A forest is T trees over F features. Tree t has L_t >= 1 leaves and L_t - 1 internal nodes; an internal
 * node has split_feature, threshold (float64 in the model file), decision_type, left_child, right_child. A child c >= 0
 * is internal node c, c < 0 is leaf ~c, node 0 is the root; a tree with L_t == 1 has no nodes and its value is
 * leaf_value[0]. Routing of a float32 feature value x at a node (LightGBM's numerical decision), with
 * missing = (decision_type >> 2) & 3 (0 none, 1 zero, 2 NaN) and default_left = decision_type & 2:
 *     1. x is NaN and missing != 2:  x := 0
 *     2. (missing == 1 and |x| <= 1e-35f) or (missing == 2 and x is NaN):  left if default_left, else right
 *     3. otherwise:  left iff (double)x <= threshold
 * decision_type & 1 (categorical) and missing == 3 are refused.
 *
 * The device never compares in float64. otto_forest_pack replaces each threshold t by t32, the largest float32 <= t
 * (-inf if there is none, +inf stays +inf). For every non-NaN float32 x:  (double)x <= t  <=>  x <= t32.  (=>: (double)x
 * is itself a float32 value <= t, so it is <= the largest such value. <=: x <= t32 <= t.) Routing is therefore exact.
 *
 * Raw score of a row = sum over t = 0 .. T-1, in that order, in float64, of the reached leaf_value (shrinkage is already
 * inside leaf_value; no output transform). One lane adds the trees of one row sequentially.
 * Fold ensemble (lgb_trainer.py:248-261):  acc = 0.0;  for each forest:  acc += (double)(float)raw / n_forests
 * (a true division).
 *
 * Session top-k: rows of session s are [row_off[s], row_off[s+1]); ordered by (score descending, row position
 * ascending), the first k. NaN scores order after every number and among themselves by position; -0.0 and +0.0 tie.
 * A session with  not (0 <= row_off[s] <= row_off[s+1] <= n_rows)  or with 2^32 rows or more is detected on the device:
 * it comes back empty and the call returns OTTO_EINVAL after the stream has drained.
 *
 * Packed image (host byte order, every section 16-byte aligned; all offsets in bytes from the start of the image):
 *     header  64 bytes   u32 magic 'OFR1' (0x3152464F), u32 version 1, i32 T, i32 F, i32 n_groups, i32 max_leaves,
 *                        i32 total_nodes, i32 total_leaves, i64 total_bytes, i64 off_trees, i64 off_groups, i64 off_blob
 *     trees   T x 8      { u32 off16, i32 n_leaves }: the tree's blob starts at off_blob + 16 * off16
 *     groups  n x 16     { i32 first_tree, i32 n_trees, u32 off16, u32 len16 }: consecutive whole trees that are staged
 *                        through LDS together (16 * len16 <= OTTO_FOREST_GROUP_BYTES); len16 == 0: one tree larger than
 *                        that, walked from global memory
 *     blob    per tree   (L-1) nodes x 16 bytes { f32 t32, u32 feature | missing << 16 | default_left << 18,
 *                        i32 left_child, i32 right_child }, then L leaf values x f64, padded to 16 bytes
 * total_bytes == otto_forest_packed_bytes(T, total_nodes, total_leaves); the tail behind the last tree is zero.
 * The image holds t32, not the float64 threshold.
 *
 * Every tree walk on the device is bounded by L_t - 1 steps and every child and leaf index is range-checked, so an
 * image damaged after packing cannot hang the device or index outside its tree: the call returns OTTO_EINVAL.
 */
#ifndef OTTO_FOREST_H
#define OTTO_FOREST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_FOREST_MAX_LEAVES 2048
#define OTTO_FOREST_MAX_FEATURES 128
#define OTTO_FOREST_MAX_K 64
#define OTTO_FOREST_GROUP_BYTES 24576 /* 8 trees of 128 leaves (8 x 3056 bytes); one tree of up to 1024 leaves */

/* bytes of the packed image; 0 for arguments the pack would refuse */
int64_t otto_forest_packed_bytes(int32_t T, int64_t total_nodes, int64_t total_leaves);

/* HOST pointers throughout. node_off, leaf_off int64 [T+1]: tree t owns nodes [node_off[t], node_off[t+1]) and leaves
 * [leaf_off[t], leaf_off[t+1]), with n_nodes == n_leaves - 1. Validates the structure (children in range, every
 * internal node and every leaf reached exactly once from the root, split_feature < F, finite leaf values, no NaN
 * threshold, no categorical bit, L_t <= OTTO_FOREST_MAX_LEAVES, 1 <= F <= OTTO_FOREST_MAX_FEATURES) and writes the image
 * into out (out_bytes >= otto_forest_packed_bytes(...)). */
int otto_forest_pack(int32_t T, int32_t F, const int64_t* node_off, const int64_t* leaf_off, const int32_t* split_feature,
                     const double* threshold, const int8_t* decision_type, const int32_t* left_child,
                     const int32_t* right_child, const double* leaf_value, void* out, int64_t out_bytes);

/* d_X float32 row-major, row stride ld >= F; d_raw float64 [n_rows] or NULL: the raw score; d_acc float64 [n_rows] or
 * NULL: d_acc[r] += (double)(float)raw / divisor. n_rows == 0 is a no-op that returns 0. */
int otto_forest_predict(const void* d_packed, int64_t packed_bytes, const float* d_X, int64_t ld, int64_t n_rows, int32_t F,
                        double* d_raw, double* d_acc, double divisor, void* stream);

/* the reached leaf of every (row, tree): d_leaf int32 [n_rows, T] row-major (LightGBM's pred_leaf) */
int otto_forest_leaves(const void* d_packed, int64_t packed_bytes, const float* d_X, int64_t ld, int64_t n_rows, int32_t F,
                       int32_t T, int32_t* d_leaf, void* stream);

/* d_score float64 [n_rows], d_aid int32 [n_rows], d_row_off int64 [S+1]; 1 <= k <= OTTO_FOREST_MAX_K.
 * d_top_aid int32 [S, k] (-1 padded), d_top_score float64 [S, k] (-inf padded), d_n int32 [S]. */
int otto_forest_session_topk(const double* d_score, const int32_t* d_aid, const int64_t* d_row_off, int64_t S, int64_t n_rows,
                             int32_t k, int32_t* d_top_aid, double* d_top_score, int32_t* d_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
