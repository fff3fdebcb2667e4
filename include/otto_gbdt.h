/*
 * otto_gbdt.h -- C-ABI of the LambdaRank gradient-boosted tree trainer (SPEC-GBDT).
 *
 * What this replaces in the reference: lgb.train over the (session, candidate) matrix, one model per event type and
 * fold (src/ranker/lgb_trainer.py:134-165). LightGBM's arithmetic is third-party; the trainer is specified here, after
 * LightGBM's published LambdarankNDCG objective and leaf-wise histogram algorithm, with the parameter values recorded in
 * the reference's model dump. The result is a forest that include/otto_forest.h scores.
 *
 * Conventions of otto_forest.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; all device
 * work on the caller's stream; no buffer is allocated per call (otto_gbdt_workspace_bytes sizes d_work; the error words
 * live in a per-device scratch the library keeps). A call that can detect an error on the device synchronises the
 * stream once to read its error words.
 * The functions without a stream parameter (the two *_workspace_bytes sizes) run on the host and enqueue nothing.
 *
 * SPEC-GBDT.
 * Inputs. X float32 [n, >= F] row-major, 1 <= F <= OTTO_FOREST_MAX_FEATURES; label int32 [n] in 0..31 (gain =
 * 2^label - 1); query_off int64 [Q+1], the rows of a query contiguous; n < 2^31; a query holds at most
 * OTTO_GBDT_MAX_QUERY rows. A query with  not (0 <= query_off[q] <= query_off[q+1] <= n)  or with more rows is detected
 * on the device: its outputs are zero (AP: -1) and the call returns OTTO_EINVAL after the stream has drained.
 *
 * Binning. Per feature at most OTTO_GBDT_MAX_EDGES float32 edges, strictly increasing, made on the host. bin(x) = the
 * number of edges < x, so  bin(x) <= b  <=>  x <= edge[b];  NaN -> bin OTTO_GBDT_NAN_BIN (255, reserved). Bins are
 * uint8 [F, n], feature-major. A model threshold is an edge itself: a float32 is exact as float64 and is its own t32
 * (otto_forest.h), so the forest scorer routes every training row exactly as the trainer partitioned it.
 *
 * Objective (LambdarankNDCG). Per query the rows are ordered by (score descending, position ascending; -0.0 == +0.0).
 * The host supplies discount[r] = 1/log2(2+r), r < OTTO_GBDT_MAX_QUERY, and a sigmoid table of
 * OTTO_GBDT_SIGMOID_BINS entries over [lo, hi] = [-25/sigma, 25/sigma]: entry i = 1/(1+exp(sigma*(lo + i/factor))),
 * factor = OTTO_GBDT_SIGMOID_BINS/(hi-lo); lookup table[(size_t)min(max((d-lo)*factor, 0), OTTO_GBDT_SIGMOID_BINS-1)].
 * inv_max_dcg = 1 / sum_{r<T} gain(labels sorted descending)[r]*discount[r] (T = truncation_level; 0 if the sum is 0),
 * summed in rank order. best / worst = the first / last sorted score. For ranks i < min(T, cnt), j > i, labels differ,
 * high / low by label:
 *     d = s_high - s_low;  delta = (gain_high - gain_low) * |discount[i] - discount[j]| * inv_max_dcg;
 *     if norm and best != worst:  delta /= (0.01 + |d|);
 *     p = sigmoid(d);  lambda = -sigma*delta*p;  eta = sigma*sigma*delta*p*(1-p)      (products left to right)
 *     grad[high] += lambda;  grad[low] -= lambda;  hess[both] += eta
 * A row adds its pairs in ascending rank of the partner (the order of the sequential double loop), in float64 without
 * contraction. If norm: S = sum over pairs of -2*lambda; if S > 0 every grad and hess of the query is multiplied by
 * log2(1+S)/S. The summation order of S and the device log2 are NOT pinned: with norm the result is not bit-exact.
 *
 * Quantisation. mg = max|grad|, mh = max hess (exact max reductions). For a maximum m*2^x, m in [0.5, 1):
 * e = 30 - x, q = (int32) rint(v * 2^e) (half to even); a maximum of 0 gives e = 0 and q = 0. d_gh holds (qg, qh) per
 * row. Every histogram sum is an int64 sum of q plus an int64 row count: independent of order and of the number of
 * workgroups, and  larger child = parent - smaller child  is exact.
 *
 * Histogram of a leaf: int64 [3, F, 256] = planes (sum qg, sum qh, rows), by feature, by bin.
 *
 * Split search. For sums (Gq, Hq, cnt): G = ldexp((double)Gq, -e_g), H = ldexp((double)Hq, -e_h). For feature f, edge
 * b < n_edges[f], two variants: NaN rows right / NaN rows left. left = bins <= b (+ bin 255 if NaN-left), right =
 * parent - left in integers. Admissible iff cnt_L, cnt_R >= min_data_in_leaf and H_L, H_R >= min_sum_hessian_in_leaf.
 *     gain = (G_L*G_L/(H_L+l2) + G_R*G_R/(H_R+l2)) - G_P*G_P/(H_P+l2)      float64, in that order
 * A split needs gain > min_gain_to_split. Best = largest gain; ties: smallest f, then smallest b, then NaN-right.
 * d_split int64 [OTTO_GBDT_SPLIT_WORDS] = { found, feature, bin, default_left, gain bits, cnt_L, Gq_L, Hq_L, cnt_P,
 * Gq_P, Hq_P, 0 }; the parent sums are those of the histogram (all 256 bins of feature 0).
 *
 * Growth, leaf-wise. Step s splits the leaf with the largest best gain (ties: smallest leaf index) into internal node
 * s; the left child keeps the leaf's index, the right child is leaf s+1; the parent's child pointer becomes s. Stops
 * at num_leaves or when no leaf has a split. threshold = (double)edge[f][b]; decision_type = (2 << 2) |
 * (default_left ? 2 : 0); leaf_value = -(G/(H+l2))*learning_rate. The row partition is stable.
 *
 * AP@k of a query, in the same order: sum_{r<k, label_r>0} hits_through_r/(r+1) / min(n_pos, k), float64 in rank
 * order; -1 for a query without a positive.
 *
 * Sampling (stochastic gradient boosting as LightGBM v3 defines it: bagging_fraction, bagging_freq, feature_fraction).
 * The draws come from a pinned counter-based sampler, not from LightGBM's RNG: the counts, the redraw schedule and the
 * determinism are LightGBM's, the sets are not.
 *     mix(s, i):  z = s + (i + 1) * 0x9E3779B97F4A7C15      (mod 2^64)
 *                 z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *                 z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *                 return z ^ (z >> 31)
 * (the row key of otto_folds.h; a bijection in i for a fixed s).
 * Row bag. Active iff bagging_freq = k > 0 and bagging_fraction = p < 1 (bagging_freq = 0: no bagging). At a 0-based
 * iteration it with it % k == 0 a new bag is drawn with draw index d = it / k, otherwise the previous bag is kept.
 * m = int(p * n): the float64 product, truncated (LightGBM's bag_data_cnt); m >= 1 is required, the host refuses
 * anything else before a launch. key(r) = mix(mix(bagging_seed, 2*d), r), r in [0, n): distinct rows have distinct
 * keys. The bag is the m rows with the smallest keys, as an ascending int32 row list: it depends on no grid, workgroup
 * size or order of atomics. The objective and the quantisation run over all n rows, unchanged. The tree is grown on
 * the bag only: the root's row list is the bag; every histogram sum, every count, min_data_in_leaf,
 * min_sum_hessian_in_leaf, leaf_value and leaf_count are over in-bag rows; hist_rows counts in-bag rows. After the
 * tree, score[r] += leaf_value[leaf(r)] for every row, out-of-bag rows included (otto_gbdt_add_tree routes all rows).
 * Feature sample. Active iff feature_fraction = q < 1; drawn for every tree, over all F features (one without an edge
 * counts too). n_used = max(min(2, F), floor(F*q + 0.5)). fkey(f) = mix(mix(feature_fraction_seed, 2*it + 1), f). The
 * tree of iteration it may split only on the n_used features with the smallest keys, kept as an ascending int32 list
 * (made on the host: F <= 128). The tie order of the split search ("smallest f") is over the listed features; the
 * parent sums of d_split are those of the FIRST LISTED feature, not of feature 0; the histogram planes of the other
 * features are zero.
 * Seeds. bagging_seed defaults to 3, feature_fraction_seed to 2 (LightGBM's defaults). `seed` is ignored: LightGBM
 * would derive the two seeds from it, and that derivation is not reproduced.
 * Objectives and metrics beyond these (the `binary` objective, NDCG, AUC, logloss): SPEC-OBJ, include/otto_objective.h.
 * Refused: an objective other than lambdarank / binary, a metric other than map / ndcg / auc / binary_logloss, is_unbalance
 * together with scale_pos_weight != 1, feature_fraction_bynode < 1, pos_bagging_fraction / neg_bagging_fraction != 1, bagging_fraction or
 * feature_fraction outside (0, 1], bagging_freq < 0.
 */
#ifndef OTTO_GBDT_H
#define OTTO_GBDT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_GBDT_MAX_QUERY 1024      /* rows of one query: one workgroup ranks a query in LDS */
#define OTTO_GBDT_MAX_EDGES 254
#define OTTO_GBDT_NAN_BIN 255
#define OTTO_GBDT_SIGMOID_BINS 1048576
#define OTTO_GBDT_MAX_LABEL 31
#define OTTO_GBDT_SPLIT_WORDS 12

/* bytes of d_work for otto_gbdt_grow_tree (and enough for otto_gbdt_partition); 0 for refused arguments */
int64_t otto_gbdt_workspace_bytes(int64_t n, int32_t F, int32_t num_leaves);

/* d_X float32, row stride ld >= F; d_edges float32 [F, OTTO_GBDT_MAX_EDGES] (row f: n_edges[f] edges, rest ignored);
 * d_n_edges int32 [F]; d_bins uint8 [F, n]. */
int otto_gbdt_bin(const float* d_X, int64_t ld, int64_t n, int32_t F, const float* d_edges, const int32_t* d_n_edges,
                  uint8_t* d_bins, void* stream);

/* d_sigmoid float64 [OTTO_GBDT_SIGMOID_BINS], d_discount float64 [OTTO_GBDT_MAX_QUERY]; d_grad, d_hess float64 [n]. */
int otto_gbdt_lambdarank(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                         const double* d_sigmoid, double sigmoid_lo, double sigmoid_factor, const double* d_discount,
                         double sigma, int32_t truncation_level, int32_t norm, double* d_grad, double* d_hess, void* stream);

/* d_gh int32 [n, 2] = (qg, qh); d_exp int32 [2] = (e_g, e_h) */
int otto_gbdt_quantize(const double* d_grad, const double* d_hess, int64_t n, int32_t* d_gh, int32_t* d_exp, void* stream);

/* d_rows int32 [n_rows]: the leaf's rows (an entry outside [0, n) is skipped and the call returns OTTO_EINVAL);
 * d_hist int64 [3, F, 256], overwritten.
 * The feature list, here and wherever d_features / n_used appear: d_features int32 [n_used] on the device, strictly
 * ascending inside [0, F), 1 <= n_used <= F (copied to the host and checked there: one synchronisation; OTTO_EINVAL
 * otherwise); d_features == NULL (n_used ignored): every feature. The histogram fills the listed features' planes and
 * leaves the others zero; the split search walks the listed features only and takes the parent sums from the first of
 * them. */
int otto_gbdt_hist(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_rows, int64_t n_rows,
                   const int32_t* d_features, int32_t n_used, int64_t* d_hist, void* stream);
int otto_gbdt_best_split(const int64_t* d_hist, int32_t F, const int32_t* d_n_edges, const int32_t* d_exp,
                         int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double lambda_l2, double min_gain_to_split,
                         const int32_t* d_features, int32_t n_used, int64_t* d_split, void* stream);

/* The row bag: d_rows_out int32 receives, ascending, the m rows of [0, n) with the smallest mix(seed, r); seed is the
 * already mixed mix(bagging_seed, 2*d). 1 <= m <= n < 2^31. out_rows: the row ids d_rows_out has room for; out_rows < m
 * or a d_work below otto_gbdt_bag_workspace_bytes(n) (0 for a refused n) returns OTTO_EINVAL before anything is launched.
 * The device checks once more that exactly m rows pass and writes nothing at or behind d_rows_out[out_rows]. */
int64_t otto_gbdt_bag_workspace_bytes(int64_t n);
int otto_gbdt_bag(int64_t n, int64_t m, uint64_t seed, int32_t* d_rows_out, int64_t out_rows, void* d_work, int64_t work_bytes,
                  void* stream);

/* d_out int32 [n_rows]: the rows that go left (bin <= bin, or bin 255 when default_left) in their order, then the
 * others in theirs; d_n_left int64 [1]. d_out must not overlap d_rows. */
int otto_gbdt_partition(const uint8_t* d_bins, int64_t n, int32_t feature, int32_t bin, int32_t default_left,
                        const int32_t* d_rows, int64_t n_rows, int32_t* d_out, int64_t* d_n_left, void* d_work,
                        int64_t work_bytes, void* stream);

/* One tree in bin space, device arrays: n_leaves - 1 nodes (split_feature, split_bin, default_left, left_child,
 * right_child; children as in otto_forest.h) and n_leaves values. d_score[r] += leaf_value[leaf(r)]; d_leaf int32 [n]
 * or NULL receives leaf(r). Walks are bounded and range-checked: a damaged tree returns OTTO_EINVAL. */
int otto_gbdt_add_tree(const uint8_t* d_bins, int64_t n, int32_t F, int32_t n_leaves, const int32_t* d_split_feature,
                       const int32_t* d_split_bin, const int32_t* d_default_left, const int32_t* d_left_child,
                       const int32_t* d_right_child, const double* d_leaf_value, double* d_score, int32_t* d_leaf,
                       void* stream);

/* d_ap float64 [Q]; 1 <= k <= OTTO_GBDT_MAX_QUERY */
int otto_gbdt_ap_at_k(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                      int32_t k, double* d_ap, void* stream);

/* One whole tree. h_* are HOST buffers: h_edges float32 [F, OTTO_GBDT_MAX_EDGES]; node arrays of num_leaves - 1
 * entries, leaf arrays of num_leaves; *h_n_leaves the leaves grown (1: no split was admissible, only h_leaf_value[0] and
 * h_leaf_count[0] are written); h_hist_rows int64 [1] or NULL: rows the histogram kernel read.
 * The row bag (SPEC-GBDT, Sampling): d_bag int32 [n_bag] on the device, 1 <= n_bag <= n, is the root's row list;
 * d_bag == NULL (n_bag ignored): all n rows. Only the range of its entries is checked (one outside [0, n) is skipped and
 * the call returns OTTO_EINVAL, as for d_rows). That the ids ascend and that none occurs twice is the caller's
 * responsibility, as it is for d_rows of otto_gbdt_hist: otto_gbdt_bag writes such a list; a row listed twice is counted
 * twice, and an order other than ascending only costs the histogram its coalesced loads. With a bag, h_leaf_count and
 * *h_hist_rows count in-bag rows. d_features / n_used: the feature list, as for otto_gbdt_hist. */
int otto_gbdt_grow_tree(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_exp,
                        const int32_t* d_n_edges, const float* h_edges, int32_t num_leaves, int64_t min_data_in_leaf,
                        double min_sum_hessian_in_leaf, double lambda_l2, double min_gain_to_split, double learning_rate,
                        const int32_t* d_bag, int64_t n_bag, const int32_t* d_features, int32_t n_used,
                        int32_t* h_n_leaves, int32_t* h_split_feature, int32_t* h_split_bin, double* h_threshold,
                        int8_t* h_decision_type, int32_t* h_left_child, int32_t* h_right_child, double* h_split_gain,
                        double* h_leaf_value, int64_t* h_leaf_count, int64_t* h_hist_rows, void* d_work, int64_t work_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
