/*
 * otto_xgb.h -- C-ABI of the XGBoost-style ranker family: the rank:pairwise objective and depth-wise tree growth
 * (SPEC-XGB). Builds on include/otto_gbdt.h.
 *
 * What this replaces in the reference: xgb.train over the (session, candidate) matrix, one model per event type and fold
 * (src/ranker/xgb_trainer.py:134-165, xgboost==1.7.2), whose scores enter the final blend as the gunes_xgboost_* columns
 * (src/ranker/inference.py:64-85, 142-176). The reference keeps no xgboost config: the parameter values are XGBoost
 * 1.7's documented defaults. XGBoost's arithmetic is third-party and the library is not available to this project: the
 * trainer is specified here, after XGBoost's published LambdaRankObj / pairwise weight computer and its `hist` tree
 * method, and pinned by a NumPy restatement (tests/xgb_restatement.py). Parity with a run of xgboost itself is neither
 * claimed nor tested.
 *
 * Conventions of otto_gbdt.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; all device work on
 * the caller's stream; no buffer is allocated per call (otto_xgb_workspace_bytes sizes d_work; the error words live in
 * the per-device scratch the GBDT family keeps, so calls of the two families on one device must not overlap).
 * otto_xgb_workspace_bytes, the one function without a stream parameter, runs on the host and enqueues nothing.
 *
 * SPEC-XGB. Normative; everything not restated here is SPEC-GBDT's (otto_gbdt.h).
 *
 * Inputs. Binning and quantisation are SPEC-GBDT's: bins uint8 [F, n] with  bin(x) <= b  <=>  x <= edge[b]  and NaN ->
 * bin 255, the edges made by the host (XGBoost's quantile sketch is NOT reproduced); (qg, qh) int32 per row with the
 * exponents (e_g, e_h). max_bin defaults to 255; XGBoost's default of 256 is accepted and treated as 255; anything
 * larger is refused. label int32 [n] in 0..31; a query holds at most OTTO_GBDT_MAX_QUERY rows; a bad query or label is
 * detected on the device and reported as in SPEC-GBDT (outputs of a bad query zero, OTTO_EINVAL after the stream has
 * drained).
 *
 * Objective: rank:pairwise, after LambdaRankObj with the pairwise weight computer of XGBoost 1.7 at num_pairsample = 1.
 * Per query of cnt rows:
 *   Rank.   The rows are ranked by (score descending, position ascending; -0.0 == +0.0; NaN last): SPEC-GBDT's order.
 *   Record order.  rec = the ranked rows ordered by (label descending, rank ascending). A maximal run of equal labels
 *           is a bucket. For a row in the bucket [i, j) of rec: nleft = i (rows with a higher label), nright = cnt - j
 *           (rows with a lower label), m = nleft + nright. m == 0 (every label of the query the same): no draw.
 *   Draw.   For every rec position pid, ascending:  u = mix(mix(objective_seed, it), row) mod m  (mix: SPEC-GBDT's; it:
 *           the 0-based iteration; row: the row's index in [0, n); mod: the unsigned 64-bit remainder).
 *           u < nleft:  the pair is (high = rec[u], low = this row); otherwise (high = this row, low = rec[u + (j - i)]).
 *           The pair's index is pid.
 *   Pair terms.  d = s_low - s_high;  x = (d - lo) * factor;  x = x > 0 ? x : 0 (NaN -> 0);  x = min(x, BINS - 1);
 *           p = T[(size_t)x], T = SPEC-GBDT's sigmoid table at sigma = 1 (entry x = 1/(1+exp(x)), so p = sigmoid(s_high -
 *           s_low));  g = p - 1.0;  h = max(p * (1.0 - p), 1e-16);  h2 = 2.0 * h.
 *           grad[high] += g;  grad[low] -= g;  hess[high] += h2;  hess[low] += h2.
 *   Summation order.  float64 without contraction; each row starts from 0.0 and adds the terms of the pairs it takes
 *           part in, in ascending pair index (its own draw sits at its own pid).
 * The draws are not XGBoost's (its RNG is not reproduced); the pair counts, the bucket rule and the gradient expressions
 * are. A query without two different labels gets zeros.
 *
 * Split search: SPEC-GBDT's, with min_data_in_leaf = 0, min_sum_hessian_in_leaf = min_child_weight (default 1),
 * lambda_l2 = lambda (default 1), min_gain_to_split = gamma (default 0; a split needs gain > gamma), the same tie rule.
 *
 * Growth: depth-wise to max_depth (default 6, allowed [1, OTTO_XGB_MAX_DEPTH] = at most 1024 leaves, one forest group).
 * Level d holds the live leaves at depth d. Every live leaf of the level that has an admissible split is split, in
 * ascending node id. Node ids are XGBoost's: root 0, a split gives left = n_nodes, right = n_nodes + 1. Growth stops at
 * max_depth or when a level splits nothing. The BinTree follows SPEC-GBDT's numbering applied in that split order: step s
 * makes internal node s, the left child keeps the leaf's index, the right child is leaf s + 1.
 *     leaf_value = (double)(float)(-(G / (H + lambda)) * eta)          eta default 0.3
 * (rounded to float32 because XGBoost stores float32 weights; scores still accumulate in float64 through
 * otto_gbdt_add_tree). threshold = the edge itself, decision_type as in SPEC-GBDT. Per internal node also cover = H_P and
 * count = cnt_P, from the parent words of the split record, and the XGBoost ids of both children.
 *
 * Sampling. subsample < 1 -> SPEC-GBDT's row bag, redrawn every iteration (bagging_freq = 1): a bag of exactly
 * int(p * n) rows, NOT XGBoost's Bernoulli draw. colsample_bytree < 1 -> SPEC-GBDT's feature list with its n_used rule.
 * One XGBoost `seed` (default 0): objective_seed = mix(seed, 1), bagging_seed = mix(seed, 2), feature_fraction_seed =
 * mix(seed, 3).
 *
 * Initial score. base_score (default 0.5). The score of a row at an iteration, in training, validation and prediction, is
 * base_score + margin in float64, where margin adds the leaf values of the trees so far in tree order starting from 0.0:
 * the scorer of otto_forest.h over the float32 matrix returns the trainer's own bits.
 *
 * Metric: map. Per query SPEC-GBDT's AP at k = OTTO_GBDT_MAX_QUERY (divided by all positives); a query without a
 * positive counts 1.0 (with `map-`: 0.0); the mean over all queries, float64 on the host over otto_gbdt_ap_at_k. Early
 * stopping as in SPEC-GBDT's trainer: strict improvement, cut at the best iteration.
 *
 * Refused by the host (ValueError naming the key): objective other than rank:pairwise, rank:ndcg and binary:logistic (the
 * latter two: SPEC-OBJ, otto_objective.h), booster other than gbtree, tree_method outside hist / gpu_hist / auto,
 * grow_policy lossguide, max_leaves != 0, alpha != 0, max_delta_step != 0, colsample_bylevel / colsample_bynode != 1,
 * scale_pos_weight != 1 with a rank objective, num_pairsample != 1, num_parallel_tree != 1, eval_metric other than map /
 * map- / map@k / ndcg / ndcg- / ndcg@k and, with binary:logistic only, auc / logloss; base_score outside (0, 1) with
 * binary:logistic; sampling_method other than uniform, max_depth outside [1, 10].
 */
#ifndef OTTO_XGB_H
#define OTTO_XGB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_XGB_MAX_DEPTH 10

/* d_score float64 [n], d_label int32 [n], d_query_off int64 [Q+1]; d_sigmoid float64 [OTTO_GBDT_SIGMOID_BINS] at sigma = 1
 * with its lo and factor (otto_gbdt.h); seed_it = the already mixed mix(objective_seed, it); d_grad, d_hess float64 [n],
 * overwritten. One synchronisation (the error words). weighting = 0 is SPEC-XGB's rank:pairwise (d_discount is not read
 * and may be NULL); weighting = 1 is rank:ndcg, the same pairs with LambdaMART's weights (SPEC-OBJ,
 * include/otto_objective.h): every pair's g and h2 multiplied by the |delta NDCG| of swapping its rows; d_discount float64
 * [OTTO_GBDT_MAX_QUERY] (otto_gbdt.h). */
int otto_xgb_lambdamart(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                        const double* d_sigmoid, double sigmoid_lo, double sigmoid_factor, uint64_t seed_it, int32_t weighting,
                        const double* d_discount, double* d_grad, double* d_hess, void* stream);

/* One tree of otto_xgb_grow_tree. The arrays are HOST buffers of the caller: node arrays of 2^max_depth - 1 entries, leaf
 * arrays of 2^max_depth. The last three fields are written by the call. */
typedef struct otto_xgb_tree {
    int32_t* split_feature;    /* per internal node, SPEC-GBDT's numbering */
    int32_t* split_bin;
    double* threshold;
    int8_t* decision_type;
    int32_t* left_child;       /* >= 0: internal node, < 0: ~leaf */
    int32_t* right_child;
    double* split_gain;
    double* cover;             /* H_P */
    double* sum_grad;          /* G_P */
    int64_t* count;            /* cnt_P */
    int32_t* left_id;          /* XGBoost node id of the left child */
    int32_t* right_id;
    double* leaf_value;        /* per leaf */
    double* leaf_cover;        /* H of the leaf */
    double* leaf_sum_grad;     /* G of the leaf */
    int64_t* leaf_count;
    int32_t n_leaves;          /* 1: the root had no admissible split; only the leaf arrays' entry 0 is written */
    int32_t n_syncs;           /* stream synchronisations inside the call: at most max_depth + 2 */
    int64_t hist_rows;         /* rows the histogram kernel read */
} otto_xgb_tree;

/* bytes of d_work for otto_xgb_grow_tree: two row lists, the level's descriptors and split records, and the resident
 * histograms of a level, max(1, 2^(max_depth-1)) * 3 * F * 256 * 8 bytes; 0 for refused arguments */
int64_t otto_xgb_workspace_bytes(int64_t n, int32_t F, int32_t max_depth);

/* One whole depth-wise tree: one synchronisation per level, none per node. d_bins, d_gh, d_exp, d_n_edges, h_edges as for
 * otto_gbdt_grow_tree, d_bag / n_bag and d_features / n_used too (NULL: all rows / every feature; a feature list costs
 * one more synchronisation). min_child_weight, lambda, gamma, eta: SPEC-XGB. */
int otto_xgb_grow_tree(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_exp,
                       const int32_t* d_n_edges, const float* h_edges, int32_t max_depth, double min_child_weight, double lambda,
                       double gamma, double eta, const int32_t* d_bag, int64_t n_bag, const int32_t* d_features, int32_t n_used,
                       otto_xgb_tree* tree, void* d_work, int64_t work_bytes, void* stream);

/* The level steps of otto_xgb_grow_tree, one launch each over a HOST array of n_nodes descriptors (int32 [n_nodes, 8]),
 * for tests and tools. A descriptor = { begin, cnt, slot, slot2, 0, feature, bin, default_left }: rows
 * d_rows[begin .. begin + cnt) (ranges must not overlap and lie inside [0, n_rows)), histogram slot `slot` of d_hist
 * int64 [n_slots, 3, F, 256]. d_work: otto_xgb_workspace_bytes(n_rows, 1, 1) is enough for each.
 *   hist:      d_hist[slot] = the histogram of the node's rows (overwritten), over d_features if given; then, for a
 *              descriptor with slot2 >= 0, d_hist[slot2] -= d_hist[slot] (the larger sibling from its parent).
 *   split:     d_split int64 [n_nodes, OTTO_GBDT_SPLIT_WORDS] = the best split of d_hist[slot]; min_data_in_leaf = 0.
 *   partition: d_out[begin .. begin + cnt) = the node's rows that go left under (feature, bin, default_left) in their
 *              order, then the others in theirs; d_n_left int64 [n_nodes]. d_out must not overlap d_rows. */
int otto_xgb_level_hist(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_gh, const int32_t* d_rows, int64_t n_rows,
                        const int32_t* h_nodes, int32_t n_nodes, const int32_t* d_features, int32_t n_used, int64_t* d_hist,
                        int32_t n_slots, void* d_work, int64_t work_bytes, void* stream);
int otto_xgb_level_split(const int64_t* d_hist, int32_t n_slots, int32_t F, const int32_t* d_n_edges, const int32_t* d_exp,
                         const int32_t* h_nodes, int32_t n_nodes, double min_child_weight, double lambda, double gamma,
                         const int32_t* d_features, int32_t n_used, int64_t* d_split, void* d_work, int64_t work_bytes,
                         void* stream);
int otto_xgb_level_partition(const uint8_t* d_bins, int64_t n, int32_t F, const int32_t* d_rows, int64_t n_rows,
                             const int32_t* h_nodes, int32_t n_nodes, int32_t* d_out, int64_t* d_n_left, void* d_work,
                             int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
