/*
 * otto_objective.h -- C-ABI of the objectives and validation metrics the two tree trainers share beyond their first ones
 * (SPEC-OBJ): pointwise logistic gradients, label counts, NDCG@k, AUC and logloss. The LambdaMART
 * weighting of the pairwise objective (rank:ndcg) is otto_xgb_lambdamart in include/otto_xgb.h and is specified here.
 *
 * What this adds over the reference: its two trainers call lgb.train with `lambdarank` and xgb.train with `rank:pairwise`
 * only; the binary objective, NDCG, AUC and logloss are what users of either library expect of a candidate ranker. Binning,
 * quantisation, histograms, split search, growth, sampling, scoring and the model writers are SPEC-GBDT's / SPEC-XGB's.
 *
 * Conventions of otto_gbdt.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; all device work on
 * the caller's stream; no buffer is allocated per call (the error words live in the per-device scratch of the GBDT family:
 * calls of the families on one device must not overlap); one synchronisation where an error word is read.
 * The functions without a stream parameter (otto_obj_constants, otto_obj_auc_workspace_bytes) run on the host and enqueue nothing.
 *
 * SPEC-OBJ. Normative. All float64 arithmetic runs without contraction, products left to right. T, lo, factor: SPEC-GBDT's
 * sigmoid table at sigma = 1 (entry i = 1/(1+exp(lo + i/factor)), lo = -25, BINS = OTTO_GBDT_SIGMOID_BINS); discount[r] =
 * 1/log2(2+r); gain(l) = 2^l - 1. Both tables come from the host.
 *
 * 1. Pointwise logistic gradients (otto_obj_binary). Per row:
 *        t = label > 0;  x = (-(sigma*score) - lo) * factor;  x = x > 0 ? x : 0 (NaN -> 0);  x = min(x, BINS - 1);
 *        p = T[(size_t)x]                       (= sigmoid(sigma*score) at the table's resolution)
 *        w = t ? w_pos : w_neg
 *        grad = sigma*(p - t)*w;   hess = max(sigma*sigma*p*(1.0 - p), hess_floor)*w
 *    A label outside 0..31: that row's outputs are zero and the call returns OTTO_EINVAL after the stream has drained.
 *    The table lookup is a departure from LightGBM's and XGBoost's exact exp, next to those SPEC-GBDT and SPEC-XGB state:
 *    |p - sigmoid(sigma*score)| <= (1/factor)/4 inside [-25, 25] (the sigmoid's slope is at most 1/4), and it is what keeps
 *    the quantised gradients, and with them the trees, bit-exact against the NumPy restatement.
 *    LightGBM `binary`: hess_floor = 0, sigma = `sigmoid`; is_unbalance gives weight 1 to the larger class and
 *    cnt_large/cnt_small to the smaller one; w_pos is then multiplied by scale_pos_weight; is_unbalance together with
 *    scale_pos_weight != 1 is refused. XGBoost `binary:logistic`: sigma = 1, hess_floor = 1e-16, w_pos = scale_pos_weight,
 *    w_neg = 1.
 *
 * 2. Label counts and initial score. otto_obj_label_counts: {rows with label > 0, n}, exact.
 *    LightGBM family, boost_from_average (default true): pavg = clip(n_pos/n, 1e-15, 1 - 1e-15); init =
 *    log(pavg/(1 - pavg))/sigma, float64 on the host. Training and validation scores start at init; the forest and the
 *    written model carry init added once into every leaf value of the first tree (LightGBM's AddBias), so that scoring
 *    the forest from 0.0 returns the trainer's own bits.
 *    XGBoost family: margin0 = log(base_score/(1 - base_score)) on the host (exactly 0.0 at 0.5); base_score outside (0, 1)
 *    is refused for binary:logistic; the JSON model stores base_score as the probability.
 *
 * 3. rank:ndcg (otto_xgb_lambdamart, weighting = 1). Pairs and draws are SPEC-XGB's. Per pair, r_high / r_low the ranks:
 *        delta = |(gain_high - gain_low) * (discount[r_high] - discount[r_low])| * inv_idcg
 *        g = (p - 1.0)*delta;   h2 = 2.0*max(p*(1.0 - p), 1e-16)*delta
 *    inv_idcg = 1/IDCG, IDCG = sum over all cnt rows of gain(labels sorted descending)[r]*discount[r] in rank order from 0.0;
 *    0 if IDCG is 0. Accumulation order as in SPEC-XGB. weighting = 0 is SPEC-XGB's rank:pairwise, bit for bit.
 *
 * 4. Metrics.
 *    NDCG@k of a query, in SPEC-GBDT's rank order: DCG = sum_{r < min(k, cnt)} gain(label_r)*discount[r] from 0.0 in rank
 *    order; maxDCG the same sum over the labels sorted descending; ndcg = DCG/maxDCG, -1 when maxDCG == 0 (also an empty
 *    query). The host mean counts -1 as 1.0 (`ndcg`) or 0.0 (`ndcg-`). A bad query: -1 and OTTO_EINVAL, as for AP@k.
 *    AUC. key = ~score_key(score) (score_key: SPEC-GBDT's order-preserving image, -0.0 == +0.0, every NaN the smallest), so
 *    ascending keys are descending scores with NaN last. The (key, label > 0) pairs are sorted; Ppre = exclusive prefix
 *    count of positives; per maximal run [a, b) of equal keys: neg = (b-a) - (Ppre(b)-Ppre(a)); A2 += neg*(Ppre(a)+Ppre(b)).
 *    int64 sums, independent of order. AUC = A2/(2*P*N) on the host, each integer converted to float64 once; 1.0 when
 *    P == 0 or N == 0. (A2 counts, twice, the (positive, negative) pairs with the positive ahead, ties half.)
 *    Logloss. Per row z = -y*sigma*score, y = label > 0 ? 1 : -1; term = z > 0 ? z + log1p(exp(-z)) : log1p(exp(z)) with the
 *    device's exp / log1p (the only unpinned functions). The rows are cut into OTTO_OBJ_LOGLOSS_PARTS contiguous parts of
 *    ceil(n / PARTS) rows rounded up to a multiple of 256; a part is summed by one workgroup of 256 threads (thread t adds
 *    rows t, t + 256, ... of the part in order, then a fixed LDS tree), and the parts by one workgroup in the same way:
 *    the sum does not depend on the grid. The host divides by n.
 *
 * Refused / out of scope: rank_xendcg, rank:map, multiclass, sample weights, several eval_at values (the first decides),
 * lambda_l1, a constant first tree when the root cannot split.
 */
#ifndef OTTO_OBJECTIVE_H
#define OTTO_OBJECTIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_OBJ_LOGLOSS_PARTS 1024

/* out int32 [5] = { threads of a workgroup of the row kernels, their largest grid (a grid-stride is the product), keys of a
 * sort tile, rows of a scan tile, OTTO_OBJ_LOGLOSS_PARTS }: for tests and tools that aim at the kernels' edges. */
void otto_obj_constants(int32_t* out);

/* d_score float64 [n], d_label int32 [n]; d_sigmoid float64 [OTTO_GBDT_SIGMOID_BINS] at sigma = 1 with its lo and factor;
 * d_grad, d_hess float64 [n], overwritten. One synchronisation (the error words). */
int otto_obj_binary(const double* d_score, const int32_t* d_label, int64_t n, const double* d_sigmoid, double sigmoid_lo,
                    double sigmoid_factor, double sigma, double w_pos, double w_neg, double hess_floor, double* d_grad,
                    double* d_hess, void* stream);

/* d_counts int64 [2] = { rows with label > 0, n }. No synchronisation. */
int otto_obj_label_counts(const int32_t* d_label, int64_t n, int64_t* d_counts, void* stream);

/* d_discount float64 [OTTO_GBDT_MAX_QUERY]; d_ndcg float64 [Q]; 1 <= k <= OTTO_GBDT_MAX_QUERY. One synchronisation. */
int otto_obj_ndcg_at_k(const double* d_score, const int32_t* d_label, const int64_t* d_query_off, int64_t Q, int64_t n,
                       int32_t k, const double* d_discount, double* d_ndcg, void* stream);

/* d_out int64 [3] = { A2, P, N }. d_work: otto_obj_auc_workspace_bytes(n) bytes (0 for a refused n); a smaller one returns
 * OTTO_EINVAL before anything is launched. 0 <= n < 2^31. One synchronisation (inside the sort). */
int64_t otto_obj_auc_workspace_bytes(int64_t n);
int otto_obj_auc(const double* d_score, const int32_t* d_label, int64_t n, int64_t* d_out, void* d_work, int64_t work_bytes,
                 void* stream);

/* d_partials float64 [OTTO_OBJ_LOGLOSS_PARTS], d_loss float64 [1] = the sum over the rows. No synchronisation.
 * otto_obj_logloss_grid: the same with a grid of `grid` workgroups (1 .. OTTO_OBJ_LOGLOSS_PARTS), for tests: the bits do not
 * depend on it. */
int otto_obj_logloss(const double* d_score, const int32_t* d_label, int64_t n, double sigma, double* d_partials, double* d_loss,
                     void* stream);
int otto_obj_logloss_grid(const double* d_score, const int32_t* d_label, int64_t n, double sigma, int32_t grid, double* d_partials,
                          double* d_loss, void* stream);

#ifdef __cplusplus
}
#endif
#endif
