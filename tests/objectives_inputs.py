"""Seeded inputs of the SPEC-OBJ tests (tests/test_objectives_cpu.py proves the restatement on them, the two GPU files run
them on the device), and the references the device tests share: each is computed once by tests/objectives_restatement.py
and kept."""
import functools

import numpy as np

import gbdt_restatement as gr
import objectives_restatement as orr
import xgb_restatement as xr

OBJECTIVE_SEED = xr.seeds(7)[0]
SIGMAS = (1.0, 0.5, 2.0)
# Relative tolerance of a device logloss against the float64 NumPy restatement: only exp / log1p and the order of the sum
# differ. Measured on an MI355X over the sums of test_objectives_gpu.py::test_logloss_is_close_and_does_not_depend_on_the_grid
# and the logloss histories of the two early-stopping trainings below: the largest relative difference was 3.667e-16 (the
# sum of 262,145 rows at sigma = 0.5; most sums had the restatement's bits). Four times that, rounded up.
LOGLOSS_RTOL = 1.5e-15


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def special_scores(sigma):
    """+-0.0, +-25/sigma (the ends of the table), the next float beyond each, +-inf, NaN."""
    e = 25.0 / sigma
    return np.array([0.0, -0.0, e, -e, np.nextafter(e, np.inf), np.nextafter(-e, -np.inf), np.inf, -np.inf, np.nan], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def binary_rows(n, sigma=1.0, labels='mixed'):
    """(score float64 [n], label int32 [n]): normal scores wide enough to saturate the table at either end, the special
    scores cycled through the first rows with both classes, labels 0 / 1 and a few up to 31."""
    rng = np.random.default_rng(1000 + n % 997)
    score = rng.standard_normal(n) * (12.0 / sigma)
    sp = special_scores(sigma)
    m = min(n, 2 * sp.size)
    score[:m] = np.tile(sp, 2)[:m]
    label = (rng.random(n) < 0.3).astype(np.int32)
    label[:m] = (np.arange(m) >= sp.size).astype(np.int32)          # every special score with a negative, then a positive
    label[m:][rng.random(n - m) < 0.02] = 31
    if labels == 'all_positive':
        label[:] = 1
    elif labels == 'all_negative':
        label[:] = 0
    return score, label


@functools.lru_cache(maxsize=None)
def binary_want(n, sigma, w_pos, w_neg, hess_floor, labels='mixed'):
    score, label = binary_rows(n, sigma, labels)
    return orr.binary(score, label, sigma, w_pos, w_neg, hess_floor)


# ---- NDCG

NDCG_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 0, 40, 40, 40, 40)
NDCG_K = (1, 20, 50, 1024)


@functools.lru_cache(maxsize=None)
def ndcg_problem():
    """(score, label, query_off): one query of every size of NDCG_SIZES (0: an empty one); the last four of 40 rows: all
    labels zero, labels 0..31, every score the same (position order), every score the same and all labels zero."""
    rng = np.random.default_rng(21)
    off = _offsets(NDCG_SIZES)
    n = int(off[-1])
    score = np.round(rng.standard_normal(n) * 2, 1)                 # ties inside the queries
    label = rng.integers(0, 3, n).astype(np.int32)
    q = len(NDCG_SIZES) - 4
    label[off[q]:off[q + 1]] = 0
    label[off[q + 1]:off[q + 2]] = rng.integers(0, 32, 40)
    label[off[q + 1]] = 31
    score[off[q + 2]:off[q + 3]] = 0.5
    score[off[q + 3]:off[q + 4]] = -1.25
    label[off[q + 3]:off[q + 4]] = 0
    return score, label, off


@functools.lru_cache(maxsize=None)
def ndcg_want(k):
    return orr.ndcg_at_k(*ndcg_problem(), k)


# ---- AUC

AUC_KINDS = ('random', 'all_equal', 'straddle', 'zeros', 'nan_last', 'only_positive', 'only_negative', 'separable', 'reversed')


@functools.lru_cache(maxsize=None)
def auc_rows(kind, n, tile=4096):
    """(score, label) of ``n`` rows. 'straddle': runs of equal scores of ``tile`` / 2 + 3 rows, so that runs start and end on
    either side of every multiple of ``tile`` (the sort's tile and the scan's are both handed in by the caller)."""
    rng = np.random.default_rng(31 + AUC_KINDS.index(kind) + n)
    score = rng.standard_normal(n)
    label = (rng.random(n) < 0.4).astype(np.int32) * rng.integers(1, 4, n).astype(np.int32)
    if kind == 'random':
        score = np.round(score, 2)
    elif kind == 'all_equal':
        score[:] = 0.75
    elif kind == 'straddle':
        score = (rng.permutation(n) // (tile // 2 + 3)).astype(np.float64)
    elif kind == 'zeros':
        score = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        score[::7] = 1.0
    elif kind == 'nan_last':
        score[rng.random(n) < 0.2] = np.nan
        score[0], label[0] = np.nan, 1
        if n > 2:
            score[1], label[1] = -np.inf, 0
    elif kind == 'only_positive':
        label[:] = 2
    elif kind == 'only_negative':
        label[:] = 0
    elif kind in ('separable', 'reversed'):
        label = (np.arange(n) % 3 == 0).astype(np.int32)
        score = np.where(label > 0, 1.0, -1.0) * (1.0 + rng.random(n)) * (1.0 if kind == 'separable' else -1.0)
    return score, label


@functools.lru_cache(maxsize=None)
def auc_want(kind, n, tile=4096):
    return orr.auc_counts(*auc_rows(kind, n, tile))


# ---- logloss

@functools.lru_cache(maxsize=None)
def logloss_rows(n, sigma=1.0):
    """The rows of binary_rows without the scores that are not numbers, plus |sigma * score| = 800 with both classes."""
    score, label = binary_rows(n, sigma)
    score = np.where(np.isfinite(score), score, 3.0)
    if n >= 4:
        score[-4:] = np.array([800.0, -800.0, 800.0, -800.0]) / sigma
        label[-4:] = [1, 1, 0, 0]
    return score, label


# ---- rank:ndcg

LAMBDAMART_SIZES = (2, 50, 64, 65, 1024, 1, 30, 129)


@functools.lru_cache(maxsize=None)
def lambdamart_problem():
    """(score, label, query_off): one query of every size of LAMBDAMART_SIZES; the query of 30 rows holds one label only."""
    rng = np.random.default_rng(41)
    off = _offsets(LAMBDAMART_SIZES)
    n = int(off[-1])
    score = np.round(rng.standard_normal(n) * 2, 1)
    label = rng.integers(0, 4, n).astype(np.int32)
    label[0], label[1] = 0, 2                                       # the query of two rows has two labels
    q = LAMBDAMART_SIZES.index(30)
    label[off[q]:off[q + 1]] = 2
    return score, label, off


@functools.lru_cache(maxsize=None)
def lambdamart_want(it=0, weighting=1):
    return orr.lambdamart(*lambdamart_problem(), OBJECTIVE_SEED, it, weighting)


# ---- training

TRAIN_N, TRAIN_F = 2048, 6
GBDT_BASE = {'objective': 'binary', 'num_leaves': 8, 'min_data_in_leaf': 20, 'learning_rate': 0.3, 'eval_at': 5}
GBDT_CASES = {
    'auc': dict(params=dict(GBDT_BASE, metric='auc'), rounds=4, early=None),
    'ndcg_no_average': dict(params=dict(GBDT_BASE, metric='ndcg', boost_from_average=False), rounds=4, early=None),
    'logloss_early_unbalanced': dict(params=dict(GBDT_BASE, metric='binary_logloss', learning_rate=2.5, is_unbalance=True, sigmoid=2.0),
                                     rounds=8, early=2),
}
XGB_BASE = {'max_depth': 3, 'eta': 0.3}
XGB_CASES = {
    'binary_auc': dict(params=dict(XGB_BASE, objective='binary:logistic', eval_metric='auc', scale_pos_weight=2.0), rounds=4, early=None),
    'binary_logloss_early': dict(params=dict(XGB_BASE, objective='binary:logistic', eval_metric='logloss', eta=3.0, base_score=0.2),
                                 rounds=8, early=2),
    'ndcg': dict(params=dict(XGB_BASE, objective='rank:ndcg', eval_metric='ndcg@5'), rounds=4, early=None),
    'ndcg_minus': dict(params=dict(XGB_BASE, objective='rank:ndcg', eval_metric='ndcg-', seed=3), rounds=3, early=None),
}
# the restatement reads the resolved names
_RESTATED = {'binary_logloss': 'logloss'}


def _queries(rng, n, max_len=40):
    """Query lengths of 1 .. max_len rows that add up to exactly n."""
    lens = []
    while sum(lens) < n:
        lens.append(int(min(rng.integers(1, max_len + 1), n - sum(lens))))
    return _offsets(lens)


def _problem(rng, n):
    off = _queries(rng, n)
    X = rng.standard_normal((n, TRAIN_F)).astype(np.float32)
    X = (np.round(X * 6) / 6).astype(np.float32)
    signal = X[:, 0] - 0.7 * X[:, 1] + 0.5 * np.abs(X[:, 2]) + rng.standard_normal(n) * 0.8
    label = (signal > np.quantile(signal, 0.8)).astype(np.int32)
    X[rng.random((n, TRAIN_F)) < 0.08] = np.nan
    return X, label, off


@functools.lru_cache(maxsize=None)
def train_problem():
    """2,048 training rows x 6 features in queries of 1 to 40 rows, 1,024 validation rows; one validation query holds no
    positive."""
    rng = np.random.default_rng(177)
    X, label, off = _problem(rng, TRAIN_N)
    Xv, vlabel, voff = _problem(rng, TRAIN_N // 2)
    q = int(np.argmax(np.diff(voff) >= 5))
    vlabel[voff[q]:voff[q + 1]] = 0
    edge_list = [gr.fit_edges(X[:, f]) for f in range(TRAIN_F)]
    return dict(X=X, label=label, query_off=off, Xv=Xv, vlabel=vlabel, voff=voff, edge_list=edge_list,
                bins=gr.bin_rows(X, edge_list), vbins=gr.bin_rows(Xv, edge_list))


@functools.lru_cache(maxsize=None)
def gbdt_want(name):
    d, c = train_problem(), GBDT_CASES[name]
    params = dict(c['params'], metric=_RESTATED.get(c['params']['metric'], c['params']['metric']))
    return orr.train_gbdt(d['bins'], d['label'], d['query_off'], d['edge_list'], params, valid=(d['vbins'], d['vlabel'], d['voff']),
                          num_boost_round=c['rounds'], early_stopping_rounds=c['early'])


@functools.lru_cache(maxsize=None)
def xgb_want(name):
    d, c = train_problem(), XGB_CASES[name]
    return orr.train_xgb(d['bins'], d['label'], d['query_off'], d['edge_list'], c['params'], valid=(d['vbins'], d['vlabel'], d['voff']),
                         num_boost_round=c['rounds'], early_stopping_rounds=c['early'])
