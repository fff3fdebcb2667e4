"""Seeded inputs of the SPEC-XGB tests (tests/test_xgb_cpu.py proves their shapes, tests/test_xgb_gpu.py runs them on the
device), and the references the device tests share: each is computed once by tests/xgb_restatement.py and kept."""
import functools

import numpy as np

import gbdt_restatement as gr
import gbdt_sampling_restatement as sr
import xgb_restatement as xr

OBJECTIVE_SEED = xr.seeds(7)[0]
OBJECTIVE_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1024)
OBJECTIVE_KINDS = ('random', 'all_equal_labels', 'no_positive', 'all_scores_equal', 'tied_scores', 'labels_0_to_31', 'beyond_table',
                   'nan_score')


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def objective_sizes():
    """(score, label, query_off): one query of every size of OBJECTIVE_SIZES, three labels, some tied scores."""
    rng = np.random.default_rng(11)
    off = _offsets(OBJECTIVE_SIZES)
    n = int(off[-1])
    score = np.round(rng.standard_normal(n) * 2, 1)
    label = rng.integers(0, 3, n).astype(np.int32)
    return score, label, off


EDGE_SIZES = (127, 128, 129, 130, 5, 128, 200, 1, 129, 60)      # 128: the longest query the one-wave kernel takes


@functools.lru_cache(maxsize=None)
def objective_edge():
    """(score, label, query_off): queries on either side of the size at which the device hands over to its second kernel,
    mixed with short ones so that one workgroup of the second kernel walks past queries that are not its own."""
    rng = np.random.default_rng(12)
    off = _offsets(EDGE_SIZES)
    n = int(off[-1])
    return np.round(rng.standard_normal(n), 2), rng.integers(0, 4, n).astype(np.int32), off


@functools.lru_cache(maxsize=None)
def objective_kind(kind):
    """(score, label, query_off): 40 queries of 20 to 60 rows (one wave per query on the device)."""
    rng = np.random.default_rng(100 + OBJECTIVE_KINDS.index(kind))
    off = _offsets(rng.integers(20, 61, 40))
    n = int(off[-1])
    score = rng.standard_normal(n)
    label = rng.integers(0, 4, n).astype(np.int32)
    if kind == 'all_equal_labels':
        label[:] = 1
    elif kind == 'no_positive':
        for q in range(0, 40, 2):                           # every other query holds no positive
            label[off[q]:off[q + 1]] = 0
    elif kind == 'all_scores_equal':
        score[:] = 0.25
    elif kind == 'tied_scores':
        score = np.round(score)                             # a handful of values; -0.0 and +0.0 both occur
        assert (np.signbit(score) & (score == 0)).any() and (~np.signbit(score) & (score == 0)).any()
    elif kind == 'labels_0_to_31':
        label = rng.integers(0, 32, n).astype(np.int32)
    elif kind == 'beyond_table':
        score = score * 100.0
    elif kind == 'nan_score':
        score[rng.random(n) < 0.1] = np.nan
    return score, label, off


@functools.lru_cache(maxsize=None)
def objective_want(name, it=0):
    score, label, off = objective_sizes() if name == 'sizes' else objective_edge() if name == 'edge' else objective_kind(name)
    return xr.pairwise(score, label, off, OBJECTIVE_SEED, it)


# ---- growth

GROW_N, GROW_F = 20000, 8
GROW_FEATURES = np.array([0, 1, 2, 4, 5, 7], dtype=np.int32)
BASE = {'max_depth': 6, 'min_child_weight': 1.0, 'lambda': 1.0, 'gamma': 0.0, 'eta': 0.3}
# name -> (parameter changes, bag, feature list)
GROW_CASES = {
    'depth1': ({'max_depth': 1}, False, False),
    'depth2': ({'max_depth': 2}, False, False),
    'depth6': ({}, False, False),
    'depth10': ({'max_depth': 10}, False, False),
    'depth6_mcw0': ({'min_child_weight': 0.0}, False, False),
    'depth10_mcw0': ({'max_depth': 10, 'min_child_weight': 0.0}, False, False),
    'depth10_mcw0_bag_list': ({'max_depth': 10, 'min_child_weight': 0.0}, True, True),
    'depth6_bag': ({}, True, False),
    'depth6_list': ({}, False, True),
    'depth2_bag_list': ({'max_depth': 2}, True, True),
    'root_cannot_split': ({'min_child_weight': 1e9}, False, False),
    'gamma_above_every_gain': ({'gamma': 1e12}, False, False),
}


@functools.lru_cache(maxsize=None)
def grow_problem():
    """dict(X, bins, edge_list, q, exps, bag): 20,000 rows x 8 features of 16 levels each (feature 3 holds NaN). The
    gradient is 2 + structure where x1 >= 0.5, exactly 0 where x1 < 0.5 and x0 < 0.25, and 0.5 + structure elsewhere: the
    root splits on x1, its left child on x0, and the rows with zero gradient form a depth-2 node that no split improves
    (G = 0: every gain is 0), while its sibling keeps growing."""
    rng = np.random.default_rng(5)
    n, F = GROW_N, GROW_F
    X = (rng.integers(0, 16, (n, F)) / 16.0).astype(np.float32)
    fine = 0.3 * np.sin(7.0 * X[:, 2] + 3.0 * X[:, 4]) + 0.2 * X[:, 5] * X[:, 6] + 0.1 * rng.standard_normal(n)
    grad = np.where(X[:, 1] >= 0.5, 2.0 + fine, np.where(X[:, 0] < 0.25, 0.0, 0.5 + fine))
    hess = 0.5 + 0.25 * rng.random(n)
    X[rng.random(n) < 0.1, 3] = np.nan
    edge_list = [gr.fit_edges(X[:, f]) for f in range(F)]
    bins = gr.bin_rows(X, edge_list)
    q, exps = gr.quantize(grad, hess)
    bag = sr.bag(n, int(0.7 * n), sr.mix(99, 0))
    return dict(X=X, bins=bins, edge_list=edge_list, q=q, exps=exps, bag=bag)


def grow_params(name):
    p = dict(BASE)
    p.update(GROW_CASES[name][0])
    return p


@functools.lru_cache(maxsize=None)
def grow_want(name):
    d = grow_problem()
    _, bag, feats = GROW_CASES[name]
    return xr.grow_tree(d['bins'], d['q'], d['exps'], d['edge_list'], grow_params(name), d['bag'] if bag else None,
                        GROW_FEATURES if feats else None)


def leaf_depths(tree):
    """The depth of every leaf of a restated tree."""
    L = tree['leaf_value'].size
    depth = np.zeros(L, dtype=np.int64)
    if L == 1:
        return depth
    stack = [(0, 1)]
    while stack:
        node, d = stack.pop()
        for c in (tree['left_child'][node], tree['right_child'][node]):
            if c >= 0:
                stack.append((int(c), d + 1))
            else:
                depth[~c] = d
    return depth


# ---- level launches

HIST_SEGMENTS = (1, 2047, 2048, 2049, 5000)                  # 2048: the chunk floor of the histogram
PART_SEGMENTS = (1, 255, 256, 257, 2048, 2049, 300, 300, 300)   # 256: a scan tile; 2048: a partition block


@functools.lru_cache(maxsize=None)
def level_problem(F):
    """dict(bins uint8 [F, n], q int32 [n, 2], rows int32: a shuffled row list longer than the segments need)."""
    rng = np.random.default_rng(40 + F)
    n = 13000
    bins = rng.integers(0, 40, (F, n)).astype(np.uint8)
    bins[rng.random((F, n)) < 0.05] = gr.NAN_BIN
    q = rng.integers(-2 ** 29, 2 ** 29, (n, 2)).astype(np.int32)
    q[:, 1] = np.abs(q[:, 1])
    rows = rng.permutation(n).astype(np.int32)
    return dict(bins=bins, q=q, rows=rows)


def segments(sizes, gap=3):
    """(begin, cnt) of consecutive segments of a row list with ``gap`` unused rows between them."""
    out, at = [], 2
    for s in sizes:
        out.append((at, s))
        at += s + gap
    return out


# ---- training

TRAIN_F = 12
TRAIN_CASES = {
    'sampled': dict(params={'subsample': 0.8, 'colsample_bytree': 0.75, 'max_depth': 4, 'seed': 3}, rounds=5, early=None),
    'plain': dict(params={'max_depth': 4, 'eval_metric': 'map-'}, rounds=5, early=None),
    'early_stopping': dict(params={'max_depth': 3, 'eta': 1.0, 'min_child_weight': 0.1}, rounds=8, early=2),
    'sampled_stop': dict(params={'max_depth': 3, 'eta': 1.0, 'min_child_weight': 0.1, 'subsample': 0.7, 'colsample_bytree': 0.5,
                                 'seed': 5}, rounds=10, early=2),
}


@functools.lru_cache(maxsize=None)
def train_problem():
    rng = np.random.default_rng(77)
    X, label, off = gr.random_problem(rng, 300, TRAIN_F, 20, 60, n_levels=24)
    Xv, vlabel, voff = gr.random_problem(rng, 100, TRAIN_F, 20, 60, n_levels=24)
    vlabel[voff[3]:voff[4]] = 0                             # a validation query without a positive
    edge_list = [gr.fit_edges(X[:, f]) for f in range(TRAIN_F)]
    return dict(X=X, label=label, query_off=off, Xv=Xv, vlabel=vlabel, voff=voff, edge_list=edge_list,
                bins=gr.bin_rows(X, edge_list), vbins=gr.bin_rows(Xv, edge_list))


@functools.lru_cache(maxsize=None)
def train_want(name):
    d, c = train_problem(), TRAIN_CASES[name]
    return xr.train(d['bins'], d['label'], d['query_off'], d['edge_list'], c['params'], valid=(d['vbins'], d['vlabel'], d['voff']),
                    num_boost_round=c['rounds'], early_stopping_rounds=c['early'])
