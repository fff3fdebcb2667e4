"""The problems and parameters of tests/test_gbdt_sampling_gpu.py, with their restated results computed once per process.
tests/test_gbdt_sampling_cpu.py proves (without a GPU) that every one of them has the shape the device tests rely on."""
import numpy as np

import gbdt_restatement as gr
import gbdt_sampling_restatement as sr

BAGGING_SEED = 42
FEATURE_SEED = 42


def first_iteration_without(F, fraction, seed, feature, start=0):
    """The first iteration >= start whose feature list leaves ``feature`` out."""
    it = start
    while feature in sr.feature_list(F, fraction, seed, it):
        it += 1
    return it


# ---- single trees: (name, F, queries, num_leaves, bagging_fraction or None, feature_fraction or None)
# queries of 5 .. 45 rows: about 4,000 / 10,000 / 20,000 rows
TREE_CASES = [
    ('f3_bag90', 3, 160, 8, 0.9, None),
    ('f3_feat50', 3, 160, 8, None, 0.5),
    ('f3_both', 3, 160, 16, 0.5, 0.5),
    ('f9_bag50', 9, 400, 16, 0.5, None),
    ('f9_feat90', 9, 400, 16, None, 0.9),
    ('f9_both', 9, 400, 8, 0.9, 0.5),
    ('f54_bag90', 54, 800, 16, 0.9, None),
    ('f54_feat90', 54, 800, 16, None, 0.9),
    ('f54_feat50', 54, 800, 8, None, 0.5),
    ('f54_both', 54, 800, 16, 0.5, 0.9),
]
TREE_NAMES = [c[0] for c in TREE_CASES]
_TREE_PROBLEMS, _TREES = {}, {}


def tree_problem(F, n_queries):
    """dict(bins uint8 [F, n], q int32 [n, 2], exps, edge_list, edges float32 [F, 254], n_edges): gradients that follow the
    label, which follows columns 0, 1 and 2 (gr.random_problem), so that feature 0 wins the root when it may."""
    key = (F, n_queries)
    if key not in _TREE_PROBLEMS:
        rng = np.random.default_rng([7, F, n_queries])
        X, label, _ = gr.random_problem(rng, n_queries, F)
        edge_list = [gr.fit_edges(X[:, f]) for f in range(F)]
        bins = gr.bin_rows(X, edge_list)
        n = X.shape[0]
        grad = (0.15 - label) * (0.5 + rng.random(n)) + 0.05 * rng.standard_normal(n)
        hess = 0.05 + 0.2 * rng.random(n)
        q, exps = gr.quantize(grad, hess)
        _TREE_PROBLEMS[key] = dict(bins=bins, q=q, exps=exps, edge_list=edge_list, n=n, F=F)
    return _TREE_PROBLEMS[key]


def tree_case(name):
    """dict(problem, params, bag (int32 or None), bag_seed, features (int32 or None), want: the restated tree)."""
    if name not in _TREES:
        _, F, n_queries, num_leaves, p_bag, q_feat = TREE_CASES[TREE_NAMES.index(name)]
        prob = tree_problem(F, n_queries)
        params = dict(gr.DEFAULTS, num_leaves=num_leaves, min_data_in_leaf=20)
        bag = bag_seed = features = None
        if p_bag is not None:
            bag_seed = sr.mix(BAGGING_SEED, 2 * 1)                 # draw 1
            bag = sr.bag(prob['n'], sr.bag_size(p_bag, prob['n']), bag_seed)
        if q_feat is not None:
            # a list without feature 0 where the list is small enough to lose it soon; otherwise iteration 0
            it = first_iteration_without(F, q_feat, FEATURE_SEED, 0) if q_feat <= 0.5 else 0
            features = sr.feature_list(F, q_feat, FEATURE_SEED, it)
        want = sr.grow_tree(prob['bins'], prob['q'], prob['exps'], prob['edge_list'], params, bag, features)
        _TREES[name] = dict(problem=prob, params=params, bag=bag, bag_seed=bag_seed, features=features, want=want)
    return _TREES[name]


# ---- trainings
TRAIN_PARAMS = dict(num_leaves=8, min_data_in_leaf=20, lambdarank_norm=False, learning_rate=0.2)
STOP_PARAMS = dict(num_leaves=4, min_data_in_leaf=10, lambdarank_norm=False, learning_rate=0.3, eval_at=5)
# name -> (sampling keywords, uses a validation set, num_boost_round, early_stopping_rounds)
TRAIN_CASES = {
    'freq1': (dict(bagging_fraction=0.9, bagging_freq=1, feature_fraction=0.5), False, 6, None),
    'freq3_valid': (dict(bagging_fraction=0.5, bagging_freq=3, feature_fraction=0.9), True, 6, None),
    'freq3_stop': (dict(bagging_fraction=0.9, bagging_freq=3, feature_fraction=0.5), True, 30, 4),
}
_TRAIN_PROBLEMS, _TRAININGS = {}, {}


def train_problem(kind):
    """dict(X, label, query_off, edge_list, bins, params[, Xv, vlabel, voff, vbins])."""
    if kind not in _TRAIN_PROBLEMS:
        if kind == 'stop':
            # training labels follow column 0 and column 1; the validation labels follow column 0 and the opposite of
            # column 1, which the later trees pick up: validation AP peaks early, then falls
            rng = np.random.default_rng(77)
            X, _, query_off = gr.random_problem(rng, 120, 3, min_len=6, max_len=14, nan_share=0.0)
            Xv, _, voff = gr.random_problem(rng, 80, 3, min_len=6, max_len=14, nan_share=0.0)
            label = ((X[:, 0] + 0.9 * X[:, 1] + 0.3 * rng.standard_normal(X.shape[0])) > 0.9).astype(np.int32)
            vlabel = ((Xv[:, 0] - 0.9 * Xv[:, 1] + 0.3 * rng.standard_normal(Xv.shape[0])) > 0.9).astype(np.int32)
            edge_list = [gr.fit_edges(X[:, f]) for f in range(3)]
            d = dict(X=X, label=label, query_off=query_off, Xv=Xv, vlabel=vlabel, voff=voff, params=dict(STOP_PARAMS))
        else:
            rng = np.random.default_rng(31)
            X, label, query_off = gr.random_problem(rng, 120, 9)
            Xv, vlabel, voff = gr.random_problem(rng, 60, 9)
            edge_list = [gr.fit_edges(X[:, f]) for f in range(9)]
            d = dict(X=X, label=label, query_off=query_off, Xv=Xv, vlabel=vlabel, voff=voff, params=dict(TRAIN_PARAMS))
        d['edge_list'] = edge_list
        d['bins'], d['vbins'] = gr.bin_rows(d['X'], edge_list), gr.bin_rows(d['Xv'], edge_list)
        _TRAIN_PROBLEMS[kind] = d
    return _TRAIN_PROBLEMS[kind]


def training(name):
    """dict(problem, sampling, valid (bool), rounds, early_stopping_rounds, want: the restated training)."""
    if name not in _TRAININGS:
        sampling, valid, rounds, stop = TRAIN_CASES[name]
        d = train_problem('stop' if name.endswith('_stop') else 'random')
        want = sr.train(d['bins'], d['label'], d['query_off'], d['edge_list'], d['params'],
                        valid=(d['vbins'], d['vlabel'], d['voff']) if valid else None, num_boost_round=rounds,
                        early_stopping_rounds=stop, bagging_seed=BAGGING_SEED, feature_fraction_seed=FEATURE_SEED, **sampling)
        _TRAININGS[name] = dict(problem=d, sampling=sampling, valid=valid, rounds=rounds, early_stopping_rounds=stop, want=want)
    return _TRAININGS[name]
