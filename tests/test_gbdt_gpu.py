"""SPEC-GBDT on the device against the NumPy restatement (tests/gbdt_restatement.py): every kernel through its own entry
point, then whole trainings. Everything but the lambdarank_norm scaling is compared bit for bit."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import gbdt_restatement as gr
from otto_amd import _lib
from otto_amd.ranker import gbdt
from otto_amd.ranker.forest import forest_leaves, forest_predict, rank_candidates

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mapper(edge_list):
    edges = np.full((len(edge_list), gbdt.MAX_EDGES), np.inf, dtype=np.float32)
    for f, e in enumerate(edge_list):
        edges[f, :len(e)] = e
    return gbdt.BinMapper(edges, [len(e) for e in edge_list])


# ---- hand fixture

def test_hand_fixture_end_to_end(gpu_device):
    with open(os.path.join(GOLDEN, 'gbdt_hand.json')) as fh:
        h = json.load(fh)
    X = np.array([[np.nan if v is None else v for v in row] for row in h['X']], dtype=np.float32)
    mapper = gbdt.fit_bins(X)
    assert [mapper.feature_edges(f).tolist() for f in range(2)] == h['edges']
    bins = gbdt.bin_matrix(_t(X, gpu_device), mapper)
    assert bins.cpu().numpy().tolist() == h['bins']
    label, off = _t(np.array(h['label'], dtype=np.int32), gpu_device), _t(np.array(h['query_off'], dtype=np.int64), gpu_device)
    res = gbdt.train(bins, label, off, mapper, h['params'], num_boost_round=1, keep_leaves=True)
    tree = res.trees[0]
    for k in ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'threshold'):
        assert getattr(tree, k).tolist() == h[k], k
    assert np.allclose(tree.leaf_value, h['leaf_value'], rtol=1e-13, atol=0)
    want_leaf = np.zeros(8, dtype=np.int32)
    for i, rows in enumerate(h['leaf_rows']):
        want_leaf[rows] = i
    assert np.array_equal(res.train_leaf.cpu().numpy()[:, 0], want_leaf)
    assert np.array_equal(forest_leaves(res.forest, _t(X, gpu_device)).cpu().numpy()[:, 0], want_leaf)


# ---- binning

@pytest.mark.parametrize('F', [1, 54, 128])
def test_binning(gpu_device, F):
    rng = np.random.default_rng(F)
    sample = rng.standard_normal((3000, F)).astype(np.float32)
    sample[:, 0] = np.round(sample[:, 0] * 3)                      # few distinct values: values equal to edges
    mapper = gbdt.fit_bins(sample)
    edge_list = [mapper.feature_edges(f) for f in range(F)]
    for n in (1, 63, 64, 65, 1000):
        X = rng.standard_normal((n, F + 3)).astype(np.float32)    # row stride ld = F + 3 > F
        X[:, 0] = np.round(X[:, 0] * 3)
        for f in range(F):                                         # edge-equal values and their neighbours
            e = edge_list[f]
            pick = rng.integers(0, e.size, n)
            X[:, f] = np.where(rng.random(n) < 0.3, e[pick], X[:, f])
            X[:, f] = np.where(rng.random(n) < 0.1, np.nextafter(e[pick], np.float32(np.inf)), X[:, f])
        X[rng.random(X.shape) < 0.1] = np.nan
        X[0, 0] = np.inf if n > 1 else X[0, 0]
        got = gbdt.bin_matrix(_t(X, gpu_device)[:, :F], mapper).cpu().numpy()
        assert got.shape == (F, n) and np.array_equal(got, gr.bin_rows(X, edge_list)), (F, n)


# ---- objective

def _objective_case(rng, lens, kind):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    score = rng.standard_normal(n)
    label = (rng.random(n) < 0.2).astype(np.int32)
    if kind == 'all_equal_labels':
        label[:] = 1
    elif kind == 'no_positive':
        label[:] = 0
    elif kind == 'all_scores_equal':
        score[:] = 0.25
    elif kind == 'tied_scores':
        score = np.round(score * 2) / 2
        score[::7] = -0.0
        score[3::7] = 0.0
    elif kind == 'beyond_table':
        score = score * 40.0                                       # differences far outside [-25, 25]
    elif kind == 'graded':
        label = rng.integers(0, 5, n).astype(np.int32)
        label[::11] = 31
    return score, label, off


OBJECTIVE_LENS = [1, 2, 30, 31, 64, 65, 257, gbdt.MAX_QUERY]


@pytest.mark.parametrize('kind', ['random', 'all_equal_labels', 'no_positive', 'all_scores_equal', 'tied_scores', 'beyond_table',
                                  'graded'])
def test_objective_without_norm_is_bit_exact(gpu_device, kind):
    rng = np.random.default_rng(len(kind))
    # long queries first / short queries only: both workgroup sizes of the kernel
    for lens in (OBJECTIVE_LENS, [1, 2, 30, 31, 64, 65]):
        score, label, off = _objective_case(rng, lens, kind)
        g, h = gbdt.lambdarank_gradients(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), norm=False)
        wg, wh, invalid = gr.lambdarank(score, label, off, norm=False)
        assert invalid == 0
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(wg)) and np.array_equal(_bits(h.cpu().numpy()), _bits(wh)), (kind, lens)


def test_objective_refuses_bad_queries(gpu_device):
    import torch
    rng = np.random.default_rng(3)
    n = gbdt.MAX_QUERY + 1 + 40
    score, label = rng.standard_normal(n), (rng.random(n) < 0.3).astype(np.int32)
    # an oversize query between two valid ones; a non-monotone query_off whose valid queries (rows 0..29, and an empty
    # one) share no row, so that no two workgroups write the same row
    for off in (np.array([0, 20, 20 + gbdt.MAX_QUERY + 1, n]), np.array([0, 30, 20, 20, n])):
        off = off.astype(np.int64)
        out = (torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device), torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device))
        with pytest.raises(_lib.OttoError, match='quer'):
            gbdt.lambdarank_gradients(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), norm=False, out=out)
        wg, wh, invalid = gr.lambdarank(score, label, off, norm=False)
        assert invalid >= 1
        assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(wg)) and np.array_equal(_bits(out[1].cpu().numpy()), _bits(wh))
        with pytest.raises(_lib.OttoError, match='quer'):
            gbdt.ap_at_k(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), k=5)


def test_objective_with_norm(gpu_device):
    """The one place SPEC-GBDT is not bit-exact: the order of S and the device log2. Largest relative difference seen on
    an MI355X: see DESIGN.md section 3g."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for kind in ('random', 'tied_scores', 'graded', 'all_scores_equal'):
        score, label, off = _objective_case(rng, OBJECTIVE_LENS, kind)
        g, h = gbdt.lambdarank_gradients(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), norm=True)
        wg, wh, _ = gr.lambdarank(score, label, off, norm=True)
        for got, want in ((g.cpu().numpy(), wg), (h.cpu().numpy(), wh)):
            nz = want != 0
            assert np.array_equal(got == 0, want == 0)
            worst = max(worst, float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0)
            assert np.allclose(got, want, rtol=1e-12, atol=0), kind
    print(f'lambdarank norm=True: largest relative difference {worst:.3e}')


# ---- quantise

def test_quantise(gpu_device):
    rng = np.random.default_rng(4)
    cases = [(np.zeros(100), np.zeros(100)),                                         # maximum 0
             (rng.standard_normal(1000) * 1e-3, np.zeros(1000)),
             (np.array([0.25, -0.5, 0.125, 0.5 - 2.0 ** -40]), np.array([1.0, 0.5, 2.0, 0.0])),   # maxima at powers of two
             (np.array([1.0 - 2.0 ** -53] + [(2 * k + 1) * 2.0 ** -31 for k in range(-6, 6)]),     # half-way values, both parities
              np.array([0.5] + [(2 * k + 1) * 2.0 ** -31 for k in range(0, 12)])),
             (rng.standard_normal(70001), rng.random(70001) * 3e-7)]
    for grad, hess in cases:
        gh, exp = gbdt.quantize_gradients(_t(grad, gpu_device), _t(hess, gpu_device))
        wq, wexp = gr.quantize(grad, hess)
        assert exp.cpu().numpy().tolist() == list(wexp)
        assert np.array_equal(gh.cpu().numpy(), wq)
    assert wq.dtype == np.int32 and np.abs(wq[:, 0]).max() >= 2 ** 29


# ---- histogram

@pytest.mark.parametrize('F', [1, 54, 128])
def test_histogram(gpu_device, F):
    rng = np.random.default_rng(100 + F)
    n = 30000
    bins = rng.integers(0, 256, (F, n)).astype(np.uint8)
    bins[0, :] = 17                                                # all rows in one bin
    if F > 1:
        bins[1, :] = 255                                           # all rows NaN
    q = rng.integers(-(2 ** 30), 2 ** 30, (n, 2)).astype(np.int32)
    q[:, 1] = np.abs(q[:, 1])
    dbins, dq = _t(bins, gpu_device), _t(q, gpu_device)
    for m in (1, 255, 256, 257, 20000):
        rows = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
        got = gbdt.leaf_histogram(dbins, dq, _t(rows, gpu_device))
        assert np.array_equal(got.cpu().numpy(), gr.histogram(bins, q, rows)), (F, m)
        again = gbdt.leaf_histogram(dbins, dq, _t(rows, gpu_device))
        assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    # every row at +-(2^30 - 1): the sums leave 32 bits after two rows
    for sign in (1, -1):
        q2 = np.full((n, 2), 2 ** 30 - 1, dtype=np.int32)
        q2[:, 0] *= sign
        rows = np.arange(20000, dtype=np.int32)
        got = gbdt.leaf_histogram(dbins, _t(q2, gpu_device), _t(rows, gpu_device)).cpu().numpy()
        assert np.array_equal(got, gr.histogram(bins, q2, rows))
        assert abs(int(got[0, 0, 17])) == 20000 * (2 ** 30 - 1)
    with pytest.raises(_lib.OttoError, match='row id'):
        gbdt.leaf_histogram(dbins, dq, _t(np.array([0, n, 5], dtype=np.int32), gpu_device))


# ---- best split

def _split_both(hist, edge_counts, exps, *args, dev):
    mapper = _mapper([np.arange(c, dtype=np.float32) for c in edge_counts])
    got = gbdt.best_split(_t(hist, dev), mapper, _t(np.array(exps, dtype=np.int32), dev), *args)
    want = gr.best_split(hist, edge_counts, exps, *args)
    assert (got is None) == (want is None), (got, want)
    if want is not None:
        assert {k: v for k, v in got.items() if k != 'gain'} == {k: v for k, v in want.items() if k != 'gain'}
        assert np.float64(got['gain']).view(np.uint64) == np.float64(want['gain']).view(np.uint64)
    return want


def test_best_split(gpu_device):
    exps = (20, 21)
    one = 1 << 21                                                  # H = 1.0 per row
    hist = np.zeros((3, 3, 256), dtype=np.int64)
    # feature 0: 5 rows in bin 0, 7 in bin 1; feature 1: the same split by a NaN bin; feature 2: a copy of feature 0
    hist[:, 0, 0], hist[:, 0, 1] = (-5 << 20, 5 * one, 5), (7 << 20, 7 * one, 7)
    hist[:, 1, 3], hist[:, 1, 255] = (7 << 20, 7 * one, 7), (-5 << 20, 5 * one, 5)
    hist[:, 2] = hist[:, 0]
    base = (0.0, 0.01, 1e-5)
    for min_data, found in ((5, True), (6, False)):               # the smaller side holds exactly 5 rows
        w = _split_both(hist, [1, 4, 1], exps, min_data, *base, dev=gpu_device)
        assert (w is not None) == found
    for min_hess, found in ((5.0, True), (np.nextafter(5.0, 6.0), False)):     # ... and H = 5.0 exactly
        w = _split_both(hist, [1, 4, 1], exps, 1, min_hess, 0.01, 1e-5, dev=gpu_device)
        assert (w is not None) == found
    # equal gains on features 0, 1 (NaN-left) and 2: the smallest feature wins; without feature 0's edge, NaN-left wins
    w = _split_both(hist, [1, 4, 1], exps, 1, *base, dev=gpu_device)
    assert (w['feature'], w['bin'], w['default_left']) == (0, 0, 0)
    h2 = hist.copy()
    h2[:, 0] = 0
    h2[:, 0, 9] = (2 << 20, 12 * one, 12)                          # feature 0: a single bin holds every row
    w = _split_both(h2, [12, 4, 1], exps, 1, *base, dev=gpu_device)
    assert (w['feature'], w['default_left']) == (1, 1) and w['bin'] == 0
    # ties across bins: empty bins between the two groups give the same gain at every edge in between
    h3 = np.zeros((3, 1, 256), dtype=np.int64)
    h3[:, 0, 2], h3[:, 0, 200] = (-3 << 20, 4 * one, 4), (9 << 20, 6 * one, 6)
    w = _split_both(h3, [254], exps, 1, *base, dev=gpu_device)
    assert (w['bin'], w['default_left']) == (2, 0)
    # no edge at all, and min_gain_to_split above every gain
    assert _split_both(h3, [0], exps, 1, *base, dev=gpu_device) is None
    assert _split_both(h3, [254], exps, 1, 0.0, 0.01, 1e9, dev=gpu_device) is None
    # random histograms
    rng = np.random.default_rng(6)
    for F in (1, 5, 54):
        rows = rng.integers(0, 40, (F, 256))
        rows[:, 255] = rng.integers(0, 200, F)
        # one leaf: every feature's bins hold the same rows in all -- spread feature 0's totals anew per feature
        g = rng.integers(-2 ** 30, 2 ** 30, 3000)
        hh = rng.integers(0, 2 ** 30, 3000)
        hist = np.zeros((3, F, 256), dtype=np.int64)
        for f in range(F):
            b = rng.integers(0, 256, 3000)
            b[rng.random(3000) < 0.1] = 255
            np.add.at(hist[0, f], b, g); np.add.at(hist[1, f], b, hh); np.add.at(hist[2, f], b, 1)
        assert _split_both(hist, list(rng.integers(0, 255, F)), (28, 29), 20, 1e-3, 0.01, 1e-5, dev=gpu_device) is not None


# ---- partition

def test_partition(gpu_device):
    rng = np.random.default_rng(9)
    n, F = 50000, 3
    bins = rng.integers(0, 256, (F, n)).astype(np.uint8)
    bins[1, rng.random(n) < 0.3] = 255
    dbins = _t(bins, gpu_device)
    for m in (1, 255, 2048, 2049, 30000):
        rows = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
        for f, b, dl in ((0, 100, 0), (1, 7, 1), (1, 253, 0), (2, 0, 1)):
            out, n_left = gbdt.partition_rows(dbins, _t(rows, gpu_device), f, b, dl)
            wl, wr = gr.partition(bins, rows, f, b, dl)
            assert n_left == wl.size
            assert np.array_equal(out.cpu().numpy(), np.concatenate([wl, wr])), (m, f, b, dl)


# ---- training

def _problem(seed=21, n_queries=200, F=8, **kw):
    rng = np.random.default_rng(seed)
    X, label, off = gr.random_problem(rng, n_queries, F, **kw)
    mapper = gbdt.fit_bins(X)
    edge_list = [mapper.feature_edges(f) for f in range(F)]
    return X, label, off, mapper, edge_list, gr.bin_rows(X, edge_list)


_PROBLEM = {}


def _shared_problem():
    if not _PROBLEM:
        _PROBLEM['p'] = _problem()
    return _PROBLEM['p']


def _train_both(problem, params, dev, rounds=5, check_restatement=True):
    X, label, off, mapper, edge_list, bins_np = problem
    dX = _t(X, dev)
    bins = gbdt.bin_matrix(dX, mapper)
    assert np.array_equal(bins.cpu().numpy(), bins_np)
    res = gbdt.train(bins, _t(label, dev), _t(off, dev), mapper, params, num_boost_round=rounds, keep_leaves=True)
    # the scorer routes the raw float32 rows as the trainer partitioned their bins, and adds the same float64 sums
    assert np.array_equal(forest_leaves(res.forest, dX).cpu().numpy(), res.train_leaf.cpu().numpy())
    assert np.array_equal(_bits(forest_predict(res.forest, dX).cpu().numpy()), _bits(res.train_score.cpu().numpy()))
    if check_restatement:
        want = gr.train(bins_np, label, off, edge_list, params, num_boost_round=rounds)
        assert res.best_iteration == want['best_iteration'] == len(res.trees)
        for t, (got, w) in enumerate(zip(res.trees, want['trees'])):
            for k in ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'decision_type', 'leaf_count'):
                assert np.array_equal(getattr(got, k), w[k]), (t, k)
            for k in ('threshold', 'split_gain', 'leaf_value'):
                assert np.array_equal(_bits(getattr(got, k)), _bits(w[k])), (t, k)
        assert np.array_equal(res.train_leaf.cpu().numpy(), want['train_leaf'])
        assert np.array_equal(_bits(res.train_score.cpu().numpy()), _bits(want['train_score']))
    return res


@pytest.mark.parametrize('num_leaves', [2, 31, 128])
@pytest.mark.parametrize('min_data', [1, 20])
def test_training_without_norm_is_bit_exact(gpu_device, num_leaves, min_data):
    res = _train_both(_shared_problem(), dict(num_leaves=num_leaves, min_data_in_leaf=min_data, lambdarank_norm=False), gpu_device)
    # with min_data_in_leaf = 20 the 5,116 rows run out of admissible splits before 128 leaves
    assert len(res.trees) == 5 and (res.trees[0].n_leaves == num_leaves or (min_data, num_leaves) == (20, 128))


def test_training_that_cannot_reach_num_leaves(gpu_device):
    n = _shared_problem()[0].shape[0]
    res = _train_both(_shared_problem(), dict(num_leaves=128, min_data_in_leaf=n // 12, lambdarank_norm=False), gpu_device)
    assert all(2 <= t.n_leaves < 128 for t in res.trees)


def test_training_ends_at_a_single_leaf_tree(gpu_device):
    # column 0 is the label itself: one split separates the classes, full Newton steps (learning_rate 1) shrink the
    # gradients tree by tree until no split gains min_gain_to_split, and that one-leaf tree ends the training
    rng = np.random.default_rng(5)
    X, label, off = gr.random_problem(rng, 60, 2, nan_share=0.0)
    X[:, 0], X[:, 1] = label, np.round(X[:, 1])
    mapper = gbdt.fit_bins(X)
    edge_list = [mapper.feature_edges(f) for f in range(2)]
    problem = (X, label, off, mapper, edge_list, gr.bin_rows(X, edge_list))
    params = dict(num_leaves=4, min_data_in_leaf=20, lambdarank_norm=False, learning_rate=1.0, min_gain_to_split=0.1)
    want = gr.train(problem[5], label, off, edge_list, params, num_boost_round=50)
    assert 2 <= len(want['trees']) < 50                            # the restatement stopped on a one-leaf tree
    res = _train_both(problem, params, gpu_device, rounds=50)
    assert len(res.trees) == len(want['trees'])
    with pytest.raises(_lib.OttoError, match='no tree'):           # min_data_in_leaf > n / 2: not even a first tree
        gbdt.train(gbdt.bin_matrix(_t(X, gpu_device), mapper), _t(label, gpu_device), _t(off, gpu_device), mapper,
                   dict(num_leaves=4, min_data_in_leaf=X.shape[0] // 2 + 1), num_boost_round=3)


def test_training_with_norm_keeps_the_invariants(gpu_device):
    res = _train_both(_shared_problem(), dict(num_leaves=31, min_data_in_leaf=20, lambdarank_norm=True), gpu_device,
                      check_restatement=False)
    assert len(res.trees) == 5


# ---- AP@k and early stopping

def test_ap_at_k_is_bit_exact(gpu_device):
    rng = np.random.default_rng(12)
    score, label, off = _objective_case(rng, [1, 2, 5, 19, 20, 21, 49, 50, 51, 300, 0, 7], 'tied_scores')
    label[off[2]:off[3]] = 0                                       # a query without a positive
    for k in (1, 20, 50):
        got = gbdt.ap_at_k(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), k=k).cpu().numpy()
        want, invalid = gr.ap_at_k(score, label, off, k)
        assert invalid == 0 and (want == -1).any() and ((want > 0).any() or k == 1)
        assert np.array_equal(_bits(got), _bits(want)), k
        assert gbdt.mean_ap(got) == gr.mean_ap(want)


def test_early_stopping_matches_the_restatement(gpu_device):
    from test_gbdt_cpu import early_stopping_case
    c = early_stopping_case()
    mapper = _mapper(c['edges'])
    dev = gpu_device
    bins, vbins = gbdt.bin_matrix(_t(c['X'], dev), mapper), gbdt.bin_matrix(_t(c['Xv'], dev), mapper)
    res = gbdt.train(bins, _t(c['label'], dev), _t(c['query_off'], dev), mapper, c['params'],
                     valid=(vbins, _t(c['vlabel'], dev), _t(c['voff'], dev)), num_boost_round=30,
                     early_stopping_rounds=c['early_stopping_rounds'])
    want = c['restated']
    assert res.best_iteration == want['best_iteration'] and res.forest.n_trees == want['best_iteration']
    assert res.history == want['history']
    wf = gr.to_forest(want['trees'], 3)
    for k in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value'):
        assert np.array_equal(getattr(res.forest, k), getattr(wf, k)), k
    assert np.array_equal(_bits(res.train_score.cpu().numpy()), _bits(want['train_score']))


# ---- chain

def test_chain_from_matrix_to_ranked_candidates(gpu_device):
    import torch
    rng = np.random.default_rng(30)
    X, label, off = gr.random_problem(rng, 150, 54, min_len=10, max_len=30)
    dX = _t(X, gpu_device)
    mapper = gbdt.fit_bins(X[::3])
    bins = gbdt.bin_matrix(dX, mapper)
    res = gbdt.train(bins, _t(label, gpu_device), _t(off, gpu_device), mapper,
                     {'num_leaves': 16, 'min_data_in_leaf': 30, 'learning_rate': 0.1, 'seed': 42, 'verbose': -1, 'metric': 'map'},
                     num_boost_round=4)
    assert res.forest.n_trees == res.best_iteration == 4 and res.history == [] and res.train_score.shape == (X.shape[0],)
    aid = torch.arange(X.shape[0], dtype=torch.int32, device=gpu_device)
    top_aid, top_score, n = rank_candidates([res.forest], dX, aid, _t(off, gpu_device), k=20)
    S = off.size - 1
    assert top_aid.shape == (S, 20) and top_score.shape == (S, 20) and n.shape == (S,)
    assert np.array_equal(n.cpu().numpy(), np.minimum(np.diff(off), 20))
    text = gbdt.write_lightgbm_model(res.forest)
    from otto_amd.ranker.forest import parse_lightgbm_model
    assert np.array_equal(parse_lightgbm_model(text).leaf_value, res.forest.leaf_value)
