"""SPEC-XGB on the device against tests/xgb_restatement.py: the rank:pairwise objective, the level launches (histogram,
split search, partition), whole depth-wise trees, trainings, the JSON model and the fold trainer. Every comparison is bit
for bit. The problems and their references come from tests/xgb_inputs.py (each reference is computed once), whose shapes
tests/test_xgb_cpu.py proves."""
import numpy as np
import pytest

import folds_restatement as fr
import gbdt_restatement as gr
import gbdt_sampling_restatement as sr
import xgb_inputs as xi
import xgb_restatement as xr
from otto_amd import _lib
from otto_amd.ranker import folds, gbdt, xgb
from otto_amd.ranker.forest import forest_predict

pytestmark = pytest.mark.gpu

TREE_INT = ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'decision_type', 'count', 'left_id', 'right_id',
            'leaf_count')
TREE_FLOAT = ('threshold', 'split_gain', 'cover', 'sum_grad', 'leaf_value', 'leaf_cover', 'leaf_sum_grad')
FOREST_ARRAYS = ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value')


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


def _same_tree(got, want, where):
    for k in TREE_INT:
        assert np.array_equal(getattr(got, k), want[k]), (where, k)
    for k in TREE_FLOAT:
        assert np.array_equal(_bits(getattr(got, k)), _bits(want[k])), (where, k)
    assert got.hist_rows == want['hist_rows'], where


def _gradients(case, dev, it=0, out=None):
    score, label, off = case
    g, h = xgb.pairwise_gradients(_t(score, dev), _t(label, dev), _t(off, dev), xi.OBJECTIVE_SEED, it, out=out)
    return g.cpu().numpy(), h.cpu().numpy()


# ---- objective

def test_objective_at_every_query_size(gpu_device):
    g, h = _gradients(xi.objective_sizes(), gpu_device)
    wg, wh, invalid, bad = xi.objective_want('sizes')
    assert invalid == 0 and not bad and wg.any()
    assert np.array_equal(_bits(g), _bits(wg)) and np.array_equal(_bits(h), _bits(wh))


def test_objective_at_the_edge_between_the_two_kernels(gpu_device):
    g, h = _gradients(xi.objective_edge(), gpu_device)
    wg, wh, invalid, bad = xi.objective_want('edge')
    assert invalid == 0 and not bad
    assert np.array_equal(_bits(g), _bits(wg)) and np.array_equal(_bits(h), _bits(wh))
    off = xi.objective_edge()[2]
    assert all(wg[a:b].any() for a, b in zip(off[:-1], off[1:]) if b - a > 1)


@pytest.mark.parametrize('kind', xi.OBJECTIVE_KINDS)
def test_objective_input_kinds(gpu_device, kind):
    g, h = _gradients(xi.objective_kind(kind), gpu_device)
    wg, wh, invalid, bad = xi.objective_want(kind)
    assert invalid == 0 and not bad
    assert np.array_equal(_bits(g), _bits(wg)) and np.array_equal(_bits(h), _bits(wh))
    assert not np.isnan(g).any() and not np.isnan(h).any()
    if kind == 'all_equal_labels':
        assert not g.any() and not h.any()


def test_objective_iterations(gpu_device):
    case = xi.objective_kind('random')
    a0, b0 = _gradients(case, gpu_device, it=0)
    a1, b1 = _gradients(case, gpu_device, it=1)
    again = _gradients(case, gpu_device, it=1)
    assert not np.array_equal(a0, a1)
    assert np.array_equal(_bits(a1), _bits(again[0])) and np.array_equal(_bits(b1), _bits(again[1]))
    wg, wh, _, _ = xi.objective_want('random', 1)
    assert np.array_equal(_bits(a1), _bits(wg)) and np.array_equal(_bits(b1), _bits(wh))


def test_objective_refuses_bad_queries_and_labels(gpu_device):
    import torch
    rng = np.random.default_rng(3)
    n = gbdt.MAX_QUERY + 1 + 40
    score, label = rng.standard_normal(n), rng.integers(0, 3, n).astype(np.int32)

    def run(label, off, match):
        out = (torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device), torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device))
        with pytest.raises(_lib.OttoError, match=match):
            xgb.pairwise_gradients(_t(score, gpu_device), _t(label, gpu_device), _t(off.astype(np.int64), gpu_device), xi.OBJECTIVE_SEED,
                                   0, out=out)
        wg, wh, invalid, bad = xr.pairwise(score, label, off, xi.OBJECTIVE_SEED, 0)
        assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(wg)) and np.array_equal(_bits(out[1].cpu().numpy()), _bits(wh))
        return wg, invalid, bad
    # a query of 1025 rows between two valid ones; descending offsets whose valid queries share no row
    for off in (np.array([0, 20, 20 + gbdt.MAX_QUERY + 1, n]), np.array([0, 30, 20, 20, n])):
        wg, invalid, bad = run(label, off, 'quer')
        assert invalid >= 1 and not bad and wg[:20].any()
    # a label of 32 and a label of -1, each in the second of three queries: the other queries stay exact
    off = np.array([0, 30, 70, 100, n])
    for wrong in (32, -1):
        lab = label.copy()
        lab[45] = wrong
        wg, invalid, bad = run(lab, off, 'label')
        assert invalid == 0 and bad and wg[:30].any() and wg[70:].any()


# ---- level launches

def _nodes(rows):
    return np.array(rows, dtype=np.int32).reshape(-1, 8)


@pytest.mark.parametrize('F', [1, 54, 128])
def test_level_histogram(gpu_device, F):
    d = xi.level_problem(F)
    bins, gh, rows = _t(d['bins'], gpu_device), _t(d['q'], gpu_device), _t(d['rows'], gpu_device)
    segs = xi.segments(xi.HIST_SEGMENTS)
    lists = [None] + [np.sort(np.random.default_rng(k).choice(F, k, replace=False)).astype(np.int32) for k in (1, 8, 9) if k <= F]
    for feats in lists:
        nodes = _nodes([[b, c, slot, -1, 0, 0, 0, 0] for slot, (b, c) in enumerate(segs)])
        hist = xgb.level_histograms(bins, gh, rows, nodes, len(segs) + 1, features=feats)
        got = hist.cpu().numpy()
        for slot, (b, c) in enumerate(segs):
            assert np.array_equal(got[slot], sr.histogram(d['bins'], d['q'], d['rows'][b:b + c], feats)), (F, feats, slot)
        assert not got[len(segs)].any()
        # the 5000-row node splits 2049 : 2951: the smaller child is built into the free slot, the larger one is what the
        # subtraction leaves in the parent's slot
        b, c = segs[-1]
        child = _nodes([[b, 2049, len(segs), len(segs) - 1, 0, 0, 0, 0]])
        got = xgb.level_histograms(bins, gh, rows, child, len(segs) + 1, features=feats, hist=hist).cpu().numpy()
        assert np.array_equal(got[len(segs)], sr.histogram(d['bins'], d['q'], d['rows'][b:b + 2049], feats))
        assert np.array_equal(got[len(segs) - 1], sr.histogram(d['bins'], d['q'], d['rows'][b + 2049:b + c], feats))
        assert np.array_equal(got[0], sr.histogram(d['bins'], d['q'], d['rows'][segs[0][0]:segs[0][0] + 1], feats))


def test_level_split_search(gpu_device):
    d = xi.grow_problem()
    dev = gpu_device
    bins, gh = _t(d['bins'], dev), _t(d['q'], dev)
    mapper = _mapper(d['edge_list'])
    exp = _t(np.array(d['exps'], dtype=np.int32), dev)
    rows = np.arange(xi.GROW_N, dtype=np.int32)
    segs = [(0, 7000), (7000, 1), (7001, 12999)]
    nodes = _nodes([[b, c, 2 - i, -1, 0, 0, 0, 0] for i, (b, c) in enumerate(segs)])      # slots in another order than the nodes
    n_edges = [len(e) for e in d['edge_list']]
    for feats in (None, xi.GROW_FEATURES):
        hist = xgb.level_histograms(bins, gh, _t(rows, dev), nodes, 3, features=feats)
        for mcw, gamma in ((1.0, 0.0), (0.0, 0.0), (1.0, 50.0)):
            rec = xgb.level_splits(hist, mapper, exp, nodes, mcw, 1.0, gamma, features=feats)
            for i, (b, c) in enumerate(segs):
                h = sr.histogram(d['bins'], d['q'], rows[b:b + c], feats)
                want = sr.best_split(h, n_edges, d['exps'], 0, mcw, 1.0, gamma, features=feats)
                assert bool(rec[i, 0]) == (want is not None), (i, mcw, gamma)
                assert rec[i, 8] == c
                if want is not None:
                    assert [int(x) for x in rec[i, [1, 2, 3, 5, 6, 7, 8, 9, 10]]] == [want[k] for k in (
                        'feature', 'bin', 'default_left', 'cnt_left', 'g_left', 'h_left', 'cnt', 'g', 'h')]
                    assert rec[i, 4:5].view(np.float64)[0] == want['gain']


def test_level_partition(gpu_device):
    d = xi.level_problem(54)
    bins, rows = _t(d['bins'], gpu_device), _t(d['rows'], gpu_device)
    segs = xi.segments(xi.PART_SEGMENTS)
    b = d['bins']
    # (feature, bin, default_left): ordinary splits; the last three: all left (bin 253, NaN left), all right (a feature made
    # to hold bin 200 on the segment), and one whose only movers are the NaN rows (bin 253: default_left decides)
    splits = [(f, 20, f & 1) for f in range(len(segs) - 3)] + [(50, 253, 1), (51, 100, 0), (52, 253, 0)]
    seg = segs[-2]
    bins[51, rows[seg[0]:seg[0] + seg[1]].long()] = 200
    b = bins.cpu().numpy()
    nodes = _nodes([[s[0], s[1], 0, -1, 0, f, sb, dl] for s, (f, sb, dl) in zip(segs, splits)])
    out, n_left = xgb.level_partition(bins, rows, nodes)
    out = out.cpu().numpy()
    want = d['rows'].copy()
    for i, ((s0, c), (f, sb, dl)) in enumerate(zip(segs, splits)):
        left, right = gr.partition(b, d['rows'][s0:s0 + c], f, sb, dl)
        want[s0:s0 + c] = np.concatenate([left, right])
        assert n_left[i] == left.size, i
    assert np.array_equal(out, want)                        # row for row, and nothing outside the segments moved
    assert n_left[-3] == segs[-3][1] and n_left[-2] == 0 and 0 < n_left[-1] < segs[-1][1]
    nan_rows = d['rows'][segs[-1][0]:segs[-1][0] + segs[-1][1]]
    assert (b[52, nan_rows] == gr.NAN_BIN).sum() == segs[-1][1] - n_left[-1]


# ---- growth

@pytest.mark.parametrize('name', list(xi.GROW_CASES))
def test_grow_tree(gpu_device, name):
    d = xi.grow_problem()
    dev = gpu_device
    _, bag, feats = xi.GROW_CASES[name]
    p = xi.grow_params(name)
    tree = xgb.grow_tree(_t(d['bins'], dev), _t(d['q'], dev), _t(np.array(d['exps'], dtype=np.int32), dev), _mapper(d['edge_list']), p,
                         bag=_t(d['bag'], dev) if bag else None, features=xi.GROW_FEATURES if feats else None)
    want = xi.grow_want(name)
    assert tree.n_leaves == want['leaf_value'].size
    _same_tree(tree, want, name)
    # float32-rounded leaf values; one synchronisation per level (and one for a feature list), none per node
    assert np.array_equal(tree.leaf_value, tree.leaf_value.astype(np.float32).astype(np.float64))
    assert tree.n_syncs == want['n_levels'] + (1 if feats else 0) <= p['max_depth'] + 2
    # the tree routes every in-bag row to the leaf the restatement put it in
    score = _t(np.zeros(xi.GROW_N), dev)
    leaf = gbdt.add_tree(_t(d['bins'], dev), tree, score, want_leaf=True).cpu().numpy()
    for i, r in enumerate(want['leaf_rows']):
        assert (leaf[r] == i).all()


def test_grow_tree_refuses_bad_arguments(gpu_device):
    d = xi.grow_problem()
    dev = gpu_device
    bins, gh, exp = _t(d['bins'], dev), _t(d['q'], dev), _t(np.array(d['exps'], dtype=np.int32), dev)
    mapper = _mapper(d['edge_list'])
    for bad in ({'max_depth': 0}, {'max_depth': 11}):
        with pytest.raises(ValueError, match='max_depth'):
            xgb.grow_tree(bins, gh, exp, mapper, dict(xi.BASE, **bad))
    with pytest.raises(_lib.OttoError, match='gamma'):
        xgb.grow_tree(bins, gh, exp, mapper, dict(xi.BASE, gamma=-1.0))
    bag = d['bag'].copy()
    bag[5] = xi.GROW_N                                      # a row id outside [0, n)
    with pytest.raises(_lib.OttoError, match='row id'):
        xgb.grow_tree(bins, gh, exp, mapper, xi.BASE, bag=_t(bag, dev))
    import torch
    with pytest.raises(_lib.OttoError, match='d_work'):
        xgb.grow_tree(bins, gh, exp, mapper, xi.BASE, work=torch.empty(1024, dtype=torch.uint8, device=dev))
    assert _lib.lib().otto_xgb_workspace_bytes(100, 8, 0) == 0 and _lib.lib().otto_xgb_workspace_bytes(100, 8, 11) == 0
    # the resident histograms of the deepest searched level: 2^(max_depth-1) * 3 * F * 256 * 8 bytes
    assert xgb.workspace_bytes(100, 54, 10) - xgb.workspace_bytes(100, 54, 9) == 256 * 3 * 54 * 256 * 8


# ---- training

def _train(name, dev):
    d, c = xi.train_problem(), xi.TRAIN_CASES[name]
    mapper = _mapper(d['edge_list'])
    dX = _t(d['X'], dev)
    bins = gbdt.bin_matrix(dX, mapper)
    assert np.array_equal(bins.cpu().numpy(), d['bins'])
    valid = (gbdt.bin_matrix(_t(d['Xv'], dev), mapper), _t(d['vlabel'], dev), _t(d['voff'], dev))
    res = xgb.train(bins, _t(d['label'], dev), _t(d['query_off'], dev), mapper, c['params'], valid=valid,
                    num_boost_round=c['rounds'], early_stopping_rounds=c['early'])
    return d, c, dX, res


@pytest.mark.parametrize('name', list(xi.TRAIN_CASES))
def test_training_equals_the_restatement(gpu_device, name):
    d, c, dX, res = _train(name, gpu_device)
    want = xi.train_want(name)
    assert res.best_iteration == want['best_iteration'] == len(res.trees) and res.history == want['history']
    assert res.base_score == want['base_score'] == 0.5 and res.forest.objective == 'rank:pairwise'
    for t, (got, w) in enumerate(zip(res.trees, want['trees'])):
        _same_tree(got, w, (name, t))
    wf = gr.to_forest(want['trees'], xi.TRAIN_F)
    for k in FOREST_ARRAYS:
        assert np.array_equal(getattr(res.forest, k), getattr(wf, k)), k
    train_score = res.train_score.cpu().numpy()
    assert np.array_equal(_bits(train_score), _bits(want['train_score']))
    # the forest scorer over the float32 matrix gives the trainer's own scores, and so does the model read back from JSON
    assert np.array_equal(_bits(xgb.predict(res, dX).cpu().numpy()), _bits(train_score))
    model = xgb.parse_xgboost_json(xgb.write_xgboost_json(res, params=c['params']))
    for k in FOREST_ARRAYS:
        a, b = getattr(model.forest, k), getattr(res.forest, k)
        # an edge of -0.0 comes back as +0.0 (nextafter32 of either zero is the same condition): equal, and it routes alike
        assert a.dtype == b.dtype and (np.array_equal(a, b) if k == 'threshold' else a.tobytes() == b.tobytes()), k
    assert np.array_equal(_bits(xgb.predict(model, dX).cpu().numpy()), _bits(train_score))
    assert np.array_equal(_bits(forest_predict(res.forest, dX).cpu().numpy() + 0.5), _bits(train_score))
    if c['early']:
        assert res.best_iteration < len(res.history)        # the cut happened
    gain, weight, cover = xgb.feature_importance(res.trees, xi.TRAIN_F)
    wgain, wweight, wcover = xr.feature_importance(want['trees'], xi.TRAIN_F)
    assert np.array_equal(weight, wweight) and np.allclose(gain, wgain, rtol=1e-12) and np.allclose(cover, wcover, rtol=1e-12)


# ---- the fold trainer

def _fold_problem():
    rng = np.random.default_rng(402)
    sizes = rng.integers(20, 41, 200)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, F = int(off[-1]), 6
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[rng.random((n, F)) < 0.02] = np.nan
    label = np.zeros(n, dtype=np.uint8)
    for q in range(200):
        a, b = off[q], off[q + 1]
        if rng.random() >= 0.15:
            label[a + int(np.argmax(X[a:b, 0] - 0.5 * np.nan_to_num(X[a:b, 1]) + 0.5 * rng.standard_normal(b - a)))] = 1
    return X, label, off


def test_cross_validate_with_the_xgboost_booster(gpu_device):
    X, label, off = _fold_problem()
    n, F = X.shape
    params = {'max_depth': 3, 'eta': 0.3, 'subsample': 0.8, 'colsample_bytree': 0.5, 'seed': 42, 'objective': 'rank:pairwise',
              'eval_metric': 'map', 'tree_method': 'gpu_hist', 'nthread': 4}
    dX, doff = _t(X, gpu_device), _t(off, gpu_device)
    res = folds.cross_validate(dX, _t(label, gpu_device), doff, params, n_splits=3, negative_sampling_ratio=0.5, seed=42,
                               num_boost_round=5, early_stopping_rounds=2, booster='xgboost')
    fold_of_query, _ = fr.group_kfold(off, 3)
    assert np.array_equal(res.fold_of_query.cpu().numpy(), fold_of_query)
    oof = np.zeros(n, dtype=np.float32)
    for fold in range(3):
        s = fr.fold_indices(label, off, fold_of_query, fold, 0.5, 42)
        mapper = gbdt.fit_bins(X[s['train_idx']])
        edge_list = [mapper.feature_edges(f) for f in range(F)]
        bins = gr.bin_rows(X, edge_list)
        t_bins, v_bins = bins[:, s['train_idx']], bins[:, s['val_idx']]
        want = xr.train(t_bins, label[s['train_idx']].astype(np.int32), s['train_query_off'], edge_list,
                        {k: params[k] for k in ('max_depth', 'eta', 'subsample', 'colsample_bytree', 'seed')},
                        valid=(v_bins, label[s['val_idx']].astype(np.int32), s['val_query_off']), num_boost_round=5,
                        early_stopping_rounds=2)
        wf = gr.to_forest(want['trees'], F)
        for name in FOREST_ARRAYS:
            assert np.array_equal(getattr(res.forests[fold], name), getattr(wf, name)), (fold, name)
        assert res.best_iterations[fold] == want['best_iteration'] and res.histories[fold] == want['history']
        oof[s['val_idx']] = xr.predict_bins(v_bins, want['trees'], 0.5).astype(np.float32)
        gain, weight, cover = xr.feature_importance(want['trees'], F)
        assert np.array_equal(res.importance_split[:, fold], weight)
        assert np.allclose(res.importance_gain[:, fold], gain, rtol=1e-12) and np.allclose(res.importance_cover[:, fold], cover, rtol=1e-12)
    assert np.array_equal(res.oof_prediction.cpu().numpy().view(np.uint32), oof.view(np.uint32))


def test_cross_validate_lightgbm_is_the_default(gpu_device):
    X, label, off = _fold_problem()
    params = {'num_leaves': 8, 'min_data_in_leaf': 20, 'learning_rate': 0.1, 'lambdarank_norm': False}
    args = (_t(X, gpu_device), _t(label, gpu_device), _t(off, gpu_device), params)
    kw = dict(n_splits=3, negative_sampling_ratio=0.5, seed=42, num_boost_round=4, early_stopping_rounds=2)
    a = folds.cross_validate(*args, **kw)
    b = folds.cross_validate(*args, booster='lightgbm', **kw)
    assert a.importance_cover is None and b.importance_cover is None
    assert np.array_equal(a.oof_prediction.cpu().numpy().view(np.uint32), b.oof_prediction.cpu().numpy().view(np.uint32))
    assert a.best_iterations == b.best_iterations and a.histories == b.histories
    for fa, fb in zip(a.forests, b.forests):
        for name in FOREST_ARRAYS:
            assert getattr(fa, name).tobytes() == getattr(fb, name).tobytes()
    assert np.array_equal(a.importance_gain, b.importance_gain) and np.array_equal(a.importance_split, b.importance_split)
    with pytest.raises(ValueError, match='booster'):
        folds.cross_validate(*args, booster='catboost', **kw)
    with pytest.raises(ValueError, match='sampling'):
        folds.cross_validate(*args, booster='xgboost', sampling=gbdt.Sampling(), **kw)
