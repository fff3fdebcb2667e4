"""The sampling of SPEC-GBDT on the device against tests/gbdt_sampling_restatement.py: the row bag, the histogram and the
split search over a feature list, trees grown on a bag and a list, whole trainings and the fold trainer. Every comparison is
bit for bit; ``lambdarank_norm`` is off wherever floats are compared, as in tests/test_gbdt_gpu.py. The problems come from
tests/gbdt_sampling_inputs.py, whose shapes tests/test_gbdt_sampling_cpu.py proves."""
import numpy as np
import pytest

import folds_restatement as fr
import gbdt_restatement as gr
import gbdt_sampling_inputs as si
import gbdt_sampling_restatement as sr
from otto_amd import _lib
from otto_amd.ranker import folds, gbdt
from otto_amd.ranker.forest import forest_predict

pytestmark = pytest.mark.gpu

TREE_INT = ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'decision_type', 'leaf_count')
TREE_FLOAT = ('threshold', 'split_gain', 'leaf_value')
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


# ---- the row bag

BAG_N = [1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 65537, 2 ** 18 + 3]


@pytest.mark.parametrize('n', BAG_N)
def test_bag_rows(gpu_device, n):
    sizes = sorted({m for m in (1, int(0.5 * n), int(0.9 * n), n - 1, n) if m >= 1})
    for s in (0, 42, 2 ** 64 - 1):
        seed = sr.mix(s, 0)
        keys = fr.keys(seed, np.arange(n))
        order = np.argsort(keys, kind='stable')
        for m in sizes:
            got = gbdt.bag_rows(n, m, seed, gpu_device)
            assert got.shape == (m,)
            got = got.cpu().numpy()
            assert got.dtype == np.int32 and (np.diff(got) > 0).all(), (n, m, s)
            assert np.array_equal(got, np.sort(order[:m])), (n, m, s)
    assert np.array_equal(gbdt.bag_rows(n, sizes[-1], sr.mix(42, 2), gpu_device).cpu().numpy(), sr.bag(n, sizes[-1], sr.mix(42, 2)))


def test_bag_refuses_short_buffers_on_the_host(gpu_device):
    import torch
    n, m = 1000, 500
    need = _lib.lib().otto_gbdt_bag_workspace_bytes(n)
    assert need > 0 and _lib.lib().otto_gbdt_bag_workspace_bytes(0) == 0 and _lib.lib().otto_gbdt_bag_workspace_bytes(2 ** 31) == 0
    out = torch.full((m,), -7, dtype=torch.int32, device=gpu_device)
    work = torch.zeros(need, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.OttoError, match='d_rows_out'):
        _lib.call('otto_gbdt_bag', gpu_device, n, m, 5, out, m - 1, work, need)
    with pytest.raises(_lib.OttoError, match='d_work'):
        _lib.call('otto_gbdt_bag', gpu_device, n, m, 5, out, m, work, need - 1)
    with pytest.raises(_lib.OttoError, match='d_work'):
        _lib.call('otto_gbdt_bag', gpu_device, n, m, 5, out, m, None, need)
    for bad_m in (0, n + 1):
        with pytest.raises(_lib.OttoError, match='m = '):
            _lib.call('otto_gbdt_bag', gpu_device, n, bad_m, 5, out, m, work, need)
    assert (out.cpu().numpy() == -7).all()                          # refused on the host: nothing was launched
    _lib.call('otto_gbdt_bag', gpu_device, n, m, 5, out, m, work, need)
    assert np.array_equal(out.cpu().numpy(), sr.bag(n, m, 5))
    with pytest.raises(ValueError):
        gbdt.bag_rows(n, 0, 5, gpu_device)
    with pytest.raises(ValueError):
        gbdt.bag_rows(n, n + 1, 5, gpu_device)


# ---- histogram and split search over a list

def _feature_lists(F):
    lists = {'one': [F // 2], 'all': list(range(F)), 'last': [F - 1]}
    if F > 1:
        lists['all_but_one'] = [f for f in range(F) if f != F // 3]
        lists['without_0'] = list(range(1, F, 2)) if F > 2 else [1]
    if F == 54:
        lists['9_of_54'] = sr.feature_list(54, 9 / 54, 42, 0).tolist()
        lists['49_of_54'] = sr.feature_list(54, 0.9, 42, 1).tolist()
        assert len(lists['9_of_54']) == 9 and len(lists['49_of_54']) == 49
    return lists


@pytest.mark.parametrize('F', [1, 7, 8, 9, 54])
def test_histogram_and_best_split_over_a_feature_list(gpu_device, F):
    rng = np.random.default_rng(200 + F)
    n = 10000
    # bins that follow a per-feature signal, so that every feature offers a split of its own
    signal = rng.standard_normal(n)
    bins = np.clip(rng.integers(0, 200, (F, n)) + (25 * signal * rng.uniform(0.2, 1.0, (F, 1))).astype(np.int64), 0, 253).astype(np.uint8)
    bins[rng.random((F, n)) < 0.05] = gbdt.NAN_BIN
    grad = -signal + 0.3 * rng.standard_normal(n)
    q, exps = gr.quantize(grad, 0.05 + rng.random(n))
    rows = sr.bag(n, 5000, sr.mix(42, 0))
    n_edges = rng.integers(100, 254, F).tolist()
    mapper = _mapper([np.arange(c, dtype=np.float32) for c in n_edges])
    dbins, dq, drows, dexp = _t(bins, gpu_device), _t(q, gpu_device), _t(rows, gpu_device), _t(np.array(exps, dtype=np.int32), gpu_device)
    args = (20, 1e-3, 0.01, 1e-5)
    full = gr.histogram(bins, q, rows)
    assert np.array_equal(gbdt.leaf_histogram(dbins, dq, drows).cpu().numpy(), full)
    for name, feats in _feature_lists(F).items():
        got = gbdt.leaf_histogram(dbins, dq, drows, features=feats)
        want = sr.histogram(bins, q, rows, feats)
        unused = [f for f in range(F) if f not in feats]
        g = got.cpu().numpy()
        assert np.array_equal(g, want), (F, name)
        assert np.array_equal(g[:, feats], full[:, feats]) and not g[:, unused].any() and g[2, feats].sum() == 5000 * len(feats)
        split = gbdt.best_split(got, mapper, dexp, *args, features=feats)
        wsplit = sr.best_split(want, n_edges, exps, *args, features=feats)
        assert split is not None and wsplit is not None, (F, name)
        assert {k: v for k, v in split.items() if k != 'gain'} == {k: v for k, v in wsplit.items() if k != 'gain'}, (F, name)
        assert np.float64(split['gain']).view(np.uint64) == np.float64(wsplit['gain']).view(np.uint64)
        assert split['feature'] in feats
        # words 8 to 10: the parent's sums, from the first listed plane (plane 0 is all zero when 0 is not listed)
        assert (split['cnt'], split['g'], split['h']) == (5000, int(q[rows, 0].astype(np.int64).sum()), int(q[rows, 1].astype(np.int64).sum()))
        # the split search over the full histogram, restricted to the list, finds the same split
        assert gbdt.best_split(_t(full, gpu_device), mapper, dexp, *args, features=feats) == split
    # a tensor goes in as it is; a list that is not one is refused on both sides of the call
    feats = _t(np.array([F - 1], dtype=np.int32), gpu_device)
    assert np.array_equal(gbdt.leaf_histogram(dbins, dq, drows, features=feats).cpu().numpy(), sr.histogram(bins, q, rows, [F - 1]))
    for bad in ([F], [-1], [0, 0], list(range(F + 1)), []):
        with pytest.raises(ValueError):
            gbdt.leaf_histogram(dbins, dq, drows, features=bad)
        if bad:
            with pytest.raises(_lib.OttoError, match='d_features|n_used'):
                gbdt.leaf_histogram(dbins, dq, drows, features=_t(np.array(bad, dtype=np.int32), gpu_device))
            with pytest.raises(_lib.OttoError, match='d_features|n_used'):
                gbdt.best_split(_t(full, gpu_device), mapper, dexp, *args, features=_t(np.array(bad, dtype=np.int32), gpu_device))


# ---- one tree on a bag and a list

@pytest.mark.parametrize('name', si.TREE_NAMES)
def test_grow_tree_on_a_bag_and_a_feature_list(gpu_device, name):
    c = si.tree_case(name)
    p, want = c['problem'], c['want']
    mapper = _mapper(p['edge_list'])
    dbins, dq = _t(p['bins'], gpu_device), _t(p['q'], gpu_device)
    dexp = _t(np.array(p['exps'], dtype=np.int32), gpu_device)
    bag = None
    if c['bag'] is not None:
        bag = gbdt.bag_rows(p['n'], c['bag'].size, c['bag_seed'], gpu_device)
        assert np.array_equal(bag.cpu().numpy(), c['bag'])
    params = gbdt.resolve_params({k: v for k, v in c['params'].items() if k in gbdt.DEFAULTS})
    tree = gbdt.grow_tree(dbins, dq, dexp, mapper, params, bag=bag, features=c['features'])
    _same_tree(tree, want, name)
    assert tree.n_leaves >= 3 and tree.hist_rows == want['hist_rows']
    assert tree.leaf_count.sum() == (p['n'] if bag is None else bag.numel())
    if c['features'] is not None:
        assert set(tree.split_feature.tolist()) <= set(c['features'].tolist())


def test_grow_tree_refuses_a_bad_bag_or_list(gpu_device):
    c = si.tree_case('f3_both')
    p = c['problem']
    mapper = _mapper(p['edge_list'])
    dbins, dq = _t(p['bins'], gpu_device), _t(p['q'], gpu_device)
    dexp = _t(np.array(p['exps'], dtype=np.int32), gpu_device)
    params = gbdt.resolve_params({'num_leaves': 8, 'min_data_in_leaf': 20})
    bad_bag = c['bag'].copy()
    bad_bag[-1] = p['n']                                            # one row id behind the matrix: skipped, then refused
    with pytest.raises(_lib.OttoError, match='row id'):
        gbdt.grow_tree(dbins, dq, dexp, mapper, params, bag=_t(bad_bag, gpu_device))
    with pytest.raises(_lib.OttoError, match='d_features'):
        gbdt.grow_tree(dbins, dq, dexp, mapper, params, features=_t(np.array([2, 1], dtype=np.int32), gpu_device))
    with pytest.raises(ValueError):
        gbdt.grow_tree(dbins, dq, dexp, mapper, params, features=[0, 3])
    # None / None is the unsampled call
    a = gbdt.grow_tree(dbins, dq, dexp, mapper, params)
    b = gbdt.grow_tree(dbins, dq, dexp, mapper, params, bag=None, features=None)
    _same_tree(a, {k: getattr(b, k) for k in TREE_INT + TREE_FLOAT}, 'none')
    # every row as a bag, every feature as a list: the same tree again
    every = gbdt.grow_tree(dbins, dq, dexp, mapper, params, bag=_t(np.arange(p['n'], dtype=np.int32), gpu_device), features=[0, 1, 2])
    _same_tree(every, {k: getattr(a, k) for k in TREE_INT + TREE_FLOAT}, 'every')
    assert every.hist_rows == a.hist_rows


# ---- trainings

def _train(name, dev, **kw):
    c = si.training(name)
    d = c['problem']
    mapper = _mapper(d['edge_list'])
    dX = _t(d['X'], dev)
    bins = gbdt.bin_matrix(dX, mapper)
    assert np.array_equal(bins.cpu().numpy(), d['bins'])
    valid = None
    if c['valid']:
        valid = (gbdt.bin_matrix(_t(d['Xv'], dev), mapper), _t(d['vlabel'], dev), _t(d['voff'], dev))
    sampling = gbdt.Sampling(bagging_seed=si.BAGGING_SEED, feature_fraction_seed=si.FEATURE_SEED, **c['sampling'])
    res = gbdt.train(bins, _t(d['label'], dev), _t(d['query_off'], dev), mapper, d['params'], valid=valid,
                     num_boost_round=c['rounds'], early_stopping_rounds=c['early_stopping_rounds'], keep_leaves=True,
                     sampling=sampling, **kw)
    return c, dX, res


@pytest.mark.parametrize('name', list(si.TRAIN_CASES))
def test_training_with_sampling_equals_the_restatement(gpu_device, name):
    c, dX, res = _train(name, gpu_device)
    want = c['want']
    assert res.best_iteration == want['best_iteration'] == len(res.trees) and res.history == want['history']
    for t, (got, w) in enumerate(zip(res.trees, want['trees'])):
        _same_tree(got, w, (name, t))
        assert got.hist_rows == w['hist_rows']
    wf = gr.to_forest(want['trees'], c['problem']['bins'].shape[0])
    for k in FOREST_ARRAYS:
        assert np.array_equal(getattr(res.forest, k), getattr(wf, k)), k
    assert np.array_equal(res.train_leaf.cpu().numpy(), want['train_leaf'])
    # over all rows, the out-of-bag ones included
    assert np.array_equal(_bits(res.train_score.cpu().numpy()), _bits(want['train_score']))
    assert np.array_equal(_bits(forest_predict(res.forest, dX).cpu().numpy()), _bits(res.train_score.cpu().numpy()))
    if c['early_stopping_rounds']:
        assert res.best_iteration < len(res.history)                # the cut happened


def test_sampling_with_both_fractions_one_changes_nothing(gpu_device):
    d = si.train_problem('random')
    mapper = _mapper(d['edge_list'])
    bins = gbdt.bin_matrix(_t(d['X'], gpu_device), mapper)
    valid = (gbdt.bin_matrix(_t(d['Xv'], gpu_device), mapper), _t(d['vlabel'], gpu_device), _t(d['voff'], gpu_device))
    label, off = _t(d['label'], gpu_device), _t(d['query_off'], gpu_device)
    plain = gbdt.train(bins, label, off, mapper, d['params'], valid=valid, num_boost_round=4, keep_leaves=True)
    for sampling in (gbdt.Sampling(), gbdt.Sampling(bagging_fraction=0.5, bagging_freq=0), gbdt.Sampling(bagging_freq=2, bagging_seed=9)):
        res = gbdt.train(bins, label, off, mapper, d['params'], valid=valid, num_boost_round=4, keep_leaves=True, sampling=sampling)
        for k in FOREST_ARRAYS:
            a, b = getattr(res.forest, k), getattr(plain.forest, k)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        assert res.history == plain.history and res.best_iteration == plain.best_iteration
        assert np.array_equal(res.train_leaf.cpu().numpy(), plain.train_leaf.cpu().numpy())
        assert np.array_equal(_bits(res.train_score.cpu().numpy()), _bits(plain.train_score.cpu().numpy()))
        assert [t.hist_rows for t in res.trees] == [t.hist_rows for t in plain.trees]
    with pytest.raises(ValueError, match='empty bag'):
        gbdt.train(bins, label, off, mapper, d['params'], num_boost_round=1, sampling=gbdt.Sampling(1e-5, 1))


# ---- the fold trainer

def test_cross_validate_with_sampling_equals_the_chain_written_out(gpu_device):
    import torch
    rng = np.random.default_rng(401)
    sizes = rng.integers(20, 41, 150)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, F = int(off[-1]), 6
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[rng.random((n, F)) < 0.02] = np.nan
    label = np.zeros(n, dtype=np.uint8)
    for q in range(150):
        a, b = off[q], off[q + 1]
        if rng.random() >= 0.15:
            label[a + int(np.argmax(X[a:b, 0] - 0.5 * np.nan_to_num(X[a:b, 1]) + 0.5 * rng.standard_normal(b - a)))] = 1
    config = {'num_leaves': 8, 'min_data_in_leaf': 20, 'learning_rate': 0.1, 'lambdarank_norm': False, 'bagging_fraction': 0.8,
              'bagging_freq': 2, 'feature_fraction': 0.5, 'feature_fraction_bynode': 1, 'bagging_seed': 42,
              'feature_fraction_seed': 42, 'seed': 42}
    params, sampling = gbdt.sampling_from_params(config)
    assert sampling == gbdt.Sampling(0.8, 2, 0.5, 42, 42)
    dX, doff = _t(X, gpu_device), _t(off, gpu_device)
    res = folds.cross_validate(dX, _t(label, gpu_device), doff, params, n_splits=3, negative_sampling_ratio=0.5, seed=42,
                               num_boost_round=6, early_stopping_rounds=3, sampling=sampling)
    fold_of_query, _ = fr.group_kfold(off, 3)
    assert np.array_equal(res.fold_of_query.cpu().numpy(), fold_of_query)
    label32 = _t(label.astype(np.int32), gpu_device)
    oof = np.zeros(n, dtype=np.float32)
    sampled = 0
    for fold in range(3):
        s = fr.fold_indices(label, off, fold_of_query, fold, 0.5, 42)
        t_idx, v_idx = _t(s['train_idx'], gpu_device).long(), _t(s['val_idx'], gpu_device).long()
        mapper = gbdt.fit_bins(X[s['train_idx']])
        bins = gbdt.bin_matrix(dX, mapper)
        t_bins, v_bins = bins[:, t_idx].contiguous(), bins[:, v_idx].contiguous()
        want = gbdt.train(t_bins, label32[t_idx], _t(s['train_query_off'], gpu_device), mapper, params,
                          valid=(v_bins, label32[v_idx], _t(s['val_query_off'], gpu_device)), num_boost_round=6,
                          early_stopping_rounds=3, sampling=sampling)
        # ... and that training is the restatement's, draws included
        edge_list = [mapper.feature_edges(f) for f in range(F)]
        restated = sr.train(t_bins.cpu().numpy(), label[s['train_idx']].astype(np.int32), s['train_query_off'], edge_list,
                            dict(num_leaves=8, min_data_in_leaf=20, learning_rate=0.1, lambdarank_norm=False),
                            valid=(v_bins.cpu().numpy(), label[s['val_idx']].astype(np.int32), s['val_query_off']),
                            num_boost_round=6, early_stopping_rounds=3, bagging_fraction=0.8, bagging_freq=2, feature_fraction=0.5,
                            bagging_seed=42, feature_fraction_seed=42)
        wf = gr.to_forest(restated['trees'], F)
        got = res.forests[fold]
        for name in FOREST_ARRAYS:
            a, b = getattr(got, name), getattr(want.forest, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (fold, name)
            assert np.array_equal(a, getattr(wf, name)), (fold, name)
        assert res.best_iterations[fold] == want.best_iteration == restated['best_iteration']
        assert res.histories[fold] == want.history == restated['history']
        m = int(0.8 * s['train_idx'].size)
        assert all(t.leaf_count.sum() == m for t in res.trees[fold])
        sampled += sum(set(t.split_feature.tolist()) <= set(f.tolist()) for t, f in zip(res.trees[fold], restated['features']))
        score = torch.zeros(v_idx.numel(), dtype=torch.float64, device=gpu_device)
        for tree in want.trees:
            gbdt.add_tree(v_bins, tree, score)
        oof[s['val_idx']] = score.to(torch.float32).cpu().numpy()
    assert sampled == sum(len(t) for t in res.trees)
    assert np.array_equal(res.oof_prediction.cpu().numpy().view(np.uint32), oof.view(np.uint32))
