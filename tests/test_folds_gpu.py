"""SPEC-FOLDS on the device against the NumPy restatement (tests/folds_restatement.py) and scikit-learn's recorded
assignments: the fold walk, the index sets of a fold, the bin gather and the fold trainer. Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import folds_restatement as fr
from otto_amd import _lib
from otto_amd.ranker import evaluate, folds, gbdt
from otto_amd.ranker.forest import session_topk

pytestmark = pytest.mark.gpu

SEEDS = (0, 42, 2 ** 64 - 1)
INDEX_ARRAYS = ('train_idx', 'train_query_off', 'train_query', 'val_idx', 'val_query_off', 'val_query')


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)                    # a copy: a one-element reversed view keeps its negative stride


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'folds_golden.npz')) as z:
        return {k: z[k] for k in z.files}


# ---- fold assignment

def _size_patterns(rng, Q, golden):
    yield 'equal', np.full(Q, 7)
    if f'distinct_{Q}_sizes' in golden:
        yield 'distinct', golden[f'distinct_{Q}_sizes']
    yield 'small', rng.integers(1, 5, Q)
    big = rng.integers(1, 60, Q)
    big[rng.choice(Q, min(Q, 3), replace=False)] = gbdt.MAX_QUERY
    yield 'big', big
    zero = rng.integers(0, 4, Q)
    zero[rng.choice(Q, max(Q // 4, 1), replace=False)] = 0
    yield 'zero', zero


@pytest.mark.parametrize('n_splits', [2, 5, 16])
def test_group_kfold_equals_restatement_and_scikit_learn(gpu_device, golden, n_splits):
    rng = np.random.default_rng(n_splits)
    distinct_seen = 0
    for Q in (n_splits, n_splits + 1, 63, 64, 65, 257, 4097):
        for name, sizes in _size_patterns(rng, Q, golden):
            off = _off(sizes)
            got, rows = folds.group_kfold(_t(off, gpu_device), n_splits, n=int(off[-1]))
            want, want_rows = fr.group_kfold(off, n_splits)
            assert got.cpu().numpy().dtype == want.dtype and np.array_equal(got.cpu().numpy(), want), (name, Q)
            assert np.array_equal(rows.cpu().numpy(), want_rows), (name, Q)
            if name == 'distinct':
                assert np.array_equal(got.cpu().numpy(), golden[f'distinct_{Q}_k{n_splits}']), Q
                distinct_seen += 1
    assert distinct_seen >= 5


def test_group_kfold_without_a_row_count_and_with_timing(gpu_device):
    off = _off(np.arange(300) % 9)
    timing = {}
    got, rows = folds.group_kfold(_t(off, gpu_device), 5, timing=timing)
    want, want_rows = fr.group_kfold(off, 5)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(rows.cpu().numpy(), want_rows)
    assert timing['walk_ms'] > 0.0


@pytest.mark.parametrize('kind', ['too_long', 'descending', 'negative', 'past_n'])
def test_group_kfold_refuses_bad_offsets_and_writes_nothing(gpu_device, kind):
    import torch
    sizes = np.full(70, 3)
    if kind == 'too_long':
        sizes[40] = gbdt.MAX_QUERY + 1
    off = _off(sizes)
    n = int(off[-1])
    if kind == 'descending':
        off[41] = off[40] - 1
    elif kind == 'negative':
        off[0] = -1
    elif kind == 'past_n':
        n -= 1
    d_off = _t(off, gpu_device)
    with pytest.raises(_lib.OttoError, match='query_off'):
        folds.group_kfold(d_off, 5, n=n)
    lib = _lib.lib()
    fold = torch.full((70,), -7, dtype=torch.int32, device=gpu_device)
    rows = torch.full((5,), -7, dtype=torch.int64, device=gpu_device)
    work = torch.empty(lib.otto_folds_kfold_workspace(70), dtype=torch.uint8, device=gpu_device)
    rc = lib.otto_folds_group_kfold(C.c_void_p(d_off.data_ptr()), 70, n, 5, C.c_void_p(fold.data_ptr()), C.c_void_p(rows.data_ptr()),
                                    None, C.c_void_p(work.data_ptr()), work.numel(),
                                    C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream))
    assert rc == -22
    assert (fold == -7).all().item() and (rows == -7).all().item()


def test_group_kfold_argument_checks(gpu_device):
    off = _t(_off([1, 2, 3]), gpu_device)
    with pytest.raises(ValueError):
        folds.group_kfold(off, 5)                                   # Q < n_splits
    for k in (1, 17):
        with pytest.raises(ValueError):
            folds.group_kfold(off, k)
    with pytest.raises(ValueError):
        folds.group_kfold(off.to(dtype=off.dtype).int(), 2)
    with pytest.raises(_lib.OttoError):
        folds.group_kfold(off.cpu(), 2)


# ---- index sets

def _index_case(rng, n, label_dtype, eligible_share=None):
    """Queries of mixed sizes (zero-row ones among them) over n rows, labels with queries of every composition."""
    sizes = []
    left = n
    top = 12 if n <= 300 else 90
    while left:
        c = int(rng.integers(0, top + 1)) if rng.random() < 0.95 else gbdt.MAX_QUERY
        c = min(c, left)
        sizes.append(c)
        left -= c
    sizes += [0, 0]
    rng.shuffle(sizes)
    off = _off(sizes)
    Q = len(sizes)
    label = np.zeros(n, dtype=np.int64)
    for q in range(Q):
        a, b = off[q], off[q + 1]
        u = rng.random()
        if eligible_share is not None:                              # nearly every query has a positive, most rows are negatives
            label[a:b] = rng.random(b - a) < 0.1
            if b > a:
                label[a] = 1
        elif u < 0.2:
            pass                                                    # no positive: dropped whole
        elif u < 0.35:
            label[a:b] = 1 + (rng.random(b - a) < 0.3)              # all positives, some with label 2
        elif u < 0.5 and b - a >= 2:
            label[a:b] = 1
            label[a + int(rng.integers(0, b - a))] = 0              # a single negative
        else:
            label[a:b] = (rng.random(b - a) < 0.3) * rng.integers(1, 3, b - a)
    fold = rng.integers(0, 5, Q).astype(np.int32)
    fold[np.asarray(sizes) == 0] = 0                                # fold 0 validates the zero-row queries
    return label.astype(label_dtype), off, fold


def _compare(gpu_device, label, off, fold_of_query, fold, ratio, seed):
    d = [_t(label, gpu_device), _t(off, gpu_device), _t(fold_of_query, gpu_device)]
    got = folds.fold_indices(*d, fold, ratio, seed)
    want = fr.fold_indices(label, off, fold_of_query, fold, ratio, seed)
    tag = (label.size, fold, ratio, seed)
    for name in INDEX_ARRAYS:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), (name, tag)
    assert got.n_eligible == want['n_eligible'] and got.n_kept == want['n_kept'] == fr.sample_size(ratio, want['n_eligible']), tag
    t_idx, v_idx = got.train_idx.cpu().numpy(), got.val_idx.cpu().numpy()
    kept_negatives = int(np.count_nonzero(label[t_idx] == 0))
    assert kept_negatives == got.n_kept, tag                        # exactly m
    assert np.intersect1d(t_idx, v_idx).size == 0 and (np.diff(t_idx) > 0).all(), tag
    again = folds.fold_indices(*d, fold, ratio, seed)
    for name in INDEX_ARRAYS:
        assert np.array_equal(getattr(again, name).cpu().numpy(), getattr(got, name).cpu().numpy()), (name, tag)
    return got


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257])
def test_fold_indices_small_shapes(gpu_device, n):
    rng = np.random.default_rng(n)
    for label_dtype in (np.uint8, np.int32):
        label, off, fold = _index_case(rng, n, label_dtype)
        for ratio in (0.0, 0.3, 0.5, 1.0):
            for seed in SEEDS:
                _compare(gpu_device, label, off, fold, 0, ratio, seed)
        _compare(gpu_device, label, off, fold, 3, 0.3, 42)
        _compare(gpu_device, label, off, fold, 7, 0.3, 42)          # a fold nobody is in: no validation row


def test_fold_indices_65537_rows(gpu_device):
    rng = np.random.default_rng(65537)
    label, off, fold = _index_case(rng, 65537, np.uint8)
    for seed in SEEDS:
        _compare(gpu_device, label, off, fold, 0, 0.3, seed)
    _compare(gpu_device, label.astype(np.int32), off, fold, 2, 0.5, 42)


def test_fold_indices_crowded_select(gpu_device):
    n = (1 << 18) + 3
    rng = np.random.default_rng(18)
    label, off, fold = _index_case(rng, n, np.uint8, eligible_share=0.7)
    got = _compare(gpu_device, label, off, fold, 0, 0.3, 42)
    assert 0.6 * n < got.n_eligible < 0.8 * n


@pytest.mark.parametrize('ratio', [0.0, 0.3, 0.5, 1.0])
def test_fold_indices_tiny_eligible_counts(gpu_device, ratio):
    # N = 0 (no eligible negative at all), 1 (0.5 x 1 -> 0: the only negative is dropped) and 3 (0.5 x 3 -> 2)
    for negatives in (0, 1, 3):
        label = np.array([1] + [0] * negatives + [1, 2] + [0, 0, 0] + [0, 1], dtype=np.int32)
        off = _off([1 + negatives, 2, 3, 0, 2])
        fold = np.array([0, 0, 0, 1, 1], dtype=np.int32)            # fold 1: a zero-row query and a real one
        for seed in SEEDS:
            got = _compare(gpu_device, label, off, fold, 1, ratio, seed)
            assert got.n_eligible == negatives
            assert got.n_kept == {0: 0, 1: round(ratio * 1), 3: round(ratio * 3)}[negatives]
            assert got.val_query.cpu().numpy().tolist() == [4]
    assert round(0.5 * 1) == 0 and round(0.5 * 3) == 2


def test_fold_indices_refusals(gpu_device):
    label, off, fold = np.zeros(10, dtype=np.int32), _off([5, 5]), np.array([0, 1], dtype=np.int32)
    d = lambda *a: [_t(x, gpu_device) for x in a]
    bad = off.copy()
    bad[1] = 11
    with pytest.raises(_lib.OttoError, match='query_off'):
        folds.fold_indices(*d(label, bad, fold), 0, 0.3)
    neg = label.copy()
    neg[7] = -1
    with pytest.raises(_lib.OttoError, match='label'):
        folds.fold_indices(*d(neg, off, fold), 0, 0.3)
    for ratio in (-0.1, 1.5):
        with pytest.raises(ValueError):
            folds.fold_indices(*d(label, off, fold), 0, ratio)
    with pytest.raises(ValueError):
        folds.fold_indices(*d(label, off, fold[:1]), 0, 0.3)
    with pytest.raises(ValueError):
        folds.fold_indices(*d(label.astype(np.int64), off, fold), 0, 0.3)


# ---- gather

@pytest.mark.parametrize('F', [1, 3, 54])
def test_gather_bins(gpu_device, F):
    n = 4099
    rng = np.random.default_rng(F)
    bins = rng.integers(0, 256, (F, n)).astype(np.uint8)
    d_bins = _t(bins, gpu_device)
    for m in (0, 1, 3, 4, 5, 63, 64, 65, 1027):
        asc = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
        rep = rng.integers(0, 7, m).astype(np.int32) * 683
        for idx in (asc, asc[::-1], rep):
            got = folds.gather_bins(d_bins, _t(idx, gpu_device)).cpu().numpy()
            assert got.shape == (F, m) and got.dtype == np.uint8 and np.array_equal(got, bins[:, idx]), (F, m)
    ends = np.array([0, n - 1, n - 1, 0, 5], dtype=np.int32)
    assert np.array_equal(folds.gather_bins(d_bins, _t(ends, gpu_device)).cpu().numpy(), bins[:, ends])
    for bad in (-1, n):
        idx = np.arange(9, dtype=np.int32)
        idx[6] = bad
        with pytest.raises(_lib.OttoError, match='index'):
            folds.gather_bins(d_bins, _t(idx, gpu_device))


# ---- the fold trainer

PARAMS = {'num_leaves': 8, 'min_data_in_leaf': 20, 'learning_rate': 0.1}
CV = dict(n_splits=5, negative_sampling_ratio=0.3, seed=42, num_boost_round=10, early_stopping_rounds=3)


@pytest.fixture(scope='module')
def driver(gpu_device):
    rng = np.random.default_rng(400)
    sizes = rng.integers(20, 41, 400)
    off = _off(sizes)
    n, F = int(off[-1]), 6
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[rng.random((n, F)) < 0.02] = np.nan
    label = np.zeros(n, dtype=np.uint8)
    aid = np.zeros(n, dtype=np.int32)
    t_off, t_aid = [0], []
    for q in range(400):
        a, b = off[q], off[q + 1]
        aid[a:b] = rng.choice(5000, b - a, replace=False)
        if rng.random() >= 0.15:                                    # 15 % of the queries have no positive
            pos = a + int(np.argmax(X[a:b, 0] + 0.5 * rng.standard_normal(b - a)))
            label[pos] = 1
            t_aid.append(aid[pos])
        if rng.random() < 0.3:
            t_aid.append(5000 + q)                                  # a label no candidate row carries
        t_off.append(len(t_aid))
    truth = (_t(np.array(t_off, dtype=np.int64), gpu_device), _t(np.array(t_aid, dtype=np.int32), gpu_device))
    dX, dlabel, doff, daid = _t(X, gpu_device), _t(label, gpu_device), _t(off, gpu_device), _t(aid, gpu_device)
    res = folds.cross_validate(dX, dlabel, doff, PARAMS, aid=daid, truth=truth, **CV)
    return dict(X=X, label=label, off=off, dX=dX, doff=doff, daid=daid, truth=truth, res=res, n=n, F=F)


def test_cross_validate_equals_the_chain_written_out(gpu_device, driver):
    import torch
    d, res = driver, driver['res']
    fold_of_query, fold_rows = fr.group_kfold(d['off'], 5)
    assert np.array_equal(res.fold_of_query.cpu().numpy(), fold_of_query) and np.array_equal(res.fold_rows.cpu().numpy(), fold_rows)
    label32 = _t(d['label'].astype(np.int32), gpu_device)
    oof = np.zeros(d['n'], dtype=np.float32)
    written = np.zeros(d['n'], dtype=np.int64)
    for fold in range(5):
        s = fr.fold_indices(d['label'], d['off'], fold_of_query, fold, 0.3, 42)
        t_idx, v_idx = _t(s['train_idx'], gpu_device).long(), _t(s['val_idx'], gpu_device).long()
        mapper = gbdt.fit_bins(d['X'][s['train_idx']])              # fewer than 200,000 rows: stride 1
        bins = gbdt.bin_matrix(d['dX'], mapper)
        t_bins, v_bins = bins[:, t_idx].contiguous(), bins[:, v_idx].contiguous()
        want = gbdt.train(t_bins, label32[t_idx], _t(s['train_query_off'], gpu_device), mapper, PARAMS,
                          valid=(v_bins, label32[v_idx], _t(s['val_query_off'], gpu_device)), num_boost_round=10,
                          early_stopping_rounds=3)
        got = res.forests[fold]
        for name in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value'):
            a, b = getattr(got, name), getattr(want.forest, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (fold, name)
        assert res.best_iterations[fold] == want.best_iteration and res.histories[fold] == want.history
        score = torch.zeros(v_idx.numel(), dtype=torch.float64, device=gpu_device)
        for tree in want.trees:
            gbdt.add_tree(v_bins, tree, score)
        oof[s['val_idx']] = score.to(torch.float32).cpu().numpy()
        written[s['val_idx']] += 1
        gain, split = np.zeros(d['F']), np.zeros(d['F'], dtype=np.int64)
        for tree in res.trees[fold]:
            for f, g in zip(tree.split_feature, tree.split_gain):
                gain[f] += g
                split[f] += 1
        assert np.array_equal(res.importance_split[:, fold], split)
        assert np.array_equal(res.importance_gain[:, fold].view(np.uint64), gain.view(np.uint64))
        assert split.sum() > 0
    assert (written == 1).all()                                     # every row is written by exactly one fold
    got_oof = res.oof_prediction.cpu().numpy()
    assert got_oof.dtype == np.float32 and np.array_equal(got_oof.view(np.uint32), oof.view(np.uint32))
    assert res.importance_gain.shape == (d['F'], 5) and res.importance_split.shape == (d['F'], 5)


def test_cross_validate_recall_equals_hits_by_hand(gpu_device, driver):
    import torch
    d, res = driver, driver['res']
    top_aid, _, top_n = session_topk(res.oof_prediction.to(torch.float64), d['daid'], d['doff'], k=20)
    assert torch.equal(top_aid, res.top_aid) and torch.equal(top_n, res.top_n)
    h, den, tot = evaluate.hits(d['truth'], (top_aid, top_n), cap=20)
    h, den, fold = h.cpu().numpy(), den.cpu().numpy(), res.fold_of_query.cpu().numpy()
    assert res.hits == tot['hits'] == int(h.sum()) and res.denom == tot['denom'] == int(den.sum())
    assert res.hits > 0 and res.recall == res.hits / res.denom
    for f in range(5):
        assert res.fold_hits[f] == int(h[fold == f].sum()) and res.fold_denom[f] == int(den[fold == f].sum()), f
        assert res.fold_recall[f] == res.fold_hits[f] / res.fold_denom[f]
    assert sum(res.fold_hits) == res.hits and sum(res.fold_denom) == res.denom


def test_cross_validate_without_truth_returns_no_recall(gpu_device, driver):
    d = driver
    res = folds.cross_validate(d['dX'], _t(d['label'], gpu_device), d['doff'], PARAMS, n_splits=2, num_boost_round=2)
    assert res.recall is None and res.fold_hits is None and len(res.forests) == 2
    assert all(f.n_trees == 2 for f in res.forests)
