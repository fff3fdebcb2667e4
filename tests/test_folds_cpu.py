"""SPEC-FOLDS without a GPU: the NumPy restatement (tests/folds_restatement.py) against scikit-learn's recorded GroupKFold
assignments (tests/golden/folds_golden.npz), the sample size against pandas, the keys, and the importances."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import folds_restatement as fr

SPLITS = (2, 5, 16)


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'folds_golden.npz')) as z:
        return {k: z[k] for k in z.files}


def _cases(golden):
    for key in golden:
        if key.endswith('_sizes'):
            name = key[:-len('_sizes')]
            for k in SPLITS:
                if f'{name}_k{k}' in golden:
                    yield name, golden[key].astype(np.int64), k, golden[f'{name}_k{k}']


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_fold_rows_and_size_multisets_equal_scikit_learn(golden):
    seen = 0
    for name, sizes, k, want in _cases(golden):
        got, rows = fr.group_kfold(_off(sizes), k)
        for f in range(k):
            assert rows[f] == sizes[want == f].sum(), (name, k, f)
            mine, theirs = np.sort(sizes[got == f]), np.sort(sizes[want == f])
            assert np.array_equal(mine[mine > 0], theirs), (name, k, f)        # scikit-learn never sees a zero-row group
        assert rows.sum() == sizes.sum() and np.array_equal(rows, np.bincount(got, weights=sizes, minlength=k).astype(np.int64))
        seen += 1
    assert seen >= 30


def test_assignment_equals_scikit_learn_for_distinct_sizes(golden):
    seen = 0
    for name, sizes, k, want in _cases(golden):
        if name.startswith('distinct_'):
            got, _ = fr.group_kfold(_off(sizes), k)
            assert np.array_equal(got, want), (name, k)
            seen += 1
    assert seen >= 20


def test_tie_order_is_size_descending_then_index_descending():
    # four equal queries, two folds: positions 3, 2, 1, 0 -> folds 0, 1, 0, 1
    got, rows = fr.group_kfold(_off([5, 5, 5, 5]), 2)
    assert got.tolist() == [1, 0, 1, 0] and rows.tolist() == [10, 10]
    got, rows = fr.group_kfold(_off([1, 3, 3, 0, 2]), 3)
    assert got.tolist() == [2, 1, 0, 0, 2] and rows.tolist() == [3, 3, 3]


@pytest.mark.parametrize('ratio', [0.0, 0.3, 0.5, 0.7, 1.0])
def test_sample_size_is_the_count_pandas_returns(ratio):
    pd = pytest.importorskip('pandas')
    for N in (0, 1, 3, 5, 7, 15, 25, 35, 45):
        assert fr.sample_size(ratio, N) == len(pd.Series(range(N)).sample(frac=ratio, random_state=42)), (ratio, N)
    assert fr.sample_size(0.5, 1) == 0 and fr.sample_size(0.5, 3) == 2


@pytest.mark.parametrize('seed', [0, 42, 2 ** 64 - 1])
def test_keys_of_consecutive_rows_are_distinct(seed):
    k = fr.keys(seed, np.arange(1 << 20))
    assert k.dtype == np.uint64 and np.unique(k).size == 1 << 20
    for r in (0, 1, 63, (1 << 20) - 1):
        assert int(k[r]) == fr.key_int(seed, r)
    assert int(fr.keys(seed, np.array([2 ** 31 - 2]))[0]) == fr.key_int(seed, 2 ** 31 - 2)


def test_restated_index_sets_on_a_hand_case():
    # queries: 0 = rows 0-2 (fold 0), 1 = rows 3-5 (one positive), 2 = rows 6-7 (no positive), 3 = no row, 4 = row 8 (positive)
    off = [0, 3, 6, 8, 8, 9]
    label = np.array([0, 1, 0, 0, 2, 0, 0, 0, 1], dtype=np.int32)
    fold = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    s = fr.fold_indices(label, off, fold, 0, 1.0, 42)
    assert s['val_idx'].tolist() == [0, 1, 2] and s['val_query'].tolist() == [0] and s['val_query_off'].tolist() == [0, 3]
    assert s['train_idx'].tolist() == [3, 4, 5, 8] and s['train_query'].tolist() == [1, 4]
    assert s['train_query_off'].tolist() == [0, 3, 4] and s['n_eligible'] == 2 and s['n_kept'] == 2
    s = fr.fold_indices(label, off, fold, 0, 0.5, 42)
    smaller = 3 if fr.key_int(42, 3) < fr.key_int(42, 5) else 5
    assert s['train_idx'].tolist() == sorted([4, 8, smaller]) and s['n_kept'] == 1
    s = fr.fold_indices(label, off, fold, 0, 0.0, 42)
    assert s['train_idx'].tolist() == [4, 8] and s['train_query_off'].tolist() == [0, 1, 2]


def test_feature_importance_of_two_hand_written_trees():
    from otto_amd.ranker.folds import feature_importance
    from otto_amd.ranker.gbdt import BinTree
    a = BinTree(split_feature=np.array([2, 0, 2], dtype=np.int32), split_gain=np.array([1.5, 0.25, 4.0]))
    b = BinTree(split_feature=np.array([1], dtype=np.int32), split_gain=np.array([0.125]))
    gain, split = feature_importance([a, b], 4)
    assert gain.dtype == np.float64 and split.dtype == np.int64
    assert gain.tolist() == [0.25, 0.125, 5.5, 0.0] and split.tolist() == [1, 1, 2, 0]
    gain, split = feature_importance([], 2)
    assert gain.tolist() == [0.0, 0.0] and split.tolist() == [0, 0]
