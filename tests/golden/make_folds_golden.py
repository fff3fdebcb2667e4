"""Writes tests/golden/folds_golden.npz: scikit-learn's own GroupKFold assignments for the inputs of the fold tests.

Per case `name`: `<name>_sizes` int32 [Q] (the rows of every query) and, per n_splits k, `<name>_k<k>` int32 [Q]: the
fold scikit-learn puts the query in (-1 for a zero-row query, which scikit-learn never sees as a group). The `distinct_*`
cases hold the sizes 1..Q in a fixed shuffled order: there scikit-learn's assignment is defined without a tie order.

    python tests/golden/make_folds_golden.py        (needs scikit-learn; recorded with 1.7.2)
"""
import os

import numpy as np

SPLITS = (2, 5, 16)
DISTINCT_Q = (2, 3, 5, 6, 16, 17, 63, 64, 65, 257)
PATTERN_Q = (65, 1500)


def cases():
    rng = np.random.default_rng(20260101)
    out = {}
    for Q in DISTINCT_Q:
        out[f'distinct_{Q}'] = rng.permutation(np.arange(1, Q + 1)).astype(np.int32)
    for Q in PATTERN_Q:
        out[f'equal_{Q}'] = np.full(Q, 7, dtype=np.int32)
        out[f'small_{Q}'] = rng.integers(1, 5, Q).astype(np.int32)
        big = rng.integers(1, 60, Q).astype(np.int32)
        big[rng.choice(Q, 5, replace=False)] = 1024
        out[f'big_{Q}'] = big
        zero = rng.integers(0, 4, Q).astype(np.int32)
        zero[:3] = 0
        out[f'zero_{Q}'] = zero
    return out


def sklearn_folds(sizes, k):
    from sklearn.model_selection import GroupKFold
    groups = np.repeat(np.arange(sizes.size), sizes)
    fold = np.full(sizes.size, -1, dtype=np.int32)
    for f, (_, test) in enumerate(GroupKFold(n_splits=k).split(np.zeros(groups.size), groups=groups)):
        fold[np.unique(groups[test])] = f
    return fold


def main():
    out = {}
    for name, sizes in cases().items():
        out[f'{name}_sizes'] = sizes
        for k in SPLITS:
            if np.count_nonzero(sizes) >= k:
                out[f'{name}_k{k}'] = sklearn_folds(sizes, k)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'folds_golden.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {len(out)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
