"""SPEC-FOLDS (include/otto_folds.h) restated in NumPy, one query at a time: the fold walk as the header writes it, the
keys with np.uint64 wrap-around (and once more with Python integers), the index sets by a loop over the queries."""
import numpy as np

MAX_QUERY = 1024
M64 = (1 << 64) - 1


def invalid_queries(off, n):
    off = np.asarray(off, dtype=np.int64)
    a, b = off[:-1], off[1:]
    return int(np.count_nonzero(~((a >= 0) & (a <= b) & (b <= n) & (b - a <= MAX_QUERY))))


def group_kfold(off, n_splits):
    """(fold_of_query int32 [Q], fold_rows int64 [n_splits])."""
    off = np.asarray(off, dtype=np.int64)
    c = off[1:] - off[:-1]
    order = np.argsort(c, kind='stable')[::-1]            # size descending, index descending among equals
    fold_rows = np.zeros(n_splits, dtype=np.int64)
    fold_of_query = np.zeros(c.size, dtype=np.int32)
    for q in order:
        f = int(np.argmin(fold_rows))                     # the first minimum: the lowest fold index
        fold_of_query[q] = f
        fold_rows[f] += c[q]
    return fold_of_query, fold_rows


def key_int(seed, r):
    """splitmix64 of the global row index with Python integers."""
    z = (seed + (r + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keys(seed, rows):
    """The same over an array of row indices, np.uint64 with wrap-around."""
    with np.errstate(over='ignore'):
        r = np.asarray(rows).astype(np.uint64)
        z = np.uint64(seed) + (r + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_size(ratio, n_eligible):
    return int(round(float(ratio) * int(n_eligible)))


def fold_indices(label, off, fold_of_query, fold, ratio, seed):
    """dict(train_idx, train_query_off, train_query, val_idx, val_query_off, val_query, n_eligible, n_kept)."""
    label = np.asarray(label)
    off = np.asarray(off, dtype=np.int64)
    if (label.astype(np.int64) < 0).any():
        raise ValueError('a label below 0')
    Q = off.size - 1
    eligible = []
    for q in range(Q):
        rows = np.arange(off[q], off[q + 1])
        if fold_of_query[q] != fold and (label[rows] > 0).any():
            eligible.append(rows[label[rows] == 0])
    eligible = np.concatenate(eligible) if eligible else np.zeros(0, dtype=np.int64)
    N = eligible.size
    m = sample_size(ratio, N)
    kept = set(eligible[np.argsort(keys(seed, eligible), kind='stable')[:m]].tolist())
    t_idx, t_off, t_q, v_idx, v_off, v_q = [], [0], [], [], [0], []
    for q in range(Q):
        rows = np.arange(off[q], off[q + 1])
        if fold_of_query[q] == fold:
            if rows.size:
                v_idx += rows.tolist()
                v_off.append(len(v_idx))
                v_q.append(q)
        elif (label[rows] > 0).any():
            keep = [int(r) for r in rows if label[r] > 0 or int(r) in kept]
            t_idx += keep
            t_off.append(len(t_idx))
            t_q.append(q)
    return dict(train_idx=np.array(t_idx, dtype=np.int32), train_query_off=np.array(t_off, dtype=np.int64),
                train_query=np.array(t_q, dtype=np.int32), val_idx=np.array(v_idx, dtype=np.int32),
                val_query_off=np.array(v_off, dtype=np.int64), val_query=np.array(v_q, dtype=np.int32), n_eligible=N, n_kept=m)
