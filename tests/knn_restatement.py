"""Float64 NumPy restatement of SPEC-KNN and the derived error band the GPU tests compare with.

Per query aid a: every valid b != a (self excluded by id), ordered by (key asc, b asc), the first k.
    euclidean  key = sum_i (a_i - b_i)^2               value = sqrt(max(key, 0))
    angular    key = 2 - 2 cos(a, b), 2 if a norm is 0   value = sqrt(max(key, 0))
    dot        key = -<a, b>                            value = <a, b>

The band ``tau`` (not tuned; u = 2^-24): an fp32 dot product of length d is off by at most d u |a| |b|. The euclidean
key is three such products, |err(D2)| <= 2 d u (|a|^2 + |b|^2); twice that for the remaining roundings (the row scale,
the subtraction, sqrt and squaring back) gives tau = 4 d u (|a|^2 + |b|^2). Likewise 8 d u on the angular key and
2 d u |a| |b| on the dot key. The returned distance is compared THROUGH ITS SQUARE against the float64 key: near
neighbours lose digits to cancellation in |a|^2 + |b|^2 - 2<a,b>, so a relative bound on the distance itself would not
hold and is not what the kernel promises.
"""
import numpy as np

U32 = 2.0 ** -24


def keys_matrix(E, metric, valid=None, rows=None):
    """float64 keys [R, N]; +inf at self (by id) and at invalid columns."""
    E = np.asarray(E, dtype=np.float64)
    N = E.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    A = E[rows]
    ab = A @ E.T
    if metric == 'euclidean':
        if E.shape[1] <= 4:      # the hand-computed fixtures: literal differences
            key = ((A[:, None, :] - E[None, :, :]) ** 2).sum(-1)
        else:                    # float64 expansion: its own error (~1e-13 here) is far inside every band used
            key = np.maximum((A * A).sum(1)[:, None] + (E * E).sum(1)[None, :] - 2.0 * ab, 0.0)
    elif metric == 'angular':
        na, nb = np.sqrt((A * A).sum(1)), np.sqrt((E * E).sum(1))
        den = na[:, None] * nb[None, :]
        cos = np.divide(ab, den, out=np.zeros_like(ab), where=den > 0)
        key = np.where(den > 0, 2.0 - 2.0 * cos, 2.0)
    elif metric == 'dot':
        key = -ab
    else:
        raise ValueError(metric)
    key = key.copy()
    key[np.arange(len(rows)), rows] = np.inf
    if valid is not None:
        key[:, np.asarray(valid) == 0] = np.inf
    return key


def knn(E, k, metric='euclidean', valid=None, rows=None, extra=0):
    """(ids int32 [R, k] (-1 padded), value float64 [R, k] (+inf padded), n int32 [R], keys float64 [R, k + extra]
    (+inf padded) and ids_x int32 [R, k + extra]: the sorted keys / ids of the first k + extra neighbours, for the
    tie-band checks)."""
    E = np.asarray(E)
    N = E.shape[0]
    q = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    key = keys_matrix(E, metric, valid, rows)
    order = np.argsort(key, axis=1, kind='stable')      # stable: equal keys keep ascending ids
    kk = k + extra
    R = len(q)
    ids = np.full((R, kk), -1, dtype=np.int64)
    keys = np.full((R, kk), np.inf)
    w = min(kk, N)
    ids[:, :w] = order[:, :w]
    keys[:, :w] = np.take_along_axis(key, order[:, :w], axis=1)
    if valid is not None:
        dead = np.asarray(valid)[q] == 0
        keys[dead] = np.inf
    ids[~np.isfinite(keys)] = -1
    n = np.minimum(np.isfinite(keys).sum(1), k).astype(np.int32)
    kz = keys[:, :k]
    if metric == 'dot':
        value = np.where(np.isfinite(kz), -kz, np.inf)
    else:
        value = np.sqrt(np.maximum(kz, 0.0))
    return ids[:, :k].astype(np.int32), value, n, keys, ids.astype(np.int32)


def tau(E, metric, row_ids, col_ids):
    """The band on the KEY for the pairs (row aid, column aid), broadcast; columns < 0 (padding) give 0."""
    E = np.asarray(E, dtype=np.float64)
    d = E.shape[1]
    n2 = (E * E).sum(1)
    c = np.maximum(col_ids, 0)
    if metric == 'euclidean':
        t = 4.0 * d * U32 * (n2[row_ids] + n2[c])
    elif metric == 'angular':
        t = np.broadcast_to(8.0 * d * U32, np.broadcast(row_ids, c).shape).copy()
    else:
        t = 2.0 * d * U32 * np.sqrt(n2[row_ids] * n2[c])
    return np.where(col_ids >= 0, t, 0.0)


def value_to_key(value, metric):
    """The key a returned value stands for, in float64 (euclidean / angular: the square; dot: the negation)."""
    v = np.asarray(value, dtype=np.float64)
    return -v if metric == 'dot' else v * v


def close_positions(E, metric, q, ids_x, keys_x, k):
    """bool [R, k]: positions whose key lies closer than tau to the key before or after it in the restatement's own
    order over its first k + 1 neighbours (``ids_x`` / ``keys_x`` from ``knn(.., extra=1)``, at least k + 1 wide). Only
    at such positions may an fp32 kernel order two candidates the other way round; a swap moves both of them, hence both
    neighbours are looked at."""
    ids1, keys1 = ids_x[:, :k + 1], keys_x[:, :k + 1]
    t = tau(E, metric, np.asarray(q)[:, None], ids1)
    with np.errstate(invalid='ignore'):
        gap = keys1[:, 1:] - keys1[:, :-1]                         # gap[j] between positions j and j + 1
    band = np.maximum(t[:, 1:], t[:, :-1])
    near = np.isfinite(keys1[:, 1:]) & np.isfinite(keys1[:, :-1]) & (gap < band)
    out = near.copy()                                               # position j close to j + 1
    out[:, 1:] |= near[:, :-1]                                      # position j close to j - 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of the GPU parity tests: standard-normal rows, fixed seeds. N and k per d were chosen by the CPU check
# ``test_restatement_near_tie_share_of_the_gpu_inputs`` (the restatement's own share of positions whose neighbouring
# float64 keys lie inside tau must stay under 1 %, else the parity test could hide behind its band). The band grows like
# d * |a|^2 ~ d^2 while the key gaps of standard-normal rows grow like sqrt(d), so that share rises steeply with d and
# k and hardly falls with N: at d = 64 the wide lists fit only a small table, and at d = 128 no N in 131 .. 5003 keeps
# k >= 20 under 1 % (1.6 % .. 6 % measured), so d = 128 is compared at k in {1, 4, 8}; its 64-wide lists are covered by
# the exact-tie and determinism tests, which need no band.
# ---------------------------------------------------------------------------------------------------------------------
PARITY_SHAPES = (
    # d, N, ks
    (8, 3001, (1, 20, 45, 50, 64)),
    (32, 3001, (1, 20, 45, 50, 64)),
    (64, 3001, (1, 20)),
    (64, 89, (45, 50, 64)),         # N <= 1024: one item range, no splits
    (128, 3001, (1, 4, 8)),
)
PARITY_MODES = ('all', 'valid', 'rows', 'valid+rows')
FEW_ROWS_SHAPE = (32, 20011, (45,))     # 50 query rows against 20,011 items: 20 item-range splits and the merge
METRIC_NAMES = ('euclidean', 'angular', 'dot')
MAX_NEAR_TIE_SHARE = 0.01


def parity_case(d, N, mode):
    """(E float32 [N, d], valid uint8 [N] or None, rows int32 [R] or None) of one parity input."""
    E = np.random.default_rng(1000 + d).standard_normal((N, d)).astype(np.float32)
    valid = rows = None
    if 'valid' in mode:
        valid = (np.random.default_rng(77).random(N) > 0.2).astype(np.uint8)
    if 'rows' in mode:
        rows = np.random.default_rng(78).choice(N, size=N // 3, replace=False).astype(np.int32)
    if mode == 'few':
        rows = np.random.default_rng(79).choice(N, size=50, replace=False).astype(np.int32)
    return E, valid, rows


def parity_cases():
    for d, N, ks in PARITY_SHAPES:
        for mode in PARITY_MODES:
            yield d, N, ks, mode
    yield FEW_ROWS_SHAPE + ('few',)


def pair_keys(E, metric, row_ids, col_ids):
    """float64 keys of the pairs (row_ids[r], col_ids[r, j]) computed literally; +inf where col_ids < 0."""
    E = np.asarray(E, dtype=np.float64)
    A = E[np.asarray(row_ids, dtype=np.int64)][:, None, :]
    B = E[np.maximum(col_ids, 0)]
    if metric == 'euclidean':
        key = ((A - B) ** 2).sum(-1)
    else:
        ab = (A * B).sum(-1)
        if metric == 'angular':
            den = np.sqrt((A * A).sum(-1)) * np.sqrt((B * B).sum(-1))
            key = np.where(den > 0, 2.0 - 2.0 * np.divide(ab, den, out=np.zeros_like(ab), where=den > 0), 2.0)
        else:
            key = -ab
    return np.where(col_ids >= 0, key, np.inf)
