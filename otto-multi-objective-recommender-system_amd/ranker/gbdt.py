"""LambdaRank gradient-boosted tree training on the device (SPEC-GBDT): the bin mapper, thin Python
over ``include/otto_gbdt.h``, :func:`train` (the family's side of the boosting loop of ``ranker.boost``) and a LightGBM v3
model writer.

What this replaces in the reference: ``lgb.train`` on the (session, candidate) matrix, one model per event type and fold
(``src/ranker/lgb_trainer.py:134-165``). The caller keeps GroupKFold and the negative down-sampling
(``lgb_trainer.py:81-128``), hands over the float32 matrix of ``ranker.features.feature_matrix`` with the rows of a
session contiguous, and gets a :class:`~otto_amd.ranker.forest.Forest` that ``ranker.forest`` scores. LightGBM's own
arithmetic is not reproduced: SPEC-GBDT states what is computed. The ``binary`` objective and the NDCG, AUC and logloss
validation metrics (SPEC-OBJ) come from ``ranker.objectives``; :func:`train` takes them by name.
"""
import ctypes as C
import dataclasses

import numpy as np

from .. import _lib
from .forest import MAX_FEATURES, MAX_LEAVES, Forest

MAX_QUERY = 1024            # OTTO_GBDT_MAX_QUERY
MAX_EDGES = 254             # OTTO_GBDT_MAX_EDGES
NAN_BIN = 255               # OTTO_GBDT_NAN_BIN
SIGMOID_BINS = 1 << 20      # OTTO_GBDT_SIGMOID_BINS
MAX_LABEL = 31              # OTTO_GBDT_MAX_LABEL
SPLIT_WORDS = 12            # OTTO_GBDT_SPLIT_WORDS

# the values recorded in the reference's model dump and config (models/lightgbm/)
DEFAULTS = {
    'num_leaves': 128, 'min_data_in_leaf': 2000, 'min_sum_hessian_in_leaf': 1e-3, 'lambda_l2': 0.01, 'min_gain_to_split': 1e-5,
    'learning_rate': 0.1, 'lambdarank_truncation_level': 30, 'lambdarank_norm': True, 'sigmoid': 1.0, 'max_bin': 255,
    'eval_at': 20, 'objective': 'lambdarank', 'metric': 'map', 'is_unbalance': False, 'scale_pos_weight': 1.0,
    'boost_from_average': True,
}
# LightGBM's names of the objectives and metrics SPEC-GBDT and SPEC-OBJ implement -> the name used here
_OBJECTIVES = {'lambdarank': 'lambdarank', 'binary': 'binary'}
_METRICS = {'map': 'map', 'mean_average_precision': 'map', 'ndcg': 'ndcg', 'lambdarank': 'ndcg', 'rank_xendcg': 'ndcg',
            'xendcg': 'ndcg', 'xe_ndcg': 'ndcg', 'xe_ndcg_mart': 'ndcg', 'xendcg_mart': 'ndcg', 'auc': 'auc',
            'binary_logloss': 'logloss', 'binary': 'logloss'}
_DEFAULT_METRIC = {'lambdarank': 'ndcg', 'binary': 'logloss'}       # LightGBM's, behind metric = '' / 'default' only
_OBJECTIVE_KEYS = ('objective', 'objective_type', 'app', 'application', 'loss')
_METRIC_KEYS = ('metric', 'metrics', 'metric_types')
_UNBALANCE_KEYS = ('is_unbalance', 'unbalance', 'unbalanced_sets')
_ALIASES = {
    'min_child_samples': 'min_data_in_leaf', 'min_child_weight': 'min_sum_hessian_in_leaf', 'reg_lambda': 'lambda_l2',
    'reg_alpha': 'lambda_l1', 'min_split_gain': 'min_gain_to_split', 'eta': 'learning_rate', 'subsample': 'bagging_fraction',
    'colsample_bytree': 'feature_fraction', 'max_leaves': 'num_leaves', 'ndcg_eval_at': 'eval_at', 'map_eval_at': 'eval_at',
}
_ROUND_KEYS = {'num_iterations', 'num_iteration', 'n_iter', 'num_tree', 'num_trees', 'num_round', 'num_rounds', 'nrounds',
               'num_boost_round', 'n_estimators', 'max_iter', 'early_stopping_round', 'early_stopping_rounds', 'early_stopping',
               'n_iter_no_change'}


class BinMapper:
    """Per feature at most 254 strictly increasing float32 edges: ``edges`` float32 [F, 254] (row f holds ``n_edges[f]``
    edges, the rest is +inf padding), ``n_edges`` int32 [F]. ``bin(x)`` = the number of edges ``< x``; NaN -> 255."""

    def __init__(self, edges, n_edges):
        self.edges = np.ascontiguousarray(edges, dtype=np.float32)
        self.n_edges = np.ascontiguousarray(n_edges, dtype=np.int32)
        if self.edges.ndim != 2 or self.edges.shape[1] != MAX_EDGES or self.n_edges.shape != (self.edges.shape[0],):
            raise ValueError(f'edges: expected float32 [F, {MAX_EDGES}] and n_edges int32 [F]')
        if not 1 <= self.edges.shape[0] <= MAX_FEATURES:
            raise ValueError(f'F must be in [1, {MAX_FEATURES}] (got {self.edges.shape[0]})')
        for f, k in enumerate(self.n_edges):
            e = self.edges[f, :k]
            if not 0 <= k <= MAX_EDGES or np.isnan(e).any() or (k > 1 and not (e[1:] > e[:-1]).all()):
                raise ValueError(f'feature {f}: the edges must be at most {MAX_EDGES}, not NaN and strictly increasing')
        self._dev = {}

    @property
    def n_features(self):
        return self.edges.shape[0]

    def feature_edges(self, f):
        return self.edges[f, :self.n_edges[f]]

    def to(self, device):
        import torch
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.edges).to(device), torch.from_numpy(self.n_edges).to(device))
        return self._dev[device]


def fit_bins(sample, max_bin=255):
    """The :class:`BinMapper` of a row sample float32 [m, F] (host array or tensor), built in NumPy. Per feature, from the
    non-NaN sample values: ``d <= max_bin`` distinct values ``v_0 < ... < v_{d-1}`` give the edges ``v_0 .. v_{d-2}``;
    otherwise the edges are the deduplicated values at positions ``floor((i+1)*m/max_bin) - 1``, ``i = 0 .. max_bin-2``,
    of the ``m`` sorted values."""
    if hasattr(sample, 'detach'):
        sample = sample.detach().cpu().numpy()
    sample = np.asarray(sample)
    if sample.ndim != 2 or sample.dtype != np.float32:
        raise ValueError('sample: expected float32 [m, F]')
    max_bin = int(max_bin)
    if not 2 <= max_bin <= 255:
        raise ValueError(f'max_bin must be in [2, 255] (got {max_bin})')
    F = sample.shape[1]
    edges = np.full((F, MAX_EDGES), np.inf, dtype=np.float32)
    n_edges = np.zeros(F, dtype=np.int32)
    for f in range(F):
        v = sample[:, f]
        v = np.sort(v[~np.isnan(v)])
        u = np.unique(v)
        if u.size <= max_bin:
            e = u[:-1]
        else:
            m = v.size
            pos = (np.arange(1, max_bin, dtype=np.int64) * m) // max_bin - 1
            e = np.unique(v[pos])
        edges[f, :e.size] = e
        n_edges[f] = e.size
    return BinMapper(edges, n_edges)


def bin_matrix(X, mapper):
    """uint8 [F, n] (feature-major) bins of ``X`` float32 [n, >= F] on the device."""
    import torch
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError('X: expected a float32 tensor [n, >= F]')
    if X.device.type != 'cuda':
        raise _lib.OttoError('bin_matrix needs a ROCm device (no CPU fallback)')
    F = mapper.n_features
    if X.shape[1] < F:
        raise ValueError(f'X has {X.shape[1]} columns, the mapper reads {F}')
    n = int(X.shape[0])
    if n and (X.stride(1) != 1 or X.stride(0) < F):
        raise ValueError('X: expected row-major rows (stride(1) == 1)')
    ld = int(X.stride(0)) if n else max(int(X.shape[1]), 1)
    edges, n_edges = mapper.to(X.device)
    bins = torch.empty((F, n), dtype=torch.uint8, device=X.device)
    # X goes in as rows with the leading dimension ld (checked above): it may be a column slice of a wider matrix
    _lib.call('otto_gbdt_bin', X.device, _lib.ptr(X), ld, n, F, edges, n_edges, bins)
    return bins


_TABLES = {}


def sigmoid_table(sigma):
    """(table float64 [2^20], lo, factor) of SPEC-GBDT, from NumPy."""
    sigma = float(sigma)
    lo, hi = -25.0 / sigma, 25.0 / sigma
    factor = SIGMOID_BINS / (hi - lo)
    i = np.arange(SIGMOID_BINS, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(sigma * (lo + i / factor))), lo, factor


def discount_table():
    return 1.0 / np.log2(2.0 + np.arange(MAX_QUERY, dtype=np.float64))


def _tables(sigma, dev):
    import torch
    key = (float(sigma), dev)
    if key not in _TABLES:
        t, lo, factor = sigmoid_table(sigma)
        _TABLES[key] = (torch.from_numpy(t).to(dev), lo, factor, torch.from_numpy(discount_table()).to(dev))
    return _TABLES[key]


def _check_queries(score, label, query_off):
    import torch
    _lib.need(score, 'score', torch.float64, 1)
    _lib.need(label, 'label', torch.int32, 1, device=score.device)
    _lib.need(query_off, 'query_off', torch.int64, 1, device=score.device)
    if label.numel() != score.numel():
        raise ValueError(f'label has {label.numel()} rows, score has {score.numel()}')
    if query_off.numel() < 1:
        raise ValueError('query_off: expected int64 [Q+1]')


def gradient_outputs(score, out):
    """The (grad, hess) a gradient wrapper writes: ``out`` where the caller passed it, checked to be two float64 [n]
    tensors beside ``score``; otherwise two new ones."""
    import torch
    grad, hess = out if out is not None else (torch.empty_like(score), torch.empty_like(score))
    _lib.need(grad, 'grad', torch.float64, 1, device=score.device, numel=score.numel())
    _lib.need(hess, 'hess', torch.float64, 1, device=score.device, numel=score.numel())
    return grad, hess


def lambdarank_gradients(score, label, query_off, sigma=1.0, truncation_level=30, norm=True, out=None):
    """(grad, hess) float64 [n] of the LambdarankNDCG objective; ``score`` float64 [n], ``label`` int32 [n] in 0..31,
    ``query_off`` int64 [Q+1], on the device. Raises ``OttoError`` for a query longer than ``MAX_QUERY`` or a malformed
    ``query_off``: the rows of such a query are zero in ``out`` = (grad, hess), if the caller passed these tensors."""
    _check_queries(score, label, query_off)
    dev = score.device
    table, lo, factor, disc = _tables(sigma, dev)
    grad, hess = gradient_outputs(score, out)
    _lib.call('otto_gbdt_lambdarank', dev, score, label, query_off, query_off.numel() - 1, score.numel(), table, lo, factor, disc,
              float(sigma), int(truncation_level), int(bool(norm)), grad, hess)
    return grad, hess


def quantize_gradients(grad, hess):
    """(gh int32 [n, 2], exp int32 [2]) of SPEC-GBDT's quantisation, on the device."""
    import torch
    _lib.need(grad, 'grad', torch.float64, 1)
    _lib.need(hess, 'hess', torch.float64, 1, device=grad.device)
    if hess.numel() != grad.numel():
        raise ValueError('grad and hess differ in length')
    gh = torch.empty((grad.numel(), 2), dtype=torch.int32, device=grad.device)
    exp = torch.empty(2, dtype=torch.int32, device=grad.device)
    _lib.call('otto_gbdt_quantize', grad.device, grad, hess, grad.numel(), gh, exp)
    return gh, exp


def check_bins(bins):
    import torch
    _lib.need(bins, 'bins (bin_matrix)', torch.uint8, 2)
    return int(bins.shape[0]), int(bins.shape[1])


def _feature_list(features, F, dev):
    """``features`` (None, or an ascending list of feature ids inside [0, F)) as an int32 device tensor, or None."""
    import torch
    if features is None:
        return None
    if isinstance(features, torch.Tensor):
        return _lib.need(features, 'features', torch.int32, 1, device=dev)
    f = np.ascontiguousarray(features, dtype=np.int32)
    if f.ndim != 1 or not 1 <= f.size <= F or f[0] < 0 or f[-1] >= F or (f.size > 1 and not (f[1:] > f[:-1]).all()):
        raise ValueError(f'features: expected 1 to {F} strictly ascending feature ids inside [0, {F})')
    return torch.from_numpy(f).to(dev)


def _numel(t):
    """The length that goes with an optional device list (a bag, a feature list): 0 beside None."""
    return 0 if t is None else t.numel()


def leaf_histogram(bins, gh, rows, features=None):
    """int64 [3, F, 256] = (sum qg, sum qh, rows) of the leaf whose row ids are ``rows`` int32. ``features``: an ascending
    list of feature ids (a tree's feature sample); the planes of the other features are zero."""
    import torch
    F, n = check_bins(bins)
    _lib.need(rows, 'rows', torch.int32, 1, device=bins.device)
    hist = torch.empty((3, F, 256), dtype=torch.int64, device=bins.device)
    feats = _feature_list(features, F, bins.device)
    _lib.call('otto_gbdt_hist', bins.device, bins, n, F, gh, rows, rows.numel(), feats, _numel(feats), hist)
    return hist


def best_split(hist, mapper, exp, min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split, features=None):
    """The best split of a leaf histogram, or ``None``: dict(feature, bin, default_left, gain, cnt_left, g_left, h_left,
    cnt, g, h) with the integer sums as Python ints. ``features``: the search walks these features only, and the parent's
    sums (cnt, g, h) are those of the first of them."""
    import torch
    dev = hist.device
    _, n_edges = mapper.to(dev)
    out = torch.empty(SPLIT_WORDS, dtype=torch.int64, device=dev)
    feats = _feature_list(features, int(hist.shape[1]), dev)
    _lib.call('otto_gbdt_best_split', dev, hist, int(hist.shape[1]), n_edges, exp, int(min_data_in_leaf),
              float(min_sum_hessian_in_leaf), float(lambda_l2), float(min_gain_to_split), feats, _numel(feats), out)
    w = out.cpu().numpy()
    if not w[0]:
        return None
    return dict(feature=int(w[1]), bin=int(w[2]), default_left=int(w[3]), gain=float(w[4:5].view(np.float64)[0]),
                cnt_left=int(w[5]), g_left=int(w[6]), h_left=int(w[7]), cnt=int(w[8]), g=int(w[9]), h=int(w[10]))


def partition_rows(bins, rows, feature, bin, default_left):
    """(out int32 like ``rows``: the left rows in their order, then the right rows in theirs; n_left)."""
    import torch
    F, n = check_bins(bins)
    _lib.need(rows, 'rows', torch.int32, 1, device=bins.device)
    if not 0 <= int(feature) < F:
        raise ValueError(f'feature {feature} outside [0, {F})')
    out = torch.empty_like(rows)
    n_left = torch.zeros(1, dtype=torch.int64, device=bins.device)
    work = torch.empty(max(rows.numel() // 2048 + 1, 64), dtype=torch.int32, device=bins.device)
    _lib.call('otto_gbdt_partition', bins.device, bins, n, int(feature), int(bin), int(bool(default_left)), rows, rows.numel(), out,
              n_left, work, work.numel() * 4)
    return out, int(n_left.item())


class BinTree:
    """One tree in bin space (host arrays): ``split_feature``, ``split_bin``, ``default_left``, ``left_child``,
    ``right_child`` int32 [L-1], ``threshold`` float64, ``decision_type`` int8, ``split_gain`` float64, ``leaf_value``
    float64 [L], ``leaf_count`` int64 [L]; ``hist_rows``: rows the histogram kernel read for it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_leaves(self):
        return self.leaf_value.size

    def to(self, dev):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return (t(self.split_feature), t(self.split_bin), t(self.default_left), t(self.left_child), t(self.right_child),
                t(self.leaf_value))


def workspace_bytes(n, F, num_leaves):
    b = int(_lib.lib().otto_gbdt_workspace_bytes(int(n), int(F), int(num_leaves)))
    if b <= 0:
        raise _lib.OttoError(f'otto_gbdt_workspace_bytes refused n = {n}, F = {F}, num_leaves = {num_leaves}')
    return b


def grow_tree(bins, gh, exp, mapper, p, work=None, bag=None, features=None):
    """One leaf-wise tree: a :class:`BinTree`. ``p``: the resolved parameters (:func:`resolve_params`). ``bag``: int32
    ascending row ids on the device (:func:`bag_rows`), the rows the tree is grown on (None: all rows); ``features``: the
    ascending feature ids it may split on (:func:`sample_features`; None: all). With a bag, ``leaf_count`` and
    ``hist_rows`` count in-bag rows."""
    import torch
    F, n = check_bins(bins)
    dev = bins.device
    if bag is not None:
        _lib.need(bag, 'bag', torch.int32, 1, device=dev)
        if not 1 <= bag.numel() <= n:
            raise ValueError(f'bag has {bag.numel()} rows, bins has {n}')
    feats = _feature_list(features, F, dev)
    L = int(p['num_leaves'])
    if work is None:
        work = torch.empty(workspace_bytes(n, F, L), dtype=torch.uint8, device=dev)
    _, n_edges = mapper.to(dev)
    sf, sb, lc, rc = (np.zeros(L - 1, dtype=np.int32) for _ in range(4))
    thr, gain = np.zeros(L - 1, dtype=np.float64), np.zeros(L - 1, dtype=np.float64)
    dt = np.zeros(L - 1, dtype=np.int8)
    lv, cnt = np.zeros(L, dtype=np.float64), np.zeros(L, dtype=np.int64)
    n_leaves, hist_rows = C.c_int32(0), C.c_int64(0)
    # the NumPy arrays are host buffers: the edges the thresholds come from, and the tree the call writes
    _lib.call('otto_gbdt_grow_tree', dev, bins, n, F, gh, exp, n_edges, mapper.edges, L, int(p['min_data_in_leaf']),
              float(p['min_sum_hessian_in_leaf']), float(p['lambda_l2']), float(p['min_gain_to_split']), float(p['learning_rate']),
              bag, _numel(bag), feats, _numel(feats), C.byref(n_leaves), sf, sb, thr, dt, lc, rc, gain, lv, cnt,
              C.byref(hist_rows), work, work.numel())
    k = n_leaves.value
    return BinTree(split_feature=sf[:k - 1], split_bin=sb[:k - 1], default_left=((dt[:k - 1] & 2) >> 1).astype(np.int32),
                   left_child=lc[:k - 1], right_child=rc[:k - 1], threshold=thr[:k - 1], decision_type=dt[:k - 1],
                   split_gain=gain[:k - 1], leaf_value=lv[:k], leaf_count=cnt[:k], hist_rows=hist_rows.value)


def add_tree(bins, tree, score, want_leaf=False):
    """``score[r] += leaf_value[leaf(r)]`` by routing the bins through ``tree``; returns leaf(r) int32 [n] if asked."""
    import torch
    F, n = check_bins(bins)
    _lib.need(score, 'score', torch.float64, 1, device=bins.device)
    if score.numel() != n:
        raise ValueError(f'score has {score.numel()} rows, bins has {n}')
    dev = bins.device
    sf, sb, dl, lc, rc, lv = tree.to(dev)
    leaf = torch.empty(n, dtype=torch.int32, device=dev) if want_leaf else None
    _lib.call('otto_gbdt_add_tree', dev, bins, n, F, tree.n_leaves, sf, sb, dl, lc, rc, lv, score, leaf)
    return leaf


def ap_at_k(score, label, query_off, k=20):
    """Per-query AP@k float64 [Q] on the device (-1 for a query without a positive), in the objective's row order."""
    import torch
    _check_queries(score, label, query_off)
    k = int(k)
    if not 1 <= k <= MAX_QUERY:
        raise ValueError(f'k must be in [1, {MAX_QUERY}] (got {k})')
    dev = score.device
    ap = torch.empty(query_off.numel() - 1, dtype=torch.float64, device=dev)
    _lib.call('otto_gbdt_ap_at_k', dev, score, label, query_off, query_off.numel() - 1, score.numel(), k, ap)
    return ap


def mean_ap(ap):
    """The metric of SPEC-GBDT from per-query AP: ``np.sum(ap[ap >= 0]) / count`` on the host (nan without such a query)."""
    ap = ap.detach().cpu().numpy() if hasattr(ap, 'detach') else np.asarray(ap)
    ok = ap >= 0
    return float(np.sum(ap[ok]) / ok.sum()) if ok.any() else float('nan')


# ---- sampling (SPEC-GBDT, Sampling): the row bag and the per-tree feature subset

_M64 = (1 << 64) - 1
_SAMPLING_ALIASES = {'subsample': 'bagging_fraction', 'sub_row': 'bagging_fraction', 'bagging': 'bagging_fraction',
                     'subsample_freq': 'bagging_freq', 'colsample_bytree': 'feature_fraction', 'sub_feature': 'feature_fraction',
                     'bagging_fraction_seed': 'bagging_seed', 'sub_feature_bynode': 'feature_fraction_bynode',
                     'colsample_bynode': 'feature_fraction_bynode', 'pos_subsample': 'pos_bagging_fraction',
                     'pos_sub_row': 'pos_bagging_fraction', 'pos_bagging': 'pos_bagging_fraction',
                     'neg_subsample': 'neg_bagging_fraction', 'neg_sub_row': 'neg_bagging_fraction',
                     'neg_bagging': 'neg_bagging_fraction'}


def mix(s, i):
    """``mix(s, i)`` of SPEC-GBDT with Python integers: splitmix64's finaliser over ``s + (i + 1) * 0x9E3779B97F4A7C15``."""
    z = (int(s) + (int(i) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def bag_size(fraction, n):
    """``int(fraction * n)``: the float64 product, truncated (LightGBM's ``bag_data_cnt``). ``ValueError`` below 1."""
    m = int(float(fraction) * int(n))
    if m < 1:
        raise ValueError(f'bagging_fraction = {fraction} of {n} rows leaves an empty bag')
    return m


def n_used_features(F, fraction):
    """``max(min(2, F), floor(F * fraction + 0.5))``."""
    F = int(F)
    return max(min(2, F), int(np.floor(F * float(fraction) + 0.5)))


def sample_features(F, fraction, seed, it):
    """The feature list of the tree of iteration ``it``: int32, ascending, the :func:`n_used_features` features of
    ``[0, F)`` with the smallest ``mix(mix(seed, 2 * it + 1), f)``. NumPy uint64 on the host."""
    F = int(F)
    s = np.uint64(mix(seed, 2 * int(it) + 1))
    with np.errstate(over='ignore'):
        z = s + (np.arange(F, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        keys = z ^ (z >> np.uint64(31))
    return np.sort(np.argsort(keys, kind='stable')[:n_used_features(F, fraction)]).astype(np.int32)


def bag_rows(n, m, seed, device):
    """int32 [m] on ``device``, ascending: the ``m`` rows of ``[0, n)`` with the smallest ``mix(seed, r)``. ``seed`` is the
    already mixed ``mix(bagging_seed, 2 * d)`` of draw ``d``."""
    import torch
    n, m, seed = int(n), int(m), int(seed)
    if not 1 <= n < 1 << 31 or not 1 <= m <= n:
        raise ValueError(f'bag_rows: m = {m} of n = {n} rows (1 <= m <= n < 2^31)')
    if not 0 <= seed <= _M64:
        raise ValueError('seed: expected a uint64')
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.OttoError('bag_rows needs a ROCm device (no CPU fallback)')
    out = torch.empty(m, dtype=torch.int32, device=device)
    work = _lib.workspace(_lib.lib().otto_gbdt_bag_workspace_bytes(n), device)
    _lib.call('otto_gbdt_bag', device, n, m, seed, out, m, work, work.numel())
    return out


@dataclasses.dataclass(frozen=True)
class Sampling:
    """The sampling of SPEC-GBDT under LightGBM's key names. The row bag is active iff ``bagging_freq > 0`` and
    ``bagging_fraction < 1``, the per-tree feature sample iff ``feature_fraction < 1``. The sets come from SPEC-GBDT's
    pinned sampler, not from LightGBM's RNG: passing one to :func:`train` accepts that."""
    bagging_fraction: float = 1.0
    bagging_freq: int = 0
    feature_fraction: float = 1.0
    bagging_seed: int = 3
    feature_fraction_seed: int = 2

    def __post_init__(self):
        for key in ('bagging_fraction', 'feature_fraction'):
            v = float(getattr(self, key))
            if not 0.0 < v <= 1.0:
                raise ValueError(f'{key} = {v} outside (0, 1]')
            object.__setattr__(self, key, v)
        if int(self.bagging_freq) != self.bagging_freq or int(self.bagging_freq) < 0:
            raise ValueError(f'bagging_freq = {self.bagging_freq}: expected an integer >= 0')
        object.__setattr__(self, 'bagging_freq', int(self.bagging_freq))
        for key in ('bagging_seed', 'feature_fraction_seed'):
            v = int(getattr(self, key))
            if not 0 <= v <= _M64:
                raise ValueError(f'{key} = {v}: expected a uint64')
            object.__setattr__(self, key, v)

    @property
    def bag_active(self):
        return self.bagging_freq > 0 and self.bagging_fraction < 1.0

    @property
    def features_active(self):
        return self.feature_fraction < 1.0


def sampling_from_params(params):
    """``(rest, Sampling)``: ``config['model'][event_type]`` of the reference's YAML, whole, split into the sampling keys
    (``bagging_fraction``, ``bagging_freq``, ``feature_fraction``, ``bagging_seed``, ``feature_fraction_seed`` and their
    aliases; where a key stands beside one of its aliases the main name wins, as in LightGBM, whatever their order) and a
    ``rest`` that :func:`resolve_params` accepts. ``seed`` stays in ``rest`` and is ignored: LightGBM
    would derive the two sampling seeds from it, SPEC-GBDT does not. Raises ``ValueError``, naming the key, for
    ``feature_fraction_bynode < 1``, ``pos_bagging_fraction`` / ``neg_bagging_fraction != 1`` and whatever
    :class:`Sampling` refuses."""
    rest, kw = {}, {}
    params = dict(params or {})
    for key, val in params.items():
        name = _SAMPLING_ALIASES.get(key, key)
        if name != key and name in params:
            continue                                  # an alias beside its main name: the main name wins, as in LightGBM
        if name in ('bagging_fraction', 'bagging_freq', 'feature_fraction', 'bagging_seed', 'feature_fraction_seed'):
            kw[name] = val
        elif name == 'feature_fraction_bynode':
            if float(val) != 1.0:
                raise ValueError(f'feature_fraction_bynode = {val} is not supported (the feature sample is drawn per tree)')
        elif name in ('pos_bagging_fraction', 'neg_bagging_fraction'):
            if float(val) != 1.0:
                raise ValueError(f'{name} = {val} is not supported (no balanced bagging)')
        else:
            rest[key] = val
    return rest, Sampling(**kw)


def _flag(key, val):
    if isinstance(val, str) and val.lower() in ('true', 'false', '+', '-'):
        return val.lower() in ('true', '+')
    if val in (True, False, 0, 1):
        return bool(val)
    raise ValueError(f'{key} = {val!r}: expected a boolean')


def _metric_name(key, val, objective):
    """The first entry of a metric value (a name, a comma-separated string or a list) as one of map / ndcg / auc /
    logloss; '' and 'default' are LightGBM's default for the objective."""
    if isinstance(val, str):
        val = val.split(',')
    val = [str(v).strip() for v in (val if isinstance(val, (list, tuple)) else [val])]
    first = val[0] if val else ''
    if first in ('', 'default'):
        return _DEFAULT_METRIC[objective]
    if first not in _METRICS:
        raise ValueError(f'{key} = {first!r} is not supported (only {" / ".join(_METRICS)})')
    return _METRICS[first]


def resolve_params(params, extended=False):
    """``extended`` (what :func:`train` and ``folds.cross_validate`` pass): also accept SPEC-OBJ's objectives and metrics
    (DESIGN.md section 3l). ``objective``: ``lambdarank`` or ``binary``. ``metric`` (aliases ``metrics``, ``metric_types``;
    of a list or a comma-separated string the first entry decides): ``map`` / ``mean_average_precision``, ``ndcg`` /
    ``lambdarank`` (and LightGBM's xendcg aliases of it), ``auc``, ``binary_logloss`` / ``binary``; without the key the
    metric stays AP@``eval_at`` whatever the objective, and only an explicit ``''`` or ``'default'`` selects LightGBM's
    default for the objective (``ndcg`` for ``lambdarank``, ``binary_logloss`` for ``binary``). ``sigmoid``, ``is_unbalance``
    (aliases ``unbalance``, ``unbalanced_sets``), ``scale_pos_weight`` and ``boost_from_average`` are read for ``binary``;
    ``is_unbalance`` together with ``scale_pos_weight != 1`` is refused, as in LightGBM. Without ``extended`` the call keeps
    its first contract: ``lambdarank`` only, and these keys change nothing.

    LightGBM's key names and aliases -> the resolved dict. ``config['model'][event_type]`` of the reference's YAML can be
    passed once the keys SPEC-GBDT refuses are taken out (:func:`sampling_from_params` takes the sampling keys out and
    hands them to :func:`train` as a :class:`Sampling`). Raises ``ValueError`` for what changes the arithmetic and is not
    implemented: ``lambda_l1 != 0``, ``bagging_fraction < 1``, ``feature_fraction < 1``, ``feature_fraction_bynode < 1``,
    categorical features, ``max_depth > 0``, ``num_leaves`` above ``OTTO_FOREST_MAX_LEAVES``, an ``objective`` other than
    ``lambdarank``, a ``boosting`` other than ``gbdt``, a ``label_gain`` other than ``2^i - 1``; and for the round counts
    (``num_iterations``, ``early_stopping_round`` and their aliases), which are arguments of :func:`train`. Every other key
    (seeds, ``verbose``, ``n_jobs``, ``metric``, ...) changes no arithmetic here and is ignored. ``eval_at``: the first entry
    of a list is the k of the validation metric."""
    p = dict(DEFAULTS)
    params = dict(params or {})
    metric = None
    for key, val in params.items():
        key = _ALIASES.get(key, key)
        if key in _METRIC_KEYS:
            if key == 'metric' or 'metric' not in params:                 # the main name wins over its aliases
                metric = (key, val)
        elif key in _UNBALANCE_KEYS:
            if extended and (key == 'is_unbalance' or 'is_unbalance' not in params):
                p['is_unbalance'] = _flag(key, val)
        elif key == 'boost_from_average':
            if extended:
                p[key] = _flag(key, val)
        elif key == 'scale_pos_weight':
            if extended:
                p[key] = val
        elif key == 'lambda_l1':
            if float(val) != 0.0:
                raise ValueError('lambda_l1 != 0 is not supported (SPEC-GBDT has no L1 term)')
        elif key == 'bagging_fraction':
            if float(val) < 1.0:
                raise ValueError('bagging_fraction < 1 is not supported (the row sample would follow LightGBM\'s unpinned RNG)')
        elif key in ('feature_fraction', 'feature_fraction_bynode'):
            if float(val) < 1.0:
                raise ValueError(f'{key} < 1 is not supported (the column sample would follow LightGBM\'s unpinned RNG)')
        elif key in ('categorical_feature', 'categorical_features', 'cat_feature'):
            if val not in (None, '', 'auto') and len(val):
                raise ValueError('categorical features are not supported (numerical splits only)')
        elif key == 'max_depth':
            if int(val) > 0:
                raise ValueError('max_depth > 0 is not supported (growth is leaf-wise up to num_leaves)')
        elif key in _OBJECTIVE_KEYS:
            if str(val) not in (_OBJECTIVES if extended else ('lambdarank',)):
                raise ValueError(f'objective {val!r} is not supported (only {" / ".join(_OBJECTIVES) if extended else "lambdarank"})')
            if key == 'objective' or 'objective' not in params:
                p['objective'] = _OBJECTIVES[str(val)]
        elif key in ('boosting', 'boosting_type', 'boost'):
            if str(val) != 'gbdt':
                raise ValueError(f'boosting {val!r} is not supported (only gbdt)')
        elif key == 'label_gain':
            if val is not None and [float(g) for g in val] != [float(2 ** i - 1) for i in range(len(val))]:
                raise ValueError('a label_gain other than 2^i - 1 is not supported')
        elif key in _ROUND_KEYS:
            raise ValueError(f'{key} is not read from params: pass num_boost_round / early_stopping_rounds to train()')
        elif key in DEFAULTS:
            p[key] = val
        # anything else (seeds, verbose, n_jobs, metric, ...) changes no arithmetic here
    if isinstance(p['eval_at'], (list, tuple)):
        p['eval_at'] = p['eval_at'][0]
    p['num_leaves'], p['min_data_in_leaf'], p['eval_at'] = int(p['num_leaves']), int(p['min_data_in_leaf']), int(p['eval_at'])
    p['lambdarank_truncation_level'], p['max_bin'] = int(p['lambdarank_truncation_level']), int(p['max_bin'])
    p['lambdarank_norm'] = bool(p['lambdarank_norm'])
    for key in ('min_sum_hessian_in_leaf', 'lambda_l2', 'min_gain_to_split', 'learning_rate', 'sigmoid', 'scale_pos_weight'):
        p[key] = float(p[key])
    if extended and metric is not None:
        p['metric'] = _metric_name(metric[0], metric[1], p['objective'])
    if not p['scale_pos_weight'] > 0:
        raise ValueError(f'scale_pos_weight = {p["scale_pos_weight"]} must be positive')
    if p['is_unbalance'] and p['scale_pos_weight'] != 1.0:
        raise ValueError('is_unbalance and scale_pos_weight != 1 cannot be used together (LightGBM refuses the pair too)')
    if p['num_leaves'] > MAX_LEAVES:
        raise ValueError(f'num_leaves = {p["num_leaves"]} above OTTO_FOREST_MAX_LEAVES = {MAX_LEAVES}')
    if p['num_leaves'] < 2:
        raise ValueError(f'num_leaves = {p["num_leaves"]} below 2')
    if p['min_data_in_leaf'] < 0 or p['min_sum_hessian_in_leaf'] < 0 or p['lambda_l2'] < 0 or p['sigmoid'] <= 0 \
            or p['lambdarank_truncation_level'] < 1:
        raise ValueError('min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2 must be >= 0, sigmoid > 0, truncation level >= 1')
    return p


def forest_from_trees(trees, n_features, feature_names=None):
    """The :class:`Forest` of a list of :class:`BinTree`."""
    cat = lambda name, dtype: np.concatenate([getattr(t, name) for t in trees]).astype(dtype)
    node_off = np.concatenate([[0], np.cumsum([t.n_leaves - 1 for t in trees])]).astype(np.int64)
    leaf_off = np.concatenate([[0], np.cumsum([t.n_leaves for t in trees])]).astype(np.int64)
    return Forest(node_off, leaf_off, cat('split_feature', np.int32), cat('threshold', np.float64), cat('decision_type', np.int8),
                  cat('left_child', np.int32), cat('right_child', np.int32), cat('leaf_value', np.float64), n_features,
                  feature_names=feature_names, objective='lambdarank')


def split_sums(trees, n_features, name=None):
    """Per feature, over the splits on it in a :class:`BinTree` list: the float64 sum of the per-node array ``name``
    (``'split_gain'``, ``'cover'``, ...) added in tree order, or with ``name`` None the int64 number of splits. The one
    accumulation behind ``folds.feature_importance`` and ``xgb.feature_importance``."""
    out = np.zeros(int(n_features), dtype=np.int64 if name is None else np.float64)
    for t in trees:
        np.add.at(out, t.split_feature, 1 if name is None else getattr(t, name))
    return out


class TrainResult:
    """``forest``: the first ``best_iteration`` trees as a ``ranker.forest.Forest``; ``best_iteration``; ``history``: the
    validation metric after every iteration (empty without a validation set); ``train_score`` float64 [n] on the device:
    the raw score of every training row under ``forest``; ``trees``: the :class:`BinTree` list of ``forest``;
    ``train_leaf`` int32 [n, T]: the leaf the trainer put every row in."""

    def __init__(self, forest, best_iteration, history, train_score, trees, train_leaf):
        self.forest, self.best_iteration, self.history = forest, best_iteration, history
        self.train_score, self.trees, self.train_leaf = train_score, trees, train_leaf


def train(bins, label, query_off, mapper, params=None, valid=None, num_boost_round=100, early_stopping_rounds=None,
          feature_names=None, keep_leaves=False, sampling=None):
    """Boost LambdaRank trees on the device (SPEC-GBDT). ``bins`` uint8 [F, n] (:func:`bin_matrix`), ``label`` int32 [n],
    ``query_off`` int64 [Q+1]; ``valid`` = (bins, label, query_off) of a validation set binned with the same mapper: its
    mean AP@``eval_at`` is recorded after every tree, and with ``early_stopping_rounds`` training stops once that many
    iterations have passed without a strict improvement and the forest is cut at the best iteration. ``keep_leaves``
    also returns the leaf of every (row, tree). ``sampling``: a :class:`Sampling`; the bag is redrawn every
    ``bagging_freq`` iterations and the feature list for every tree, each tree is grown on its bag and list, and its
    values are added to the score of every row. Raises ``OttoError`` if not a single tree could be grown.

    ``params`` may also name SPEC-OBJ's ``binary`` objective and the metrics ``ndcg``, ``auc``, ``binary_logloss``
    (:func:`resolve_params` with ``extended``). ``binary``: positives are the rows with ``label > 0``; with
    ``boost_from_average`` every score starts at ``objectives.init_score`` and that value is added once into the leaf
    values of the first tree, so ``forest`` and ``trees`` scored from 0.0 return ``train_score``'s bits.
    ``binary_logloss`` stops early on a strict decrease, every other metric on a strict increase.

    The loop itself is ``boost.boost``, shared with ``xgb.train``: this function resolves the parameters, hands over its
    gradients, :func:`grow_tree` and ``objectives.evaluate``, and wraps the result."""
    import torch
    from . import boost, objectives
    p = resolve_params(params, extended=True)
    binary = p['objective'] == 'binary'
    w_pos = w_neg = 1.0

    def start():
        nonlocal w_pos, w_neg
        if not binary:
            return 0.0
        n_pos, n = objectives.label_counts(label)
        w_pos, w_neg = objectives.class_weights(n_pos, n, p['is_unbalance'], p['scale_pos_weight'])
        return objectives.init_score(n_pos, n, p['sigmoid']) if p['boost_from_average'] and n else 0.0

    def gradients(score, it):
        if binary:
            return objectives.binary_gradients(score, label, p['sigmoid'], w_pos, w_neg, 0.0)
        return lambdarank_gradients(score, label, query_off, p['sigmoid'], p['lambdarank_truncation_level'], p['lambdarank_norm'])

    b = boost.boost(
        bins, label, query_off, mapper, gradients=gradients, start=start,
        grow=lambda gh, exp, bag, features, work: grow_tree(bins, gh, exp, mapper, p, work, bag=bag, features=features),
        work_bytes=lambda n, F: workspace_bytes(n, F, p['num_leaves']),
        metric=lambda vscore: objectives.evaluate(p['metric'], vscore, valid[1], valid[2], k=p['eval_at'], minus=None,
                                                  sigma=p['sigmoid']),
        higher_is_better=objectives.HIGHER_IS_BETTER[p['metric']], sampling=sampling, valid=valid,
        num_boost_round=num_boost_round, early_stopping_rounds=early_stopping_rounds, keep_leaves=keep_leaves,
        no_tree='no tree could be grown: no split of the root is admissible (min_data_in_leaf, min_sum_hessian_in_leaf, '
                'min_gain_to_split) or every label of a query is the same')
    trees = b.trees
    if b.start != 0.0:
        # LightGBM's AddBias: 0.0 + (value + init) has the bits of init + value, so the trees score from 0.0 from here on
        first = BinTree(**trees[0].__dict__)
        first.leaf_value = first.leaf_value + np.float64(b.start)
        trees[0] = first
    train_leaf = torch.stack(b.leaves, dim=1).contiguous() if keep_leaves else None
    forest = forest_from_trees(trees, int(bins.shape[0]), feature_names)
    if binary:
        forest.objective = f'binary sigmoid:{p["sigmoid"]:g}'
    return TrainResult(forest, b.best_iteration, b.history, b.score, trees, train_leaf)


def write_lightgbm_model(forest, feature_names=None):
    """A text dump of ``forest`` in the layout of LightGBM's v3 model files, holding what
    :func:`~otto_amd.ranker.forest.parse_lightgbm_model` reads, and read back by it to identical arrays (every float is
    written with ``repr``, which round-trips a float64). It carries no ``feature_infos``, ``split_gain``, ``leaf_count`` or
    ``internal_*`` lines; whether LightGBM's own loader accepts it has not been tried. The ``objective`` line is the
    forest's: ``lambdarank``, or ``binary sigmoid:<sigma>`` for a model of :func:`train` with ``objective: binary`` (whose
    first tree carries the initial score, as LightGBM's does)."""
    names = list(feature_names) if feature_names is not None else list(forest.feature_names)
    if len(names) != forest.n_features:
        raise ValueError(f'{len(names)} feature_names for {forest.n_features} features')
    if any((not str(s)) or any(ch.isspace() for ch in str(s)) for s in names):
        raise ValueError('a feature name must be non-empty and hold no white space')
    ints = lambda a: ' '.join(str(int(x)) for x in a)
    floats = lambda a: ' '.join(repr(float(x)) for x in a)
    blocks = []
    for t in range(forest.n_trees):
        n0, n1, l0, l1 = (int(x) for x in (forest.node_off[t], forest.node_off[t + 1], forest.leaf_off[t], forest.leaf_off[t + 1]))
        lines = [f'Tree={t}', f'num_leaves={l1 - l0}', 'num_cat=0']
        if l1 - l0 > 1:
            lines += [f'split_feature={ints(forest.split_feature[n0:n1])}', f'threshold={floats(forest.threshold[n0:n1])}',
                      f'decision_type={ints(forest.decision_type[n0:n1])}', f'left_child={ints(forest.left_child[n0:n1])}',
                      f'right_child={ints(forest.right_child[n0:n1])}']
        lines += [f'leaf_value={floats(forest.leaf_value[l0:l1])}', 'is_linear=0', 'shrinkage=1']
        blocks.append('\n'.join(lines) + '\n\n')
    head = ['tree', 'version=v3', 'num_class=1', 'num_tree_per_iteration=1', 'label_index=0',
            f'max_feature_idx={forest.n_features - 1}', f'objective={forest.objective or "lambdarank"}',
            'feature_names=' + ' '.join(str(s) for s in names), 'tree_sizes=' + ' '.join(str(len(b)) for b in blocks)]
    return '\n'.join(head) + '\n\n' + ''.join(blocks) + 'end of trees\n'
