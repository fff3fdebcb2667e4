"""The XGBoost ranker family on the device (SPEC-XGB): the ``rank:pairwise`` objective, depth-wise
trees, :func:`train` (the family's side of the boosting loop of ``ranker.boost``) and an XGBoost JSON model writer / parser;
thin Python over ``include/otto_xgb.h`` and the pieces of ``ranker.gbdt`` it shares (bins, quantisation, row bag, feature
sample, ``add_tree``, AP).

What this replaces in the reference: ``xgb.train`` on the (session, candidate) matrix, one model per event type and fold
(``src/ranker/xgb_trainer.py:134-165``), whose out-of-fold scores are the ``gunes_xgboost_*`` columns of the final blend
(``src/ranker/inference.py:64-85``). The reference keeps no XGBoost config: the defaults here are XGBoost 1.7's documented
ones. XGBoost's own arithmetic is not reproduced and the library is not available to this project: SPEC-XGB states what
is computed, ``tests/xgb_restatement.py`` pins it, and parity with a run of xgboost is neither claimed nor tested.
``rank:ndcg``, ``binary:logistic`` and the ``ndcg`` / ``auc`` / ``logloss`` metrics are SPEC-OBJ's (DESIGN.md section 3l,
``ranker.objectives``).
"""
import ctypes as C
import json

import numpy as np

from .. import _lib
from . import gbdt
from .forest import Forest, ModelFormatError, forest_predict
from .gbdt import MAX_QUERY, mix

MAX_DEPTH = 10              # OTTO_XGB_MAX_DEPTH
_ROOT_PARENT = 2147483647   # XGBoost's "no parent"

# XGBoost 1.7's documented defaults (max_bin: 256 there, 255 here, see resolve_params)
DEFAULTS = {'max_depth': 6, 'min_child_weight': 1.0, 'lambda': 1.0, 'gamma': 0.0, 'eta': 0.3, 'max_bin': 255, 'base_score': 0.5,
            'subsample': 1.0, 'colsample_bytree': 1.0, 'seed': 0, 'eval_metric': 'map', 'objective': 'rank:pairwise',
            'scale_pos_weight': 1.0}
OBJECTIVES = ('rank:pairwise', 'rank:ndcg', 'binary:logistic')        # what resolve_params(extended=True) accepts
_ALIASES = {'learning_rate': 'eta', 'min_split_loss': 'gamma', 'reg_lambda': 'lambda', 'reg_alpha': 'alpha', 'random_state': 'seed'}
# key -> the only value(s) accepted
_ONLY = {'objective': ('rank:pairwise',), 'booster': ('gbtree',), 'tree_method': ('hist', 'gpu_hist', 'auto'),
         'grow_policy': ('depthwise',), 'sampling_method': ('uniform',)}
_ONLY_NUMBER = {'max_leaves': 0, 'alpha': 0, 'max_delta_step': 0, 'colsample_bylevel': 1, 'colsample_bynode': 1,
                'scale_pos_weight': 1, 'num_pairsample': 1, 'num_parallel_tree': 1}


def derived_seeds(seed):
    """(objective_seed, bagging_seed, feature_fraction_seed) = (mix(seed, 1), mix(seed, 2), mix(seed, 3))."""
    return mix(seed, 1), mix(seed, 2), mix(seed, 3)


def parse_metric(name):
    """``(metric, k, minus)`` of an ``eval_metric`` string: ``map`` / ``ndcg`` with an optional ``@k`` (default: the whole
    query) and an optional trailing ``-`` (a query without a positive counts 0.0, not 1.0), ``auc``, ``logloss``; None for
    anything else."""
    name = str(name)
    if name in ('auc', 'logloss'):
        return name, MAX_QUERY, False
    minus = name.endswith('-')
    head, _, k = (name[:-1] if minus else name).partition('@')
    if head not in ('map', 'ndcg') or (k and not k.isdigit()) or ('@' in name and not k):
        return None
    k = int(k) if k else MAX_QUERY
    return (head, k, minus) if 1 <= k <= MAX_QUERY else None


def resolve_params(params, extended=False):
    """``extended`` (what :func:`train`, :func:`write_xgboost_json` and ``folds.cross_validate`` pass): also accept SPEC-OBJ's
    objectives and metrics: ``objective`` in ``rank:pairwise`` / ``rank:ndcg`` / ``binary:logistic``;
    ``eval_metric`` in ``map``, ``map-``, ``map@k``, ``ndcg``, ``ndcg-``, ``ndcg@k`` and, with ``binary:logistic`` only,
    ``auc`` and ``logloss`` (``p['metric']`` = :func:`parse_metric` of it); ``scale_pos_weight`` with ``binary:logistic``
    (it stays refused for the rank objectives), whose ``base_score`` must lie inside (0, 1). Without ``extended`` the call
    keeps its first contract: ``rank:pairwise`` with ``map`` / ``map-``.

    XGBoost's key names and aliases -> ``(p, sampling)``: the resolved dict (``max_depth``, ``min_child_weight``,
    ``lambda``, ``gamma``, ``eta``, ``max_bin``, ``base_score``, ``subsample``, ``colsample_bytree``, ``seed``,
    ``eval_metric``, ``objective_seed``) and the ``gbdt.Sampling`` that ``subsample`` / ``colsample_bytree`` / ``seed`` map
    to. Aliases: ``learning_rate``, ``min_split_loss``, ``reg_lambda``, ``reg_alpha``, ``random_state``; where a key stands
    beside its alias the main name wins. ``max_bin``: 255 here; XGBoost's default of 256 is accepted and treated as 255
    (bin 255 is reserved for NaN), anything larger is refused. Raises ``ValueError`` naming the key for what would change
    the arithmetic and is not implemented (the list in SPEC-XGB). Keys that change no arithmetic (``nthread``,
    ``verbosity``, ``predictor``, ``gpu_id``, ...) are ignored."""
    params = dict(params or {})
    p = dict(DEFAULTS)
    for key, val in params.items():
        name = _ALIASES.get(key, key)
        if name != key and name in params:
            continue
        if extended and name == 'objective':
            if str(val) not in OBJECTIVES:
                raise ValueError(f'{key} = {val!r} is not supported (only {" / ".join(OBJECTIVES)})')
            p[name] = str(val)
        elif extended and name == 'scale_pos_weight':
            p[name] = val
        elif name in _ONLY:
            if str(val) not in _ONLY[name]:
                raise ValueError(f'{key} = {val!r} is not supported (only {" / ".join(_ONLY[name])})')
        elif name in _ONLY_NUMBER:
            if float(val) != _ONLY_NUMBER[name]:
                raise ValueError(f'{key} = {val!r} is not supported (only {_ONLY_NUMBER[name]})')
        elif name == 'eval_metric':
            if isinstance(val, (list, tuple)):
                if len(val) != 1:
                    raise ValueError(f'eval_metric = {val!r}: expected one metric, map or map-')
                val = val[0]
            if val not in ('map', 'map-') and not (extended and parse_metric(val)):
                raise ValueError(f'eval_metric = {val!r} is not supported (only map / map-' +
                                 (' / map@k / ndcg / ndcg- / ndcg@k / auc / logloss)' if extended else ')'))
            p[name] = val
        elif name in DEFAULTS:
            p[name] = val
    p['max_depth'], p['max_bin'], p['seed'] = int(p['max_depth']), int(p['max_bin']), int(p['seed'])
    for key in ('min_child_weight', 'lambda', 'gamma', 'eta', 'base_score', 'subsample', 'colsample_bytree', 'scale_pos_weight'):
        p[key] = float(p[key])
    p['metric'] = parse_metric(p['eval_metric'])
    if p['objective'] == 'binary:logistic':
        if not p['scale_pos_weight'] > 0:
            raise ValueError(f'scale_pos_weight = {p["scale_pos_weight"]} must be positive')
        if not 0.0 < p['base_score'] < 1.0:
            raise ValueError(f'base_score = {p["base_score"]} outside (0, 1): binary:logistic starts from its logit')
    else:
        if p['scale_pos_weight'] != 1.0:
            raise ValueError(f'scale_pos_weight = {p["scale_pos_weight"]} is not supported with {p["objective"]} (only 1)')
        if p['metric'][0] in ('auc', 'logloss'):
            raise ValueError(f'eval_metric = {p["eval_metric"]!r} needs objective binary:logistic')
    if not 1 <= p['max_depth'] <= MAX_DEPTH:
        raise ValueError(f'max_depth = {p["max_depth"]} outside [1, {MAX_DEPTH}] (0, "no limit", is not supported)')
    if p['max_bin'] == 256:
        p['max_bin'] = 255
    if not 2 <= p['max_bin'] <= 255:
        raise ValueError(f'max_bin = {p["max_bin"]} outside [2, 256]')
    if p['min_child_weight'] < 0 or p['lambda'] < 0 or p['gamma'] < 0 or p['min_child_weight'] + p['lambda'] <= 0:
        raise ValueError('min_child_weight, lambda, gamma must be >= 0 and min_child_weight + lambda > 0')
    for key in ('subsample', 'colsample_bytree'):
        if not 0.0 < p[key] <= 1.0:
            raise ValueError(f'{key} = {p[key]} outside (0, 1]')
    if not 0 <= p['seed'] < 1 << 64:
        raise ValueError('seed: expected a uint64')
    if not np.isfinite(p['base_score']) or not np.isfinite(p['eta']):
        raise ValueError('base_score and eta must be finite')
    p['objective_seed'], bagging_seed, feature_seed = derived_seeds(p['seed'])
    sampling = gbdt.Sampling(bagging_fraction=p['subsample'], bagging_freq=1 if p['subsample'] < 1.0 else 0,
                             feature_fraction=p['colsample_bytree'], bagging_seed=bagging_seed, feature_fraction_seed=feature_seed)
    return p, sampling


def pairwise_gradients(score, label, query_off, seed, it, out=None):
    """(grad, hess) float64 [n] of SPEC-XGB's ``rank:pairwise``; ``score`` float64 [n], ``label`` int32 [n] in 0..31,
    ``query_off`` int64 [Q+1], on the device; ``seed``: the objective seed (``derived_seeds(xgb_seed)[0]``), ``it``: the
    0-based iteration. Raises ``OttoError`` for a query longer than ``MAX_QUERY``, a malformed ``query_off`` or a label
    outside 0..31: the rows of a refused query are zero in ``out`` = (grad, hess), if the caller passed these tensors."""
    return lambdamart_gradients(score, label, query_off, seed, it, weighting=0, out=out)


def lambdamart_gradients(score, label, query_off, seed, it, weighting=1, out=None):
    """The pairwise objective of ``otto_xgb_lambdamart``, arguments as :func:`pairwise_gradients` takes them:
    ``weighting = 0`` is ``rank:pairwise``, ``weighting = 1`` is SPEC-OBJ's ``rank:ndcg`` (every pair weighted by the
    |delta NDCG| of swapping its rows)."""
    gbdt._check_queries(score, label, query_off)
    dev = score.device
    table, lo, factor, disc = gbdt._tables(1.0, dev)
    grad, hess = gbdt.gradient_outputs(score, out)
    _lib.call('otto_xgb_lambdamart', dev, score, label, query_off, query_off.numel() - 1, score.numel(), table, lo, factor,
              mix(seed, it), int(weighting), disc, grad, hess)
    return grad, hess


class XgbTree(gbdt.BinTree):
    """A ``gbdt.BinTree`` grown depth-wise, plus per internal node ``cover`` (H), ``sum_grad`` (G) float64, ``count`` int64,
    ``left_id`` / ``right_id`` int32 (XGBoost's node ids of the children; the root is 0), per leaf ``leaf_cover``,
    ``leaf_sum_grad`` float64, and ``n_syncs``: the stream synchronisations the library counted inside the call."""


def workspace_bytes(n, F, max_depth):
    b = int(_lib.lib().otto_xgb_workspace_bytes(int(n), int(F), int(max_depth)))
    if b <= 0:
        raise _lib.OttoError(f'otto_xgb_workspace_bytes refused n = {n}, F = {F}, max_depth = {max_depth}')
    return b


def grow_tree(bins, gh, exp, mapper, p, work=None, bag=None, features=None):
    """One depth-wise tree: an :class:`XgbTree`. ``p``: the resolved parameters (:func:`resolve_params`); ``bag`` and
    ``features`` as ``gbdt.grow_tree`` takes them."""
    import torch
    F, n = gbdt.check_bins(bins)
    dev = bins.device
    if bag is not None:
        _lib.need(bag, 'bag', torch.int32, 1, device=dev)
        if not 1 <= bag.numel() <= n:
            raise ValueError(f'bag has {bag.numel()} rows, bins has {n}')
    feats = gbdt._feature_list(features, F, dev)
    depth = int(p['max_depth'])
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f'max_depth = {depth} outside [1, {MAX_DEPTH}]')
    L = 1 << depth
    if work is None:
        work = torch.empty(workspace_bytes(n, F, depth), dtype=torch.uint8, device=dev)
    _, n_edges = mapper.to(dev)
    a = dict(split_feature=np.zeros(L - 1, np.int32), split_bin=np.zeros(L - 1, np.int32), threshold=np.zeros(L - 1, np.float64),
             decision_type=np.zeros(L - 1, np.int8), left_child=np.zeros(L - 1, np.int32), right_child=np.zeros(L - 1, np.int32),
             split_gain=np.zeros(L - 1, np.float64), cover=np.zeros(L - 1, np.float64), sum_grad=np.zeros(L - 1, np.float64),
             count=np.zeros(L - 1, np.int64), left_id=np.zeros(L - 1, np.int32), right_id=np.zeros(L - 1, np.int32),
             leaf_value=np.zeros(L, np.float64), leaf_cover=np.zeros(L, np.float64), leaf_sum_grad=np.zeros(L, np.float64),
             leaf_count=np.zeros(L, np.int64))
    out = _lib.XgbTree(**{k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()})
    # mapper.edges is a host buffer: the thresholds come from it
    _lib.call('otto_xgb_grow_tree', dev, bins, n, F, gh, exp, n_edges, mapper.edges, depth, float(p['min_child_weight']),
              float(p['lambda']), float(p['gamma']), float(p['eta']), bag, gbdt._numel(bag), feats, gbdt._numel(feats),
              C.byref(out), work, work.numel())
    k = out.n_leaves
    tree = {name: (v[:k] if name.startswith('leaf_') else v[:k - 1]) for name, v in a.items()}
    tree['default_left'] = ((tree['decision_type'] & 2) >> 1).astype(np.int32)
    return XgbTree(hist_rows=out.hist_rows, n_syncs=out.n_syncs, **tree)


def _nodes(nodes):
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    if nodes.ndim != 2 or nodes.shape[1] != 8 or nodes.shape[0] < 1:
        raise ValueError('nodes: expected int32 [n_nodes, 8] = (begin, cnt, slot, slot2, 0, feature, bin, default_left)')
    return nodes


def level_histograms(bins, gh, rows, nodes, n_slots, features=None, hist=None):
    """One level's histogram launch (``otto_xgb_level_hist``): int64 [n_slots, 3, F, 256]. ``nodes`` int32 [k, 8] on the
    host: slot ``nodes[i, 2]`` receives the histogram of ``rows[begin : begin + cnt]``; then slot ``nodes[i, 3]`` (if
    >= 0) has it subtracted. ``hist``: the slots to work on (another slot keeps what it held); None: zeros."""
    import torch
    F, n = gbdt.check_bins(bins)
    dev = bins.device
    _lib.need(rows, 'rows', torch.int32, 1, device=dev)
    nodes = _nodes(nodes)
    feats = gbdt._feature_list(features, F, dev)
    if hist is None:
        hist = torch.zeros((int(n_slots), 3, F, 256), dtype=torch.int64, device=dev)
    _lib.need(hist, 'hist', torch.int64, 4, device=dev, numel=int(n_slots) * 3 * F * 256)
    work = _lib.workspace(workspace_bytes(rows.numel(), 1, 1), dev)
    _lib.call('otto_xgb_level_hist', dev, bins, n, F, gh, rows, rows.numel(), nodes, nodes.shape[0], feats, gbdt._numel(feats),
              hist, int(n_slots), work, work.numel())
    return hist


def level_splits(hist, mapper, exp, nodes, min_child_weight=1.0, lam=1.0, gamma=0.0, features=None):
    """One level's split search (``otto_xgb_level_split``): int64 [k, SPLIT_WORDS] on the host, one record per node, over
    ``hist`` int64 [n_slots, 3, F, 256]."""
    import torch
    dev = hist.device
    _lib.need(hist, 'hist', torch.int64, 4, device=dev)
    F = int(hist.shape[2])
    nodes = _nodes(nodes)
    _, n_edges = mapper.to(dev)
    feats = gbdt._feature_list(features, F, dev)
    out = torch.empty((nodes.shape[0], gbdt.SPLIT_WORDS), dtype=torch.int64, device=dev)
    work = _lib.workspace(workspace_bytes(0, 1, 1), dev)
    _lib.call('otto_xgb_level_split', dev, hist, int(hist.shape[0]), F, n_edges, exp, nodes, nodes.shape[0], float(min_child_weight),
              float(lam), float(gamma), feats, gbdt._numel(feats), out, work, work.numel())
    return out.cpu().numpy()


def level_partition(bins, rows, nodes):
    """One level's partition launch (``otto_xgb_level_partition``): ``(out int32 like rows, n_left int64 [k] on the
    host)``. Inside every node's range the rows that go left under (feature, bin, default_left) keep their order, then the
    others in theirs; positions outside every range keep what ``out`` held (a copy of ``rows``)."""
    import torch
    F, n = gbdt.check_bins(bins)
    dev = bins.device
    _lib.need(rows, 'rows', torch.int32, 1, device=dev)
    nodes = _nodes(nodes)
    out = rows.clone()
    n_left = torch.zeros(nodes.shape[0], dtype=torch.int64, device=dev)
    work = _lib.workspace(workspace_bytes(rows.numel(), 1, 1), dev)
    _lib.call('otto_xgb_level_partition', dev, bins, n, F, rows, rows.numel(), nodes, nodes.shape[0], out, n_left, work, work.numel())
    return out, n_left.cpu().numpy()


def mean_average_precision(ap, minus=False):
    """SPEC-XGB's ``map`` from per-query AP (``gbdt.ap_at_k`` at k = MAX_QUERY): a query without a positive (-1) counts
    1.0, with ``minus`` (``map-``) 0.0; ``np.sum(ap) / Q`` in float64 on the host (nan without a query)."""
    from . import objectives
    return objectives.query_mean(ap, minus)


def feature_importance(trees, n_features):
    """(gain float64 [F], weight int64 [F], cover float64 [F]) over an :class:`XgbTree` list as ``Booster.get_score``
    defines them: the mean ``split_gain`` per split of the feature, the number of splits, the mean ``cover`` per split. A
    feature that was never used gets 0 (XGBoost leaves it out; ``xgb_trainer.py:175-180`` adds into zeros)."""
    gain, cover = gbdt.split_sums(trees, n_features, 'split_gain'), gbdt.split_sums(trees, n_features, 'cover')
    weight = gbdt.split_sums(trees, n_features)
    used = weight > 0
    gain[used] /= weight[used]
    cover[used] /= weight[used]
    return gain, weight, cover


def _base_margin(base_score, objective):
    """What a raw score starts from: ``base_score`` itself for the rank objectives (SPEC-XGB), its logit for
    ``binary:logistic`` (SPEC-OBJ; exactly 0.0 at 0.5)."""
    from . import objectives
    return objectives.base_margin(base_score) if objective == 'binary:logistic' else float(base_score)


class TrainResult(gbdt.TrainResult):
    """``gbdt.TrainResult`` plus ``base_score`` and ``base_margin``: ``train_score`` = ``base_margin`` + the forest's raw
    score; ``base_margin`` is ``base_score`` itself, or its logit for ``binary:logistic``."""

    def __init__(self, base_score, *args, objective='rank:pairwise'):
        super().__init__(*args)
        self.base_score = float(base_score)
        self.objective = objective
        self.base_margin = _base_margin(base_score, objective)


class XgbModel:
    """What :func:`parse_xgboost_json` returns: ``forest`` (a ``ranker.forest.Forest``), ``base_score``,
    ``feature_names``, ``objective``."""

    def __init__(self, forest, base_score, feature_names, objective):
        self.forest, self.base_score, self.feature_names, self.objective = forest, float(base_score), feature_names, objective
        self.base_margin = _base_margin(base_score, objective)


def train(bins, label, query_off, mapper, params=None, valid=None, num_boost_round=10, early_stopping_rounds=None,
          feature_names=None):
    """Boost depth-wise ``rank:pairwise`` trees on the device (SPEC-XGB): a :class:`TrainResult`. Arguments as
    ``gbdt.train``; ``params`` under XGBoost's key names (:func:`resolve_params`); the defaults of the two round arguments
    are ``xgb.train``'s. The score of iteration ``it`` is ``base_score + margin``, ``margin`` the leaf values of the trees
    so far added in tree order from 0.0: the float64 operations of :func:`predict`. ``valid``: its ``map`` / ``map-`` is
    recorded after every tree; early stopping on a strict improvement, cut at the best iteration. Boosting stops at a tree
    whose root has no admissible split. Raises ``OttoError`` if not a single tree could be grown.

    The loop itself is ``boost.boost``, shared with ``gbdt.train``: this function resolves the parameters, hands over its
    gradients, :func:`grow_tree` and ``objectives.evaluate``, and wraps the result."""
    from . import boost, objectives
    p, sampling = resolve_params(params, extended=True)
    objective = p['objective']
    base = _base_margin(p['base_score'], objective)
    metric, metric_k, minus = p['metric']

    def gradients(margin, it):
        if objective == 'binary:logistic':
            return objectives.binary_gradients(margin + base, label, 1.0, p['scale_pos_weight'], 1.0, 1e-16)
        return lambdamart_gradients(margin + base, label, query_off, p['objective_seed'], it, int(objective == 'rank:ndcg'))

    b = boost.boost(
        bins, label, query_off, mapper, gradients=gradients, start=lambda: 0.0,
        grow=lambda gh, exp, bag, features, work: grow_tree(bins, gh, exp, mapper, p, work, bag=bag, features=features),
        work_bytes=lambda n, F: workspace_bytes(n, F, p['max_depth']),
        metric=lambda vmargin: objectives.evaluate(metric, vmargin + base, valid[1], valid[2], k=metric_k, minus=minus),
        higher_is_better=objectives.HIGHER_IS_BETTER[metric], sampling=sampling, valid=valid,
        num_boost_round=num_boost_round, early_stopping_rounds=early_stopping_rounds,
        no_tree='no tree could be grown: no split of the root is admissible (min_child_weight, gamma) or every label of a '
                'query is the same')
    forest = gbdt.forest_from_trees(b.trees, int(bins.shape[0]), feature_names)
    forest.objective = objective
    return TrainResult(p['base_score'], forest, b.best_iteration, b.history, b.score + base, b.trees, None, objective=objective)


def predict(model, X, output_margin=False):
    """``base_margin + forest_predict(model.forest, X)`` float64 [n] on the device; ``model``: a :class:`TrainResult` or
    an :class:`XgbModel`. A ``binary:logistic`` model returns the probability ``sigmoid(margin)`` unless
    ``output_margin``; for the rank objectives the margin is the prediction and ``base_margin`` is ``base_score``."""
    margin = forest_predict(model.forest, X) + model.base_margin
    if model.objective == 'binary:logistic' and not output_margin:
        from . import objectives
        return objectives.transform(margin)
    return margin


# ---- XGBoost's JSON model layout

def split_condition(edge):
    """XGBoost routes left on ``x < split_condition``, SPEC-GBDT on ``x <= edge``: ``nextafter32(edge, +inf)``; for every
    float32 ``x``, ``x < nextafter32(e) <=> x <= e``."""
    return np.nextafter(np.asarray(edge, dtype=np.float32), np.float32(np.inf))


def threshold_of(condition):
    """The inverse of :func:`split_condition`: ``nextafter32(condition, -inf)``. An edge of -0.0 comes back as +0.0: both
    zeros have the same condition, and ``x <= -0.0 <=> x <= +0.0``."""
    return np.nextafter(np.asarray(condition, dtype=np.float32), np.float32(-np.inf))


def _tree_json(t, k, F, lam, eta):
    """The tree object of tree ``t`` (an :class:`XgbTree`) with the nodes in XGBoost id order."""
    L = t.n_leaves
    N = 2 * L - 1
    node_id, leaf_id = np.zeros(L - 1, np.int64), np.zeros(L, np.int64)
    for s in range(L - 1):                                  # a parent's step precedes its children's
        for child, cid in ((t.left_child[s], t.left_id[s]), (t.right_child[s], t.right_id[s])):
            if child >= 0:
                node_id[child] = cid
            else:
                leaf_id[~child] = cid
    left, right, parents = np.full(N, -1, np.int64), np.full(N, -1, np.int64), np.full(N, _ROOT_PARENT, np.int64)
    split_idx, default_left = np.zeros(N, np.int64), np.zeros(N, np.int64)
    cond, base_w, loss, hess = (np.zeros(N, np.float32) for _ in range(4))
    for s in range(L - 1):
        i = node_id[s]
        left[i], right[i] = t.left_id[s], t.right_id[s]
        parents[t.left_id[s]] = parents[t.right_id[s]] = i
        split_idx[i], default_left[i] = t.split_feature[s], t.default_left[s]
        cond[i] = split_condition(np.float32(t.threshold[s]))
        base_w[i] = np.float32(-(t.sum_grad[s] / (t.cover[s] + lam)) * eta)
        loss[i], hess[i] = np.float32(t.split_gain[s]), np.float32(t.cover[s])
    for leaf in range(L):
        i = leaf_id[leaf]
        cond[i] = base_w[i] = np.float32(t.leaf_value[leaf])
        hess[i] = np.float32(t.leaf_cover[leaf])
    ints = lambda a: [int(x) for x in a]
    floats = lambda a: [float(x) for x in a]
    return {'base_weights': floats(base_w), 'categories': [], 'categories_nodes': [], 'categories_segments': [],
            'categories_sizes': [], 'default_left': ints(default_left), 'id': k, 'left_children': ints(left),
            'loss_changes': floats(loss), 'parents': ints(parents), 'right_children': ints(right), 'split_conditions': floats(cond),
            'split_indices': ints(split_idx), 'split_type': [0] * N, 'sum_hessian': floats(hess),
            'tree_param': {'num_deleted': '0', 'num_feature': str(F), 'num_nodes': str(N), 'size_leaf_vector': '0'}}


def write_xgboost_json(result, feature_names=None, params=None):
    """The model of a :class:`TrainResult` as text in XGBoost's published JSON model layout (version [1, 7, 2]):
    ``learner.learner_model_param`` (``base_score``, ``num_feature``, ``num_class``), ``learner.objective.name``,
    ``learner.gradient_booster.model`` (``gbtree_model_param``, ``tree_info``, ``trees[]`` with the node structure, the
    split data, the statistics and the bookkeeping), nodes in XGBoost id order, a leaf with children -1 and its value in
    ``split_conditions``, every float a float32. ``split_condition = nextafter32(edge, +inf)`` (:func:`split_condition`).
    ``params``: the training parameters (``lambda`` and ``eta`` enter ``base_weights`` of the internal nodes; default: the
    defaults). The layout is restated from XGBoost's documentation; the file has never been loaded by xgboost itself (the
    library is not available to this project). :func:`parse_xgboost_json` reads it back to identical arrays."""
    p, _ = resolve_params(params, extended=True)
    objective = getattr(result, 'objective', None) or p['objective']
    if objective == 'binary:logistic':
        objective_json = {'name': objective, 'reg_loss_param': {'scale_pos_weight': repr(float(p['scale_pos_weight']))}}
    else:
        objective_json = {'lambda_rank_param': {'fix_list_weight': '0', 'num_pairsample': '1'}, 'name': objective}
    forest = result.forest
    F = forest.n_features
    names = list(feature_names) if feature_names is not None else list(forest.feature_names)
    if len(names) != F:
        raise ValueError(f'{len(names)} feature_names for {F} features')
    trees = [_tree_json(t, k, F, p['lambda'], p['eta']) for k, t in enumerate(result.trees)]
    model = {'learner': {
        'attributes': {}, 'feature_names': [str(s) for s in names], 'feature_types': ['float'] * F,
        'gradient_booster': {'model': {'gbtree_model_param': {'num_parallel_tree': '1', 'num_trees': str(len(trees)),
                                                               'size_leaf_vector': '0'},
                                       'tree_info': [0] * len(trees), 'trees': trees}, 'name': 'gbtree'},
        'learner_model_param': {'base_score': repr(float(result.base_score)), 'boost_from_average': '1',
                                'num_class': '0', 'num_feature': str(F), 'num_target': '1'},
        'objective': objective_json},
        'version': [1, 7, 2]}
    return json.dumps(model)


def _expect(cond, msg):
    if not cond:
        raise ModelFormatError(msg)


def parse_xgboost_json(text):
    """An :class:`XgbModel` from XGBoost's JSON model text: ``gbtree`` with numerical splits and ``num_class <= 1``
    (``ModelFormatError`` otherwise). The forest follows SPEC-GBDT's numbering applied in ascending node id: internal
    node ``s`` is the ``s``-th split node by id, its left child keeps the leaf index, the right child is leaf ``s + 1``;
    ``threshold = nextafter32(split_condition, -inf)`` (:func:`threshold_of`), ``decision_type`` NaN-missing with the
    node's default direction."""
    try:
        doc = json.loads(text)
        learner = doc['learner']
        lp = learner['learner_model_param']
        booster = learner['gradient_booster']
        _expect(booster.get('name') == 'gbtree', f'gradient_booster {booster.get("name")!r}: only gbtree')
        model = booster['model']
        trees_in = model['trees']
        base_score, F, num_class = float(lp['base_score']), int(lp['num_feature']), int(lp.get('num_class', 0))
        objective = learner.get('objective', {}).get('name', '')
    except ModelFormatError:
        raise
    except (KeyError, TypeError, ValueError) as e:
        raise ModelFormatError(f'not an XGBoost JSON model: {e!r}') from e
    _expect(num_class <= 1, f'num_class = {num_class}: only single-output models')
    _expect(len(trees_in) >= 1, 'the model holds no tree')
    _expect(int(model.get('gbtree_model_param', {}).get('num_parallel_tree', 1)) == 1, 'num_parallel_tree != 1')
    _expect(all(int(g) == 0 for g in model.get('tree_info', [])), 'tree_info names more than one group')
    out = {k: [] for k in ('split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value')}
    node_off, leaf_off = [0], [0]
    for k, t in enumerate(trees_in):
        try:
            left, right = np.asarray(t['left_children'], np.int64), np.asarray(t['right_children'], np.int64)
            cond = np.asarray(t['split_conditions'], np.float64).astype(np.float32)
            idx, dleft = np.asarray(t['split_indices'], np.int64), np.asarray(t['default_left'], np.int64)
            stype = np.asarray(t.get('split_type', [0] * left.size), np.int64)
        except (KeyError, TypeError, ValueError) as e:
            raise ModelFormatError(f'tree {k}: {e!r}') from e
        N = left.size
        _expect(N >= 1 and all(a.shape == (N,) for a in (right, cond, idx, dleft, stype)), f'tree {k}: node arrays differ in length')
        _expect(not stype.any() and not t.get('categories') and not t.get('categories_nodes'), f'tree {k}: categorical splits')
        internal = left >= 0
        _expect(((right >= 0) == internal).all(), f'tree {k}: a node with one child')
        ids = np.flatnonzero(internal)
        _expect(N == 2 * ids.size + 1, f'tree {k}: {N} nodes with {ids.size} splits')
        for a in (left[ids], right[ids]):
            _expect(((a > ids) & (a < N)).all(), f'tree {k}: a child id outside (parent, num_nodes)')
        _expect(((idx[ids] >= 0) & (idx[ids] < F)).all(), f'tree {k}: a split index outside [0, {F})')
        _expect(not np.isnan(cond).any(), f'tree {k}: a NaN split condition or leaf value')
        step = {int(v): s for s, v in enumerate(ids)}
        leaf_of = {0: 0}
        lc, rc = np.zeros(ids.size, np.int32), np.zeros(ids.size, np.int32)
        lv = np.zeros(ids.size + 1, np.float64)
        seen = 1
        for s, v in enumerate(ids):
            v = int(v)
            _expect(v in leaf_of, f'tree {k}: node {v} is not reached from the root')
            a, b = int(left[v]), int(right[v])
            _expect(a not in leaf_of and b not in leaf_of and a != b, f'tree {k}: node {a} or {b} has two parents')
            leaf_of[a], leaf_of[b] = leaf_of.pop(v), s + 1
            seen += 2
            lc[s] = step[a] if internal[a] else ~leaf_of[a]
            rc[s] = step[b] if internal[b] else ~leaf_of[b]
        _expect(seen == N, f'tree {k}: {N - seen} nodes are not reached from the root')
        for v, leaf in leaf_of.items():
            lv[leaf] = np.float64(cond[v])
        _expect(np.isfinite(lv).all(), f'tree {k}: a leaf value is not finite')
        out['split_feature'].append(idx[ids].astype(np.int32))
        out['threshold'].append(threshold_of(cond[ids]).astype(np.float64))
        out['decision_type'].append(((2 << 2) | np.where(dleft[ids] != 0, 2, 0)).astype(np.int8))
        out['left_child'].append(lc)
        out['right_child'].append(rc)
        out['leaf_value'].append(lv)
        node_off.append(node_off[-1] + ids.size)
        leaf_off.append(leaf_off[-1] + ids.size + 1)
    cat = lambda name: np.concatenate(out[name])
    names = learner.get('feature_names') or None
    if names is not None:
        _expect(len(names) == F, f'{len(names)} feature_names for num_feature = {F}')
    forest = Forest(node_off, leaf_off, cat('split_feature'), cat('threshold'), cat('decision_type'), cat('left_child'),
                    cat('right_child'), cat('leaf_value'), F, feature_names=names, objective=objective)
    return XgbModel(forest, base_score, forest.feature_names, objective)
