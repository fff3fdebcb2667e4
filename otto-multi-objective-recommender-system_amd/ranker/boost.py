"""The boosting loop of the two tree trainers (SPEC-GBDT, SPEC-XGB; DESIGN.md sections 3g and 3k): what ``gbdt.train`` and
``xgb.train`` share. A family brings its gradients, its tree growth and its validation metric as callables; the argument
checks, the scores, the workspace, the sampling schedule, the best-iteration bookkeeping, the early stop and its cut are
here, once.
"""
import collections

from .. import _lib
from . import gbdt

Boosted = collections.namedtuple('Boosted', 'trees leaves history best_iteration score start')
Boosted.__doc__ = """What :func:`boost` returns: ``trees``, the kept trees as ``grow`` made them; ``leaves``: per kept tree the
int32 [n] leaf of every training row (``keep_leaves``), else None; ``history``: the metric after every iteration;
``best_iteration`` = ``len(trees)``; ``score`` float64 [n] on the device: ``start`` plus the leaf values of ``trees`` in tree
order; ``start``: the value ``start()`` returned."""


def boost(bins, label, query_off, mapper, *, gradients, grow, work_bytes, start, metric, higher_is_better, no_tree,
          sampling=None, valid=None, num_boost_round=100, early_stopping_rounds=None, keep_leaves=False):
    """Boost trees over ``bins`` uint8 [F, n], ``label`` int32 [n], ``query_off`` int64 [Q+1]: a :class:`Boosted`.

    ``gradients(score, it) -> (grad, hess)`` float64 [n] at the scores of iteration ``it``;
    ``grow(gh, exp, bag, features, work) -> tree``, a ``gbdt.BinTree`` over the quantised gradients, ``work`` uint8
    [``work_bytes(n, F)``] allocated here once; ``start() -> float``: the value every training and validation score starts from,
    called once after the arguments have been checked (a family's set-up that reads the labels belongs in it);
    ``metric(valid_score) -> float`` with ``higher_is_better``; ``no_tree``: the text of the ``OttoError`` for a first tree
    without a split. ``valid`` = (bins, label, query_off); ``sampling``: a ``gbdt.Sampling`` or None.

    Per iteration: gradients, ``gbdt.quantize_gradients``, a new bag when ``it % bagging_freq == 0`` (seed
    ``mix(bagging_seed, 2 * (it // bagging_freq))``, kept in between), the feature list of the tree, ``grow``; a tree with
    fewer than two leaves ends boosting and is not kept; ``gbdt.add_tree`` on the training and the validation score; the
    metric. With ``early_stopping_rounds`` boosting stops once that many iterations have passed without a strict
    improvement, and the trees and the score are cut at the best iteration: the score is rebuilt from ``start`` by the
    same float64 additions in the same order, so it has the bits it had after that iteration."""
    import torch
    if sampling is not None and not isinstance(sampling, gbdt.Sampling):
        raise ValueError('sampling: expected a gbdt.Sampling (see sampling_from_params)')
    F, n = gbdt.check_bins(bins)
    dev = bins.device
    if mapper.n_features != F:
        raise ValueError(f'the mapper has {mapper.n_features} features, bins has {F}')
    score = torch.zeros(n, dtype=torch.float64, device=dev)
    gbdt._check_queries(score, label, query_off)
    if valid is not None:
        vbins, vlabel, voff = valid
        if gbdt.check_bins(vbins)[0] != F:
            raise ValueError('the validation bins have another feature count')
        vscore = torch.zeros(vbins.shape[1], dtype=torch.float64, device=dev)
        gbdt._check_queries(vscore, vlabel, voff)
    elif early_stopping_rounds:
        raise ValueError('early_stopping_rounds needs a validation set')
    work = torch.empty(work_bytes(n, F), dtype=torch.uint8, device=dev)
    first = float(start())
    if first != 0.0:
        score.fill_(first)
        if valid is not None:
            vscore.fill_(first)
    bag_on = sampling is not None and sampling.bag_active
    features_on = sampling is not None and sampling.features_active
    m = gbdt.bag_size(sampling.bagging_fraction, n) if bag_on else n       # refuses an empty bag before any launch
    trees, leaves, history = [], [], []
    best_metric, best_iter = None, 0
    bag = features = None
    for it in range(int(num_boost_round)):
        gh, exp = gbdt.quantize_gradients(*gradients(score, it))
        if bag_on and it % sampling.bagging_freq == 0:
            bag = gbdt.bag_rows(n, m, gbdt.mix(sampling.bagging_seed, 2 * (it // sampling.bagging_freq)), dev)
        if features_on:
            features = gbdt.sample_features(F, sampling.feature_fraction, sampling.feature_fraction_seed, it)
        tree = grow(gh, exp, bag, features, work)
        if tree.n_leaves < 2:
            break
        trees.append(tree)
        leaf = gbdt.add_tree(bins, tree, score, want_leaf=keep_leaves)
        if keep_leaves:
            leaves.append(leaf)
        if valid is not None:
            gbdt.add_tree(vbins, tree, vscore)
            value = metric(vscore)
            history.append(value)
            if best_metric is None or (value > best_metric if higher_is_better else value < best_metric):
                best_metric, best_iter = value, it + 1
            if early_stopping_rounds and it + 1 - best_iter >= int(early_stopping_rounds):
                break
    if not trees:
        raise _lib.OttoError(no_tree)
    if valid is None or not early_stopping_rounds:
        best_iter = len(trees)
    elif best_iter < len(trees):
        score.fill_(first)
        for tree in trees[:best_iter]:
            gbdt.add_tree(bins, tree, score)
    return Boosted(trees[:best_iter], leaves[:best_iter] if keep_leaves else None, history, best_iter, score, first)
