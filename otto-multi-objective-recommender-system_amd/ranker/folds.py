"""GroupKFold over the sessions, the index sets of a fold with the negative down-sampling, the gather of the binned
matrix, and the fold trainer that joins them to ``ranker.gbdt``, ``ranker.forest`` and ``ranker.evaluate`` (SPEC-FOLDS,
DESIGN.md section 3h): thin Python over ``include/otto_folds.h``.

What this replaces in the reference: the fold loop of ``src/ranker/lgb_trainer.py:81-198`` around ``lgb.train``:
``GroupKFold(n_splits=5)`` over the session ids, ``sample(frac=negative_sampling_ratio, random_state=42)`` over the
negatives of the training sessions that have a positive, the rebuilt query sizes, the out-of-fold predictions, recall@20
per fold and over all folds, and the gain and split feature importances. The fold assignment is scikit-learn's with the
tie order pinned; pandas' Mersenne-Twister permutation is deliberately not reproduced: the kept negatives are the ``m``
with the smallest ``splitmix64`` keys of their row index (SPEC-FOLDS states both).
"""
import collections
import ctypes as C

import numpy as np

from .. import _lib
from . import gbdt, xgb
from .forest import MAX_FEATURES

MAX_SPLITS = 16             # OTTO_FOLDS_MAX_SPLITS
BIN_SAMPLE_ROWS = 200000    # LightGBM's bin_construct_sample_cnt
_MAX_N = (1 << 31) - 1


def _check_query_off(query_off):
    import torch
    _lib.need(query_off, 'query_off', torch.int64, 1)
    if query_off.numel() < 1:
        raise ValueError('query_off: expected int64 [Q+1]')
    return query_off.numel() - 1


def _scratch(size_fn, dev, *args):
    """The workspace of the size ``size_fn(*args)`` asks for; a size <= 0 is the library's refusal of ``args``."""
    n_bytes = getattr(_lib.lib(), size_fn)(*args)
    if n_bytes <= 0:
        raise _lib.OttoError(f'{size_fn} refused its arguments')
    return _lib.workspace(n_bytes, dev)


def group_kfold(query_off, n_splits=5, n=None, timing=None):
    """(fold_of_query int32 [Q], fold_rows int64 [n_splits]) of SPEC-FOLDS on the device: queries in the order (size
    descending, index descending), each to the fold with the fewest rows so far (ties: the lowest fold). ``query_off``
    int64 [Q+1] on the device; ``n``: the row count, the bound the offsets are checked against (None: 2^31 - 1).
    ``timing``: a dict that receives ``walk_ms``, the device time of the sequential walk alone. Raises ``ValueError``
    unless ``2 <= n_splits <= 16`` and ``Q >= n_splits``, ``OttoError`` for a query of more than 1024 rows or offsets
    that do not ascend inside ``[0, n]``."""
    import torch
    n_splits = int(n_splits)
    if not 2 <= n_splits <= MAX_SPLITS:
        raise ValueError(f'n_splits must be in [2, {MAX_SPLITS}] (got {n_splits})')
    Q = _check_query_off(query_off)
    if Q < n_splits:
        raise ValueError(f'{Q} queries cannot fill {n_splits} folds')
    n = _MAX_N if n is None else int(n)
    if not 0 <= n <= _MAX_N:
        raise ValueError(f'n = {n} outside [0, 2^31)')
    dev = query_off.device
    # the outputs are handed over only after the call succeeded: a refused call leaves nothing behind
    fold_of_query = torch.empty(Q, dtype=torch.int32, device=dev)
    fold_rows = torch.empty(n_splits, dtype=torch.int64, device=dev)
    walk_ms = C.c_float(0.0)
    work = _scratch('otto_folds_kfold_workspace', dev, Q)
    _lib.call('otto_folds_group_kfold', dev, query_off, Q, n, n_splits, fold_of_query, fold_rows,
              C.byref(walk_ms) if timing is not None else None, work, work.numel())
    if timing is not None:
        timing['walk_ms'] = float(walk_ms.value)
    return fold_of_query, fold_rows


def sample_size(ratio, n_eligible):
    """``int(round(ratio * N))``: float64 product, half to even; the count ``pandas.Series.sample(frac=)`` returns."""
    return int(round(float(ratio) * int(n_eligible)))


class FoldIndices:
    """The index sets of one fold, on the device: ``train_idx`` int32 [Mt] ascending, ``train_query_off`` int64 [Qt+1],
    ``train_query`` int32 [Qt], ``val_idx`` int32 [Mv], ``val_query_off`` int64 [Qv+1], ``val_query`` int32 [Qv];
    ``n_eligible``: the eligible negatives N, ``n_kept``: the m of them in ``train_idx``, ``n_positive``: the training
    positives."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def fold_indices(label, query_off, fold_of_query, fold, ratio, seed=42):
    """The :class:`FoldIndices` of fold ``fold`` (SPEC-FOLDS): every row of the fold's queries validates; of the other
    queries, those with a positive give their positives and the ``m = int(round(ratio * N))`` of all ``N`` such queries'
    negatives with the smallest ``splitmix64(seed, row)`` keys. ``label`` uint8 or int32 [n], ``query_off`` int64 [Q+1],
    ``fold_of_query`` int32 [Q], on the device. The host reads back ``N`` and the output sizes, nothing else."""
    import torch
    if not isinstance(label, torch.Tensor) or label.dtype not in (torch.uint8, torch.int32):
        raise ValueError('label: expected a contiguous 1-d uint8 or int32 tensor')
    _lib.need(label, 'label', label.dtype, 1)
    dev = label.device
    Q = _check_query_off(query_off)
    _lib.need(fold_of_query, 'fold_of_query', torch.int32, 1, device=dev)
    if query_off.device != dev:
        raise ValueError(f'query_off must be on {dev}')
    if fold_of_query.numel() != Q:
        raise ValueError(f'fold_of_query has {fold_of_query.numel()} entries for {Q} queries')
    n = label.numel()
    if n > _MAX_N:
        raise ValueError(f'n = {n} outside [0, 2^31)')
    fold, ratio, seed = int(fold), float(ratio), int(seed)
    if not 0 <= fold < MAX_SPLITS:
        raise ValueError(f'fold must be in [0, {MAX_SPLITS}) (got {fold})')
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f'ratio must be in [0, 1] (got {ratio})')
    if not 0 <= seed < 1 << 64:
        raise ValueError('seed: expected a uint64')
    counts = (C.c_int64 * 5)()
    state = _scratch('otto_folds_state_bytes', dev, n)
    _lib.call('otto_folds_classify', dev, label, label.element_size(), query_off, Q, n, fold_of_query, fold, state, counts)
    N, P, Mv, Qt, Qv = (int(c) for c in counts)
    m = sample_size(ratio, N)
    Mt = P + m
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
    out = FoldIndices(train_idx=i32(Mt), train_query_off=i64(Qt + 1), train_query=i32(Qt), val_idx=i32(Mv),
                      val_query_off=i64(Qv + 1), val_query=i32(Qv), n_eligible=N, n_kept=m, n_positive=P)
    work = _scratch('otto_folds_emit_workspace', dev, Q)
    _lib.call('otto_folds_emit', dev, state, query_off, Q, n, N, m, seed, Mt, Qt, Mv, Qv, out.train_idx, out.train_query_off,
              out.train_query, out.val_idx, out.val_query_off, out.val_query, work, work.numel())
    return out


def gather_bins(bins, idx):
    """``out[f, i] = bins[f, idx[i]]``: uint8 [F, m] from ``bins`` uint8 [F, n] (``gbdt.bin_matrix``) and ``idx`` int32
    [m] on the device; any order, repeats allowed. Raises ``OttoError`` for an index outside ``[0, n)``."""
    import torch
    F, n = gbdt.check_bins(bins)
    _lib.need(idx, 'idx', torch.int32, 1, device=bins.device)
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f'F must be in [1, {MAX_FEATURES}] (got {F})')
    out = torch.empty((F, idx.numel()), dtype=torch.uint8, device=bins.device)
    _lib.call('otto_folds_gather_u8', bins.device, bins, n, F, idx, idx.numel(), out)
    return out


def feature_importance(trees, n_features):
    """(gain float64 [F], split int64 [F]): the sum of ``split_gain`` and the number of splits per feature over a
    ``BinTree`` list, in NumPy on the host. LightGBM's ``feature_importance('gain' | 'split')`` counts the splits with a
    positive gain; every split of SPEC-GBDT has one."""
    return gbdt.split_sums(trees, n_features, 'split_gain'), gbdt.split_sums(trees, n_features)


class CVResult:
    """``forests``: one ``ranker.forest.Forest`` per fold; ``trees``: their ``BinTree`` lists; ``best_iterations``,
    ``histories``: per fold, as ``gbdt.TrainResult``; ``mappers``: the fold's ``BinMapper``; ``oof_prediction`` float32
    [n] on the device; ``fold_of_query`` int32 [Q], ``fold_rows`` int64 [n_splits]; ``importance_gain`` float64 and
    ``importance_split`` int64 [F, n_splits], ``importance_cover`` float64 [F, n_splits] (``booster='xgboost'`` only, else
    None). With ``aid`` and ``truth``: ``top_aid`` int32 [Q, 20] and ``top_n``, the
    out-of-fold top-20 of every session; ``fold_hits``, ``fold_denom``, ``fold_recall``: per fold; ``hits``, ``denom``,
    ``recall``: over all folds (otherwise None)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _lightgbm_resolve(params, sampling):
    return gbdt.resolve_params(params, extended=True)


def _lightgbm_oof(res, val_bins, X, val_idx):
    import torch
    score = torch.zeros(val_bins.shape[1], dtype=torch.float64, device=val_bins.device)
    for tree in res.trees:
        gbdt.add_tree(val_bins, tree, score)
    return score


def _xgboost_resolve(params, sampling):
    if sampling is not None:
        raise ValueError("sampling: with booster='xgboost' subsample / colsample_bytree / seed are keys of params")
    return xgb.resolve_params(params, extended=True)[0]


# What cross_validate asks of a booster. resolve(params, sampling) -> the resolved dict; train(*data, params, sampling,
# **kw) -> a TrainResult; oof_score(result, val_bins, X, val_idx) -> the raw float64 score of the validation rows;
# importances(trees, F) -> the per-feature columns (gain, split[, cover]).
_Booster = collections.namedtuple('_Booster', 'resolve train oof_score importances')
_BOOSTERS = {
    'lightgbm': _Booster(_lightgbm_resolve, lambda *data, params, sampling, **kw: gbdt.train(*data, params, sampling=sampling, **kw),
                         _lightgbm_oof, feature_importance),
    'xgboost': _Booster(_xgboost_resolve, lambda *data, params, sampling, **kw: xgb.train(*data, params, **kw),
                        lambda res, val_bins, X, val_idx: xgb.predict(res, X[val_idx.long()], output_margin=True),
                        xgb.feature_importance),
}


def cross_validate(X, label, query_off, params, n_splits=5, negative_sampling_ratio=0.3, seed=42, num_boost_round=100,
                   early_stopping_rounds=None, feature_names=None, aid=None, truth=None, sampling=None, booster='lightgbm'):
    """The fold loop of ``lgb_trainer.py:81-198`` (and of ``xgb_trainer.py:81-200``) on the device: a :class:`CVResult`.

    ``booster='xgboost'`` trains the XGBoost family instead (``ranker.xgb``): ``params`` under XGBoost's key names
    (``xgb.resolve_params``; ``sampling`` must stay None, the sampling keys are part of ``params``), ``xgb.train``, the
    out-of-fold prediction by ``xgb.predict`` (``base_score`` included), and the importances of ``xgb.feature_importance``:
    ``importance_gain`` (mean gain per split), ``importance_split`` (= weight) and ``importance_cover`` (None for
    ``'lightgbm'``). Everything else in the loop is the same.

    ``params`` may name SPEC-OBJ's objectives and metrics (``objective: binary`` / ``binary:logistic`` / ``rank:ndcg``,
    ``metric`` / ``eval_metric``: ``ndcg``, ``auc``, ``binary_logloss`` / ``logloss``): both trainers
    take them as they are. The out-of-fold prediction of a binary model is its raw score (the blend rescales every column
    anyway); ``objectives.transform`` turns it into a probability.

    ``X`` float32 [n, F] (``ranker.features.feature_matrix``), ``label`` uint8 or int32 [n], ``query_off`` int64 [Q+1]
    (the ``row_off`` of ``ranker_table``), on the device; ``params`` and ``sampling`` as ``gbdt.train`` takes them
    (``gbdt.sampling_from_params`` makes both from a section of the reference's config). :func:`group_kfold`
    once, then per fold: :func:`fold_indices`; a ``BinMapper`` from ``gbdt.fit_bins`` (host) over at most 200,000 evenly
    strided training rows, ``train_idx[::ceil(Mt / 200000)]``; ``gbdt.bin_matrix`` over all rows; :func:`gather_bins` of
    the training and validation rows; ``gbdt.train(..., valid=...)``; the validation score by ``gbdt.add_tree`` over the
    kept trees, written as float32 at ``val_idx`` into the out-of-fold prediction; the importances.

    ``aid`` int32 [n] and ``truth`` = (off int64 [Q+1], aid int32), the label lists of ``ranker.evaluate`` aligned with
    the queries, add recall@20: ``forest.session_topk`` over the out-of-fold prediction and ``evaluate.hits`` with the
    fold as the mask. Test-time averaging of the folds' models is ``forest.ensemble_predict(result.forests, X_test)``."""
    import torch
    from . import evaluate
    from .forest import session_topk
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError('X: expected a float32 tensor [n, F]')
    if X.device.type != 'cuda':
        raise _lib.OttoError('cross_validate needs a ROCm device (no CPU fallback)')
    dev = X.device
    n, F = int(X.shape[0]), int(X.shape[1])
    if label.numel() != n:
        raise ValueError(f'label has {label.numel()} rows, X has {n}')
    if booster not in _BOOSTERS:
        raise ValueError(f"booster = {booster!r}: expected 'lightgbm' or 'xgboost'")
    family = _BOOSTERS[booster]
    p = family.resolve(params, sampling)
    n_splits = int(n_splits)
    fold_of_query, fold_rows = group_kfold(query_off, n_splits, n=n)
    label32 = label if label.dtype == torch.int32 else label.to(torch.int32)
    oof = torch.zeros(n, dtype=torch.float32, device=dev)
    forests, trees, best, histories, mappers = [], [], [], [], []
    importances = []
    for fold in range(n_splits):
        fi = fold_indices(label, query_off, fold_of_query, fold, negative_sampling_ratio, seed)
        Mt = fi.train_idx.numel()
        stride = max(-(-Mt // BIN_SAMPLE_ROWS), 1)
        mapper = gbdt.fit_bins(X[fi.train_idx[::stride].long()], p['max_bin'])
        bins = gbdt.bin_matrix(X, mapper)
        train_bins, val_bins = gather_bins(bins, fi.train_idx), gather_bins(bins, fi.val_idx)
        del bins
        train_label, val_label = label32[fi.train_idx.long()], label32[fi.val_idx.long()]
        res = family.train(train_bins, train_label, fi.train_query_off, mapper, params=params, sampling=sampling,
                           valid=(val_bins, val_label, fi.val_query_off), num_boost_round=num_boost_round,
                           early_stopping_rounds=early_stopping_rounds, feature_names=feature_names)
        oof[fi.val_idx.long()] = family.oof_score(res, val_bins, X, fi.val_idx).to(torch.float32)
        forests.append(res.forest)
        trees.append(res.trees)
        best.append(res.best_iteration)
        histories.append(res.history)
        mappers.append(mapper)
        importances.append(family.importances(res.trees, F))
    imp_gain, imp_split, imp_cover = ([np.stack(columns, axis=1) for columns in zip(*importances)] + [None])[:3]
    out = CVResult(forests=forests, trees=trees, best_iterations=best, histories=histories, mappers=mappers, oof_prediction=oof,
                   fold_of_query=fold_of_query, fold_rows=fold_rows, importance_gain=imp_gain, importance_split=imp_split, importance_cover=imp_cover,
                   top_aid=None, top_n=None, fold_hits=None, fold_denom=None, fold_recall=None, hits=None, denom=None, recall=None)
    if (aid is None) != (truth is None):
        raise ValueError('recall@20 needs both aid and truth')
    if aid is not None:
        top_aid, _, top_n = session_topk(oof.to(torch.float64), aid, query_off, k=20)
        out.top_aid, out.top_n = top_aid, top_n
        out.fold_hits, out.fold_denom, out.fold_recall = [], [], []
        for fold in range(n_splits):
            _, _, t = evaluate.hits(truth, (top_aid, top_n), cap=20, mask=(fold_of_query == fold).to(torch.uint8))
            out.fold_hits.append(t['mask_hits'])
            out.fold_denom.append(t['mask_denom'])
            out.fold_recall.append(evaluate._ratio(t['mask_hits'], t['mask_denom']))
            out.hits, out.denom = t['hits'], t['denom']
        out.recall = evaluate._ratio(out.hits, out.denom)
    return out
