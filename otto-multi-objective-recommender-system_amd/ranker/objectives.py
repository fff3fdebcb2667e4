"""Objectives and validation metrics the two tree trainers share (SPEC-OBJ): thin Python over
``include/otto_objective.h`` and the host halves the spec leaves to float64 NumPy -- the class weights and the initial score
of the ``binary`` objective, the means of NDCG, the AUC ratio, the logloss mean, and the metric dispatch of ``gbdt.train``
and ``xgb.train``.

What this adds over the reference: its trainers use ``lambdarank`` / ``rank:pairwise`` with MAP only. A pointwise binary
classifier on the candidate labels, NDCG, AUC and logloss are what LightGBM and XGBoost users expect of a candidate ranker.
"""
import ctypes as C

import numpy as np

from .. import _lib

MAX_QUERY = 1024            # OTTO_GBDT_MAX_QUERY
LOGLOSS_PARTS = 1024        # OTTO_OBJ_LOGLOSS_PARTS


def constants():
    """dict(threads, max_blocks, sort_tile, scan_tile, logloss_parts) of the kernels, for tests and tools."""
    out = (C.c_int32 * 5)()
    _lib.lib().otto_obj_constants(out)
    return dict(zip(('threads', 'max_blocks', 'sort_tile', 'scan_tile', 'logloss_parts'), (int(v) for v in out)))


def _tables(dev):
    from . import gbdt
    return gbdt._tables(1.0, dev)


def _rows(score, label):
    import torch
    _lib.need(score, 'score', torch.float64, 1)
    _lib.need(label, 'label', torch.int32, 1, device=score.device, numel=score.numel())


def binary_gradients(score, label, sigma=1.0, w_pos=1.0, w_neg=1.0, hess_floor=0.0, out=None):
    """(grad, hess) float64 [n] of SPEC-OBJ's pointwise logistic objective; ``score`` float64 [n], ``label`` int32 [n] in
    0..31 (positive: > 0), on the device. Raises ``OttoError`` for a label outside 0..31: such a row's outputs are zero in
    ``out`` = (grad, hess), if the caller passed these tensors."""
    from . import gbdt
    _rows(score, label)
    dev = score.device
    table, lo, factor, _ = _tables(dev)
    grad, hess = gbdt.gradient_outputs(score, out)
    _lib.call('otto_obj_binary', dev, score, label, score.numel(), table, lo, factor, float(sigma), float(w_pos), float(w_neg),
              float(hess_floor), grad, hess)
    return grad, hess


def label_counts(label):
    """(positives, rows) of ``label`` int32 [n] on the device, as Python ints."""
    import torch
    _lib.need(label, 'label', torch.int32, 1)
    out = torch.empty(2, dtype=torch.int64, device=label.device)
    _lib.call('otto_obj_label_counts', label.device, label, label.numel(), out)
    n_pos, n = out.cpu().tolist()
    return int(n_pos), int(n)


def class_weights(n_pos, n, is_unbalance=False, scale_pos_weight=1.0):
    """(w_pos, w_neg) of LightGBM's ``binary``: ``is_unbalance`` gives 1 to the larger class and ``cnt_large / cnt_small``
    to the smaller one (a class without a row keeps 1); ``w_pos`` is then multiplied by ``scale_pos_weight``."""
    w_pos, w_neg = 1.0, 1.0
    n_pos, n_neg = int(n_pos), int(n) - int(n_pos)
    if is_unbalance and n_pos > 0 and n_neg > 0:
        if n_pos > n_neg:
            w_neg = float(n_pos) / float(n_neg)
        else:
            w_pos = float(n_neg) / float(n_pos)
    return w_pos * float(scale_pos_weight), w_neg


def init_score(n_pos, n, sigma=1.0):
    """LightGBM's ``boost_from_average`` of ``binary``: ``log(pavg / (1 - pavg)) / sigma``, ``pavg = clip(n_pos / n, 1e-15,
    1 - 1e-15)``, float64 on the host."""
    pavg = np.float64(n_pos) / np.float64(n)
    pavg = min(max(pavg, np.float64(1e-15)), np.float64(1.0 - 1e-15))
    return float(np.log(pavg / (1.0 - pavg)) / np.float64(sigma))


def base_margin(base_score):
    """XGBoost's ``binary:logistic``: ``log(base_score / (1 - base_score))``; exactly 0.0 at 0.5."""
    b = np.float64(base_score)
    return float(np.log(b / (1.0 - b)))


def ndcg_at_k(score, label, query_off, k=MAX_QUERY):
    """Per-query NDCG@k float64 [Q] on the device; -1 for a query whose ideal DCG is 0 (no positive, or no row)."""
    import torch
    from . import gbdt
    gbdt._check_queries(score, label, query_off)
    k = int(k)
    if not 1 <= k <= MAX_QUERY:
        raise ValueError(f'k must be in [1, {MAX_QUERY}] (got {k})')
    dev = score.device
    out = torch.empty(query_off.numel() - 1, dtype=torch.float64, device=dev)
    _lib.call('otto_obj_ndcg_at_k', dev, score, label, query_off, query_off.numel() - 1, score.numel(), k, _tables(dev)[3], out)
    return out


def query_mean(values, minus=False):
    """The mean of a per-query figure (float64 [Q], device tensor or array) over all queries: a query without a positive
    (-1) counts 1.0, with ``minus`` 0.0; ``np.sum / Q`` in float64 on the host (nan without a query)."""
    v = values.detach().cpu().numpy() if hasattr(values, 'detach') else np.asarray(values, dtype=np.float64)
    v = np.where(v < 0, 0.0 if minus else 1.0, v)
    return float(np.sum(v) / v.size) if v.size else float('nan')


def mean_ndcg(ndcg, minus=False):
    """:func:`query_mean` of per-query NDCG: LightGBM's and XGBoost's ``ndcg``, with ``minus`` ``ndcg-``."""
    return query_mean(ndcg, minus)


def auc_counts(score, label, work=None):
    """(A2, P, N) as Python ints: twice the number of (positive, negative) pairs the score orders correctly (a tie counts
    half), the positives and the negatives."""
    import torch
    _rows(score, label)
    dev = score.device
    n = score.numel()
    if work is None:
        work = _lib.workspace(_lib.lib().otto_obj_auc_workspace_bytes(n), dev)
    out = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.call('otto_obj_auc', dev, score, label, n, out, work, work.numel())
    return tuple(int(v) for v in out.cpu().tolist())


def auc_from_counts(a2, p, n):
    """``A2 / (2 * P * N)``, each integer converted to float64 once; 1.0 when a class is missing (LightGBM)."""
    if p == 0 or n == 0:
        return 1.0
    return float(np.float64(a2) / (2.0 * np.float64(p) * np.float64(n)))


def auc(score, label, work=None):
    return auc_from_counts(*auc_counts(score, label, work))


def logloss_sum(score, label, sigma=1.0, grid=None):
    """The sum over the rows of ``log1p(exp(-y * sigma * score))`` (y = +1 for label > 0, else -1) as a float. ``grid``: the
    number of workgroups (tests; the bits do not depend on it)."""
    import torch
    _rows(score, label)
    dev = score.device
    partials = torch.empty(LOGLOSS_PARTS, dtype=torch.float64, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    if grid is None:
        _lib.call('otto_obj_logloss', dev, score, label, score.numel(), float(sigma), partials, out)
    else:
        _lib.call('otto_obj_logloss_grid', dev, score, label, score.numel(), float(sigma), int(grid), partials, out)
    return float(out.item())


def logloss(score, label, sigma=1.0):
    """The mean binary logloss of raw scores (nan without a row)."""
    n = score.numel()
    return logloss_sum(score, label, sigma) / n if n else float('nan')


def transform(score, sigma=1.0):
    """Raw scores of a binary model -> probabilities ``1 / (1 + exp(-sigma * score))`` (torch, on the score's device)."""
    import torch
    return torch.sigmoid(score * float(sigma))


# ---- the validation metric of a train loop

HIGHER_IS_BETTER = {'map': True, 'ndcg': True, 'auc': True, 'logloss': False}


def evaluate(metric, score, label, query_off, k=MAX_QUERY, minus=None, sigma=1.0):
    """One validation figure. ``metric``: 'map' | 'ndcg' | 'auc' | 'logloss'; ``minus``: None = LightGBM's MAP (queries
    without a positive are left out); False / True = XGBoost's ``map`` / ``map-`` rule, which NDCG always follows."""
    from . import gbdt
    if metric == 'map':
        ap = gbdt.ap_at_k(score, label, query_off, k)
        return gbdt.mean_ap(ap) if minus is None else query_mean(ap, minus)
    if metric == 'ndcg':
        return mean_ndcg(ndcg_at_k(score, label, query_off, k), bool(minus))
    if metric == 'auc':
        return auc(score, label)
    if metric == 'logloss':
        return logloss(score, label, sigma)
    raise ValueError(f'metric {metric!r}: expected map, ndcg, auc or logloss')
