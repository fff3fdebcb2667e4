"""Robust scaling and outer-join blend of several model families' scores on the device (SPEC-BLEND, DESIGN.md
section 3d): thin Python over ``include/otto_blend.h``.

What this replaces in the reference: ``src/ranker/inference.py`` -- ``RobustScaler().fit_transform`` on every family's
score column (``read_predictions``, :14-55), the left / outer / outer join on (session, aid) with nulls filled by 0
(:160-163, :227-231, :297-301), the weighted sum and "sort by (session, predictions desc), head(20)" (:167-176).

A model is a tuple ``(session, aid, score)`` of 1-d device tensors of one length: session and aid int32 (int64 is
narrowed after a range check on the device), score float64 or float32. A float32 score column is widened to float64
before scaling -- a stated departure: scikit-learn would compute the statistics in float32. No CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .forest import MAX_K, session_topk

MAX_MODELS = 8           # OTTO_BLEND_MAX_MODELS
_TINY = 10 * np.finfo(np.float64).eps


def _column(t, what):
    """``t`` as a contiguous 1-d device tensor, of whatever dtype."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{what}: expected a 1-d tensor')
    return _lib.need(t, what, t.dtype, 1, copy=True)


def center_scale(nv, stats):
    """center and scale from the count of non-NaN values and the six order statistics of ``otto_blend_robust_stats``
    (SPEC-BLEND: integer ranks, NumPy's linear interpolation, float64 throughout)."""
    s = [np.float64(v) for v in stats]
    nv = int(nv)
    center = s[1] if nv & 1 else (s[0] + s[1]) / np.float64(2.0)

    def lerp(a, b, t):
        if b == a:
            return a
        if t >= 0.5:
            return b - (b - a) * (np.float64(1.0) - t)
        return a + (b - a) * t

    q25 = lerp(s[2], s[3], np.float64(((nv - 1) & 3) / 4.0))
    q75 = lerp(s[4], s[5], np.float64(((3 * (nv - 1)) & 3) / 4.0))
    scale = q75 - q25
    if scale < _TINY:
        scale = np.float64(1.0)
    return float(center), float(scale)


def robust_stats(score):
    """(nv, stats float64 [6]) of a float64 device column: the number of non-NaN values and v[(nv-1)>>1], v[nv>>1], the
    two neighbours of the 25th and of the 75th percentile. Raises ``OttoError`` for an empty or all-NaN column or an
    infinite value."""
    import torch
    _lib.need(score, 'score', torch.float64, 1)
    n = score.numel()
    ws_bytes = int(_lib.lib().otto_blend_select_workspace(n))
    nv = C.c_int64(0)
    stats = (C.c_double * 6)()
    ws = _lib.workspace(ws_bytes, score.device)
    _lib.call('otto_blend_robust_stats', score.device, score, n, C.byref(nv), stats, ws, ws_bytes)
    return int(nv.value), np.array(list(stats), dtype=np.float64)


def robust_scale(score):
    """``RobustScaler().fit_transform`` of one score column, cast to float32: (scaled float32 tensor, center, scale).
    NaN entries are ignored by the statistics and stay NaN."""
    import torch
    score = _column(score, 'score')
    if score.dtype == torch.float32:
        score = score.double()
    nv, stats = robust_stats(score)
    center, scale = center_scale(nv, stats)
    out = torch.empty(score.numel(), dtype=torch.float32, device=score.device)
    _lib.call('otto_blend_scale', score.device, score, score.numel(), center, scale, out)
    return out, center, scale


def _ids(t, what):
    import torch
    t = _column(t, what)
    if t.dtype == torch.int64:
        if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 31)):
            raise ValueError(f'{what}: values outside int32')
        t = t.to(torch.int32)
    if t.dtype != torch.int32:
        raise ValueError(f'{what}: expected an int32 (or int64) tensor')
    return t


def _prepare(models, weights, left_of_base, scale):
    import torch
    models = list(models)
    M = len(models)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f'models: expected 1 to {MAX_MODELS} (session, aid, score) tuples')
    weights = [float(w) for w in weights]
    if len(weights) != M:
        raise ValueError(f'weights: {len(weights)} for {M} models')
    left = [0] * M if left_of_base is None else [int(bool(f)) for f in left_of_base]
    if len(left) != M or left[0]:
        raise ValueError('left_of_base: one flag per model, and model 0 (the base) cannot be flagged')
    cols = []
    for m, (session, aid, score) in enumerate(models):
        session, aid = _ids(session, f'session of model {m}'), _ids(aid, f'aid of model {m}')
        score = _column(score, f'score of model {m}')
        if not (session.numel() == aid.numel() == score.numel()):
            raise ValueError(f'model {m}: session, aid and score differ in length')
        if session.device != score.device or aid.device != score.device or score.device != models[0][2].device:
            raise ValueError('all columns of all models must be on one device')
        if scale and score.numel():
            score = robust_scale(score)[0]
        elif score.dtype != torch.float32:
            score = score.to(torch.float32)
        cols.append((session, aid, score.contiguous()))
    return cols, weights, left


def blend_predictions(models, weights, left_of_base=None, scale=True, _want64=False):
    """Join the models on (session, aid) -- model 0 and every un-flagged model outer, a ``left_of_base`` model only where
    model 0 has the key, absent scores 0 -- and weight them: ``p = ((s_0 w_0 + s_1 w_1) + s_2 w_2) + ...`` in float32,
    each product and sum rounded on its own. ``scale=True`` robust-scales every model's score column first. Returns
    (session_id int32 [S], row_off int64 [S+1], aid int32 [R], pred float32 [R]) on the device, rows in ascending
    (session, aid) order. Raises ``OttoError`` for a negative id or a (session, aid) twice in one model."""
    import torch
    cols, weights, left = _prepare(models, weights, left_of_base, scale)
    M = len(cols)
    dev = cols[0][2].device
    ns = [c[0].numel() for c in cols]
    tot = sum(ns)
    if tot >= 1 << 31:
        raise ValueError('more than 2^31 - 1 rows in all')
    # one pointer per model and column (_prepare made the columns contiguous on dev); an empty column goes in as NULL
    arr = lambda i: (C.c_void_p * M)(*[_lib.ptr(c[i], dev, f'model {m}') if c[i].numel() else None for m, c in enumerate(cols)])
    ws_bytes = int(_lib.lib().otto_blend_join_workspace(tot, M))
    ws = _lib.workspace(ws_bytes, dev)
    sid = torch.empty(tot, dtype=torch.int32, device=dev)
    off = torch.empty(tot + 1, dtype=torch.int64, device=dev)
    aid = torch.empty(tot, dtype=torch.int32, device=dev)
    pred = torch.empty(tot, dtype=torch.float32, device=dev)
    pred64 = torch.empty(tot, dtype=torch.float64, device=dev) if _want64 else None
    n_out, n_sess = C.c_int64(0), C.c_int64(0)
    _lib.call('otto_blend_join', dev, M, arr(0), arr(1), arr(2), (C.c_int64 * M)(*ns), (C.c_double * M)(*weights),
              (C.c_int32 * M)(*left), sid, off, aid, pred, pred64, C.byref(n_out), C.byref(n_sess), ws, ws_bytes)
    R, S = int(n_out.value), int(n_sess.value)
    out = (sid[:S], off[:S + 1], aid[:R], pred[:R])
    return out + (pred64[:R],) if _want64 else out


def blend_topk(models, weights, left_of_base=None, k=20, scale=True):
    """:func:`blend_predictions`, then per session the first ``k`` aids by (prediction descending, aid ascending), NaN
    last: (session_id int32 [S], top_aid int32 [S, k] (-1 padded), n int32 [S])."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    sid, off, aid, _, pred64 = blend_predictions(models, weights, left_of_base, scale, _want64=True)
    top_aid, _, n = session_topk(pred64.contiguous(), aid.contiguous(), off.contiguous(), k=k)
    return sid, top_aid, n
