"""Validation split, ground-truth labels and recall@20 on the device (SPEC-EVAL): thin Python over
``include/otto_eval.h``.

What this replaces in the reference: ``src/validation.py`` (the cutoff per last-week session, :71-85, and ``get_labels``,
:9-52) and the recall loops of ``src/ranker/inference.py:176-180, 248-250, 317-322``, ``src/ranker/lgb_trainer.py:190-197``
and ``src/ranker/covisitation_candidate_generation.py:159-164``. Events are a :class:`otto_amd.events.DeviceEvents`; label
lists are CSR pairs ``(off int64 [S+1], aid int32)``, the form ``candidates.ranker_table(labels=...)`` takes. Predictions
are padded (``[P, k]`` int32, or ``([P, k], n int32 [P])``: what ``session_topk`` / ``predictions`` emit) or CSR
(``(off int64 [P+1], aid int32)``: a ranker table's ``row_off`` / ``candidates``). No CPU fallback.
"""
import ctypes as C
import functools
import math

from .. import _lib
from ..events import DeviceEvents
from ..metrics import weighted_recall
from .forest import MAX_K

TYPES = ('clicks', 'carts', 'orders')
# the 1-d device tensor every argument here is; a strided one is copied, not refused
_tensor = functools.partial(_lib.need, dim=1, copy=True)


def _events(events):
    import torch
    if not isinstance(events, DeviceEvents):
        raise ValueError('events: expected a DeviceEvents')
    aid, ts = _tensor(events.aid, 'events.aid', torch.int32), _tensor(events.ts, 'events.ts', torch.int32)
    typ, off = _tensor(events.type, 'events.type', torch.uint8), _tensor(events.sess_off, 'events.sess_off', torch.int64)
    if off.numel() < 1 or not (aid.numel() == ts.numel() == typ.numel()):
        raise ValueError('events: columns differ in length or sess_off is empty')
    return aid, ts, typ, off


def last_click(events):
    """int32 [S]: the in-session index of every session's last click, -1 without one."""
    import torch
    _, _, typ, off = _events(events)
    S = off.numel() - 1
    out = torch.empty(S, dtype=torch.int32, device=typ.device)
    _lib.call('otto_eval_last_click', typ.device, typ, off, S, out)
    return out


def cutoffs(events, seed):
    """(cutoff int32 [S], n_without_click): 0 for a session of two events or with no click after index 0, else a keyed
    hash of (seed, session position) mapped uniformly to [0, last_click). ``n_without_click`` counts the sessions the
    reference's ``np.where(...)[0][-1]`` would raise for (no click, length != 2); their cutoff is 0."""
    import torch
    _, _, typ, off = _events(events)
    S = off.numel() - 1
    out = torch.empty(S, dtype=torch.int32, device=typ.device)
    n_wo = C.c_int64(0)
    _lib.call('otto_eval_cutoffs', typ.device, typ, off, S, int(seed) & (2 ** 64 - 1), out, C.byref(n_wo))
    return out, int(n_wo.value)


def split(events, cutoff):
    """Cut every session after event ``cutoff[s]``: (the kept events as a ``DeviceEvents``, {'clicks': (off, aid), 'carts':
    ..., 'orders': ...}). The labels are over the events after the cutoff: the first click, the distinct cart aids and
    the distinct order aids, both ascending. Raises ``OttoError`` for a cutoff outside ``[0, max(n, 1))`` or an event
    type outside 0..2."""
    import torch
    aid, ts, typ, off = _events(events)
    dev = aid.device
    S, E = off.numel() - 1, aid.numel()
    cutoff = _tensor(cutoff, 'cutoff', torch.int32)
    if cutoff.numel() != S or cutoff.device != dev:
        raise ValueError('cutoff: expected int32 [S] on the events\' device')
    ws = _lib.workspace(_lib.lib().otto_eval_split_workspace(S, E), dev)
    offs = [torch.empty(S + 1, dtype=torch.int64, device=dev) for _ in range(4)]
    counts = (C.c_int64 * 4)()
    _lib.call('otto_eval_split_count', dev, aid, typ, off, S, E, cutoff, *offs, counts, ws, ws.numel())
    kept, n_lab = int(counts[0]), [int(c) for c in counts[1:]]
    k_aid = torch.empty(kept, dtype=torch.int32, device=dev)
    k_ts = torch.empty(kept, dtype=torch.int32, device=dev)
    k_typ = torch.empty(kept, dtype=torch.uint8, device=dev)
    labs = [torch.empty(n, dtype=torch.int32, device=dev) for n in n_lab]
    _lib.call('otto_eval_split', dev, aid, ts, typ, off, S, E, cutoff, *offs, k_aid, k_ts, k_typ, *labs, ws, ws.numel())
    kept_events = DeviceEvents(k_aid, k_ts, k_typ, offs[0], events.session_ids, None, events.n_aids)
    return kept_events, {name: (offs[1 + i], labs[i]) for i, name in enumerate(TYPES)}


def _ratio(h, d):
    return h / d if d else math.nan


def hits(labels, preds, label_session=None, pred_session=None, cap=20, mask=None):
    """Per label session ``|distinct(row[:cap]) & distinct(labels)|`` and ``min(len(labels), 20)``.

    ``labels``: ``(off int64 [S+1], aid int32)``. ``preds``: ``[P, k]`` int32 (k <= 64, negative entries are padding),
    ``([P, k], n int32 [P])``, or ``(off int64 [P+1], aid int32)``. ``label_session`` / ``pred_session``: int32 ids,
    ascending and distinct (None: the position); without ``pred_session`` the rows are position-aligned. ``cap``: only
    the first ``cap`` entries of a row count (None or <= 0: all). ``mask``: uint8 / bool [S], the holdout subset.
    Returns (hits int32 [S], denom int32 [S], totals) with ``totals = {'hits', 'denom', 'mask_hits', 'mask_denom'}``
    (Python ints). Raises ``OttoError`` for a prediction session that is no label session."""
    import torch
    l_off, l_aid = labels
    l_off, l_aid = _tensor(l_off, 'label off', torch.int64), _tensor(l_aid, 'label aid', torch.int32)
    dev = l_off.device
    S = l_off.numel() - 1
    p_n = p_off = None
    if isinstance(preds, (tuple, list)):
        first, second = preds
        if isinstance(first, torch.Tensor) and first.dim() == 2:
            p_aid, p_n = _tensor(first, 'pred aid', torch.int32, dim=2), _tensor(second, 'pred n', torch.int32)
        else:
            p_off, p_aid = _tensor(first, 'pred off', torch.int64), _tensor(second, 'pred aid', torch.int32)
    else:
        p_aid = _tensor(preds, 'pred aid', torch.int32, dim=2)
    if p_off is not None:
        P, k = p_off.numel() - 1, 0
    else:
        P, k = int(p_aid.shape[0]), int(p_aid.shape[1])
        if not 1 <= k <= MAX_K:
            raise ValueError(f'padded predictions: k must be in [1, {MAX_K}] (got {k}); longer rows go in as CSR')
        if p_n is not None and p_n.numel() != P:
            raise ValueError('pred n: expected int32 [P]')
    if S < 0 or P < 0:
        raise ValueError('labels / preds: an offset array needs at least one entry')
    if label_session is not None:
        label_session = _tensor(label_session, 'label_session', torch.int32)
        if label_session.numel() != S:
            raise ValueError('label_session: expected int32 [S]')
    if pred_session is not None:
        pred_session = _tensor(pred_session, 'pred_session', torch.int32)
        if pred_session.numel() != P:
            raise ValueError('pred_session: expected int32 [P]')
    elif P != S:
        raise ValueError(f'without pred_session the rows are position-aligned: {P} rows for {S} label sessions')
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        mask = _tensor(mask, 'mask', torch.uint8)
        if mask.numel() != S:
            raise ValueError('mask: expected uint8 [S]')
    for t in (l_aid, p_aid, p_n, p_off, label_session, pred_session, mask):
        if t is not None and t.device != dev:
            raise ValueError('all tensors must be on one device')
    out_h = torch.empty(S, dtype=torch.int32, device=dev)
    out_d = torch.empty(S, dtype=torch.int32, device=dev)
    tot = (C.c_int64 * 4)()
    ws = _lib.workspace(_lib.lib().otto_eval_hits_workspace(S), dev)
    _lib.call('otto_eval_hits', dev, label_session, l_off, l_aid, S, p_aid, p_n, p_off, k, P, pred_session, int(cap) if cap else 0,
              mask, out_h, out_d, tot, ws, ws.numel())
    return out_h, out_d, {'hits': int(tot[0]), 'denom': int(tot[1]), 'mask_hits': int(tot[2]), 'mask_denom': int(tot[3])}


def recall_at_20(labels, preds, label_session=None, pred_session=None, mask=None):
    """``metrics.recall_at_20`` on the device: sum of hits over sum of ``min(len(labels), 20)``, the first 20 entries of
    every row counted; NaN without a label. With ``mask``: (recall over all, recall over the masked sessions)."""
    _, _, t = hits(labels, preds, label_session, pred_session, cap=20, mask=mask)
    r = _ratio(t['hits'], t['denom'])
    return r if mask is None else (r, _ratio(t['mask_hits'], t['mask_denom']))


def evaluate(top20_by_type, labels_by_type, pred_session=None, holdout=None, label_session=None):
    """Recall of every type and the weighted recall (``inference.py:176-180, 248-250, 317-322``): ``top20_by_type`` and
    ``labels_by_type`` are dicts over 'clicks', 'carts', 'orders' of predictions and label lists as :func:`hits` takes
    them; ``pred_session``: one id tensor for all types or a dict per type; ``holdout``: uint8 / bool [S]
    (``holdout_sessions``). Returns {'clicks', 'carts', 'orders', 'weighted'}, plus 'holdout': the same four over the
    masked sessions, when ``holdout`` is given."""
    out, held = {}, {}
    for name in TYPES:
        ps = pred_session.get(name) if isinstance(pred_session, dict) else pred_session
        _, _, t = hits(labels_by_type[name], top20_by_type[name], label_session, ps, cap=20, mask=holdout)
        out[name] = _ratio(t['hits'], t['denom'])
        held[name] = _ratio(t['mask_hits'], t['mask_denom'])
    out['weighted'] = weighted_recall(out['clicks'], out['carts'], out['orders'])
    if holdout is not None:
        held['weighted'] = weighted_recall(held['clicks'], held['carts'], held['orders'])
        out['holdout'] = held
    return out
