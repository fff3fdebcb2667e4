"""Validation split, ground-truth labels and recall@20 on the device (SPEC-EVAL): thin Python over
``include/otto_eval.h``.

What this replaces in the reference: ``src/validation.py`` (the cutoff per last-week session, :71-85, and ``get_labels``,
:9-52) and the recall loops of ``src/ranker/inference.py:176-180, 248-250, 317-322``, ``src/ranker/lgb_trainer.py:190-197``
and ``src/ranker/covisitation_candidate_generation.py:159-164``. Events are a :class:`otto_amd.events.DeviceEvents`; label
lists are CSR pairs ``(off int64 [S+1], aid int32)``, the form ``candidates.ranker_table(labels=...)`` takes. Predictions
are padded (``[P, k]`` int32, or ``([P, k], n int32 [P])``: what ``session_topk`` / ``predictions`` emit) or CSR
(``(off int64 [P+1], aid int32)``: a ranker table's ``row_off`` / ``candidates``). No CPU fallback.

Labels on the organisers' split come from ``DATA/splits/val_labels.parquet``: :func:`read_labels` decodes the file on the
device and :func:`assemble_labels` (SPEC-LABELS, ``include/otto_labels.h``) aligns its rows to a session list, in place of
the ``map`` + three ``merge(how='left')`` + ``fillna`` of ``src/covisitation/inference.py:118-123`` and
``src/ranker/lgb_trainer.py:54-75``.
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


# ---- val_labels.parquet -> label lists (SPEC-LABELS, include/otto_labels.h) ------------------------------------------------------
TYPE_CODES = {'clicks': 0, 'carts': 1, 'orders': 2}
LABEL_REASONS = {1: 'a session outside int32', 2: 'a type code above 2', 3: 'list offsets that descend or leave the values',
                 4: 'the same (session, type) as an earlier row', 5: 'a value outside [0, n_aids)'}


def assemble_labels(session, type, off, value, null, label_session, n_aids, work=None):
    """SPEC-LABELS: the rows ``session int64 [R], type uint8 [R], off int64 [R+1], value int64 [V], null uint8 [R]`` of a label
    file (what ``parquet.read_columns`` / ``read_string_codes`` / ``read_lists`` return) -> ``({'clicks': (off int64 [S+1],
    aid int32), 'carts': ..., 'orders': ...}, n_dropped)`` aligned to ``label_session`` (int32 [S], ascending and distinct).
    The list of (session, type) is the values of its one row, in file order, repeated aids kept; no row, a null list and an
    empty list are an empty list. A row whose session is not in ``label_session`` is dropped and counted. ``OttoError``
    naming the smallest offending row for a type code above 2, a second row of one (session, type), a value outside
    ``[0, n_aids)`` or a session outside int32. ``work``: a uint8 scratch tensor to use instead of a fresh one."""
    import numpy as np
    import torch
    dev = session.device if isinstance(session, torch.Tensor) else None
    if dev is None or dev.type != 'cuda':
        raise _lib.OttoError('evaluate.assemble_labels needs tensors on a ROCm device (no CPU fallback)')
    R = int(session.numel())
    _lib.need(session, 'session', torch.int64, 1, device=dev)
    _lib.need(type, 'type', torch.uint8, 1, device=dev, numel=R)
    _lib.need(off, 'off', torch.int64, 1, device=dev, numel=R + 1)
    _lib.need(value, 'value', torch.int64, 1, device=dev)
    _lib.need(null, 'null', torch.uint8, 1, device=dev, numel=R)
    _lib.need(label_session, 'label_session', torch.int32, 1, device=dev)
    S, V, n_aids = int(label_session.numel()), int(value.numel()), int(n_aids)
    if not 0 <= n_aids < 1 << 31:
        raise ValueError(f'n_aids must be in [0, 2^31) (got {n_aids})')
    with torch.cuda.device(dev):
        offs = [torch.empty(S + 1, dtype=torch.int64, device=dev) for _ in TYPES]
        job = _lib.LabelsJob(_lib.ptr(session, dev), _lib.ptr(type, dev), _lib.ptr(off, dev), _lib.ptr(value, dev), _lib.ptr(null, dev), R, V,
                             _lib.ptr(label_session, dev), S, n_aids, (C.c_void_p * 3)(*[o.data_ptr() for o in offs]), (C.c_void_p * 3)(),
                             None, 0, _lib.stream(dev))
        need = int(_lib.lib().otto_labels_workspace(C.byref(job)))
        if need < 0:
            _lib.check(need, 'otto_labels_workspace')
        if work is None:
            work = _lib.workspace(need, dev)
        elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
            raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
        job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
        counts, err = np.zeros(4, dtype=np.int64), np.full(2, -1, dtype=np.int64)
        try:
            _lib.call('otto_labels_count', dev, C.byref(job), counts, err, stream=False)
        except _lib.OttoError:
            if err[0] < 0:
                raise
            raise _lib.OttoError(f'assemble_labels: row {int(err[0])}: {LABEL_REASONS.get(int(err[1]), "?")}') from None
        aids = [torch.empty(max(int(n), 1), dtype=torch.int32, device=dev) for n in counts[:3]]
        job.d_out_aid = (C.c_void_p * 3)(*[a.data_ptr() for a in aids])
        _lib.call('otto_labels_fill', dev, C.byref(job), stream=False)
    return {name: (offs[t], aids[t][:int(counts[t])]) for t, name in enumerate(TYPES)}, int(counts[3])


def read_labels(path, device, session=None, n_aids=None):
    """``DATA/splits/val_labels.parquet`` (columns ``session``, ``type``: 'clicks' / 'carts' / 'orders', ``ground_truth``: a list
    of aids) -> ``(label_session int32 [S], {'clicks': (off, aid), 'carts': ..., 'orders': ...}, n_dropped)``, decoded and
    assembled on the device: ``parquet.read_columns``, ``parquet.read_string_codes``, ``parquet.read_lists``, then
    :func:`assemble_labels`. ``session``: the session list to align to (int32, ascending and distinct; rows of other sessions
    are dropped and counted); None: the file's distinct sessions, ascending. ``n_aids``: the bound every label must stay
    below; None: the file's largest aid + 1. The lists go into :func:`hits`, :func:`evaluate`,
    ``candidates.ranker_table(labels=...)`` and ``cross_validate(truth=...)`` as they are."""
    import torch
    from .. import parquet
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.OttoError('evaluate.read_labels needs a ROCm device (no CPU fallback)')
    sess, = parquet.read_columns(path, ['session'], dev, dtypes={'session': torch.int64})
    typ = parquet.read_string_codes(path, 'type', TYPE_CODES, dev, dtype=torch.uint8)
    off, value, null = parquet.read_lists(path, 'ground_truth', dev, dtype=torch.int64)
    if not (sess.numel() == typ.numel() == null.numel()):
        raise _lib.OttoError(f'{path}: the columns differ in length ({sess.numel()}, {typ.numel()}, {null.numel()} rows)')
    if session is None:
        if sess.numel() and (int(sess.min()) < -2 ** 31 or int(sess.max()) >= 2 ** 31):
            raise _lib.OttoError(f'{path}: a session outside int32')
        session = torch.unique(sess).to(torch.int32)
    else:
        session = _tensor(session, 'session', torch.int32)
    if n_aids is None:
        n_aids = int(value.max()) + 1 if value.numel() else 0
        if not 0 <= n_aids < 1 << 31:
            raise _lib.OttoError(f'{path}: a label outside [0, 2^31)')
    labels, dropped = assemble_labels(sess, typ, off, value, null, session, n_aids)
    return session, labels, dropped
