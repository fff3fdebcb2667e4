"""Exact nearest-neighbour tables over aid embeddings on the device (SPEC-KNN): thin Python over
``include/otto_knn.h``.

The reference takes its neighbour lists from an Annoy index over fastText vectors, queried once per session
(``src/covisitation/inference.py:58-69,166,223``, ``src/ranker/regular_candidate_generation.py:58-70,157,338``,
``src/ranker/fasttext_candidate_generator.py:75-98``). Here the table is an exact k-NN over the embeddings this package
trains, built once; it closes the chain *train item embeddings -> neighbour table -> candidate recipes*. The lists are
not expected to reproduce those of an approximate index over other vectors.
"""
from .. import _lib

METRICS = {'euclidean': 0, 'angular': 1, 'dot': 2}
MAX_K = 64
DIMS = (8, 16, 32, 64, 128)
# state_dict keys of the item tables this package trains: CollaborativeFiltering, MatrixFactorization
# (torch_modules.py), the BPR model (bpr.py)
ITEM_TABLE_KEYS = ('embeddings.weight', 'aid_embeddings.weight', 'item_embedding.weight')


def neighbour_table(E, k=45, metric='euclidean', valid=None, rows=None):
    """The ``k`` nearest neighbours of every query aid under ``metric`` ('euclidean', 'angular', 'dot').

    ``E`` float32 [N, d] on the device, d in {8, 16, 32, 64, 128}; ``valid`` uint8 / bool [N] (0 = the aid has no
    vector: nobody's neighbour, its own row empty); ``rows`` int32 [R] = the query aids (default: all N, in order).
    Returns device tensors (ids int32 [R, k] (-1 padded), dist float32 [R, k] (+inf padded), n int32 [R]);
    ``(ids, None, n)`` or the tuple itself is what ``candidate_lookup`` takes as ``matrices['neighbours']``."""
    import torch
    if not isinstance(E, torch.Tensor) or E.dim() != 2:
        raise ValueError('E: expected a float32 tensor [N, d]')
    if E.dtype != torch.float32 or not E.is_contiguous():
        raise ValueError(f'E: expected contiguous float32, got {E.dtype}')
    N, d = int(E.shape[0]), int(E.shape[1])
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    if d not in DIMS:
        raise ValueError(f'd must be one of {DIMS} (got {d})')
    if metric not in METRICS:
        raise ValueError(f'metric must be one of {tuple(METRICS)} (got {metric!r})')
    if N < 1:
        raise ValueError('E has no rows')
    dev = E.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        if valid.dtype != torch.uint8 or valid.shape != (N,) or not valid.is_contiguous() or valid.device != dev:
            raise ValueError('valid: expected contiguous uint8 [N] on the device of E')
    if rows is not None:
        if rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.device != dev or rows.numel() < 1:
            raise ValueError('rows: expected non-empty contiguous int32 [R] on the device of E')
    if dev.type != 'cuda':
        raise _lib.OttoError('neighbour_table needs a ROCm device (no CPU fallback)')
    R = N if rows is None else int(rows.numel())
    ws_bytes = int(_lib.lib().otto_knn_workspace(R, N, d, k, METRICS[metric]))
    ws = _lib.workspace(ws_bytes, dev)
    ids = torch.empty((R, k), dtype=torch.int32, device=dev)
    dist = torch.empty((R, k), dtype=torch.float32, device=dev)
    n = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call('otto_knn_table', dev, E, N, d, valid, rows, R, k, METRICS[metric], ids, dist, n, ws, ws_bytes)
    return ids, dist, n


def item_table(model_or_state_dict):
    """The item (aid) embedding table of one of this package's models or of a checkpoint's ``state_dict``:
    ``embeddings.weight`` (CollaborativeFiltering), ``aid_embeddings.weight`` (MatrixFactorization) or
    ``item_embedding.weight`` (BPR)."""
    sd = model_or_state_dict if isinstance(model_or_state_dict, dict) else model_or_state_dict.state_dict()
    found = [key for key in ITEM_TABLE_KEYS if key in sd]
    if len(found) != 1:
        raise ValueError(f'expected exactly one of {ITEM_TABLE_KEYS} in the state dict, found {found or sorted(sd)}')
    return sd[found[0]]


def neighbour_table_from_model(model_or_state_dict, k=45, metric='euclidean', valid=None, rows=None, device=None):
    """:func:`neighbour_table` over the item table of a model / a checkpoint written by ``torch_trainer.py``
    (``torch.load(path, weights_only=True)`` goes straight in). ``device``: where to put a table loaded on the host."""
    import torch
    E = item_table(model_or_state_dict).detach()
    if device is not None:
        E = E.to(torch.device(device))
    return neighbour_table(E.to(torch.float32).contiguous(), k=k, metric=metric, valid=valid, rows=rows)


def split_rows(n_aids, rank, world, rows=None):
    """The query aids of ``rank`` out of ``world``: a contiguous, balanced slice of ``rows`` (default ``0..n_aids-1``) as
    an int32 tensor. Every rank builds the lists of its slice from its own copy of E; no communication, and the
    concatenation of the ranks' outputs in rank order is the single-GPU table."""
    import torch
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f'rank {rank} outside world {world}')
    total = int(n_aids) if rows is None else int(rows.numel())
    lo, hi = total * rank // world, total * (rank + 1) // world
    if rows is None:
        return torch.arange(lo, hi, dtype=torch.int32)
    return rows[lo:hi].contiguous()


def neighbour_candidates(aid, sess_off, table, n_candidates=20, labels=None, session_ids=None):
    """The fourth candidate generator (``src/ranker/fasttext_candidate_generator.py:75-98``): per session the first
    ``n_candidates`` neighbours of the LAST event's aid, scored with their distances; the session's own aids stay in.

    ``table`` = ``(ids, dist, n)`` of :func:`neighbour_table` over all aids; ``labels`` = the CSR pair ``(label_off
    int64 [S+1], label_aid int32)`` that ``ranker_table`` takes (None: test mode, no label column); ``session_ids``
    int64 [S] = the values of the ``session`` column (None: the session's index). Returns a dict of tensors on the
    table's device -- ``session`` int64, ``candidates`` int32, ``candidate_scores`` float32, ``candidate_labels`` uint8
    (or None), one row per (session, candidate), and ``row_off`` int64 [S+1]. A session without events, or whose last
    aid has an empty row, yields no rows. A row gather: torch indexing, no kernel."""
    import torch
    ids, dist, n = table
    dev = ids.device
    if dist is None:
        raise ValueError('table: the distances are the candidate scores; pass (ids, dist, n)')
    if ids.dim() != 2 or dist.shape != ids.shape or n.shape != (ids.shape[0],):
        raise ValueError('table: expected (ids [N, k], dist [N, k], n [N])')
    if sess_off.dtype != torch.int64 or sess_off.numel() < 1:
        raise ValueError('sess_off: expected int64 [S+1]')
    if not 1 <= int(n_candidates) <= ids.shape[1]:
        raise ValueError(f'n_candidates must be in [1, {ids.shape[1]}] (the width of the table)')
    S = sess_off.numel() - 1
    if session_ids is not None and (session_ids.dtype != torch.int64 or session_ids.numel() != S):
        raise ValueError('session_ids: expected int64 [S]')
    aid, sess_off = aid.to(dev), sess_off.to(dev)
    length = sess_off[1:] - sess_off[:-1]
    last = aid[(sess_off[1:] - 1).clamp(min=0)].to(torch.int64) if aid.numel() else torch.zeros(S, dtype=torch.int64, device=dev)
    if S and bool(((last < 0) | (last >= ids.shape[0]))[length > 0].any()):
        raise ValueError('a session ends on an aid outside the table')
    last = last.clamp(0, ids.shape[0] - 1)
    m = torch.where(length > 0, n[last].to(torch.int64).clamp(max=int(n_candidates)), torch.zeros_like(length))
    row_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    row_off[1:] = torch.cumsum(m, 0)
    sess = torch.repeat_interleave(torch.arange(S, dtype=torch.int64, device=dev), m)
    slot = torch.arange(sess.numel(), dtype=torch.int64, device=dev) - row_off[sess]
    cand = ids[last[sess], slot]
    out = {'session': sess if session_ids is None else session_ids.to(dev)[sess], 'candidates': cand,
           'candidate_scores': dist[last[sess], slot], 'candidate_labels': None, 'row_off': row_off}
    if labels is not None:
        l_off, l_aid = labels
        if l_off.dtype != torch.int64 or l_aid.dtype != torch.int32 or l_off.numel() != S + 1:
            raise ValueError('labels: expected (int64 [S+1], int32) CSR lists')
        l_off, l_aid = l_off.to(dev), l_aid.to(dev)
        l_sess = torch.repeat_interleave(torch.arange(S, dtype=torch.int64, device=dev), l_off[1:] - l_off[:-1])
        keys = torch.sort((l_sess << 32) | l_aid.to(torch.int64)).values
        want = (sess << 32) | cand.to(torch.int64)
        pos = torch.searchsorted(keys, want).clamp(max=max(keys.numel() - 1, 0))
        hit = keys[pos] == want if keys.numel() else torch.zeros_like(want, dtype=torch.bool)
        out['candidate_labels'] = hit.to(torch.uint8)
    return out


def neighbour_candidates_frame(aid, sess_off, table, n_candidates=20, labels=None, session_ids=None):
    """:func:`neighbour_candidates` as the frame ``fasttext_candidate_generator.py:118-136`` pickles: columns ``session``,
    ``candidates`` (uint64), ``candidate_scores`` (float32) and, with ``labels``, ``candidate_labels`` (uint8)."""
    import numpy as np
    import pandas as pd
    out = neighbour_candidates(aid, sess_off, table, n_candidates=n_candidates, labels=labels, session_ids=session_ids)
    cols = {'session': out['session'].cpu().numpy(), 'candidates': out['candidates'].cpu().numpy().astype(np.uint64),
            'candidate_scores': out['candidate_scores'].cpu().numpy().astype(np.float32)}
    if out['candidate_labels'] is not None:
        cols['candidate_labels'] = out['candidate_labels'].cpu().numpy().astype(np.uint8)
    return pd.DataFrame(cols)
