"""Covisitation candidate lookup on the device: the per-session loop of the reference's
``src/ranker/covisitation_candidate_generation.py:108-157`` over the builder's resident top-k arrays."""
import ctypes as C

from .. import _lib

SOURCES = {'U': 0, 'CC': 1, 'CO': 2, 'LAST': 3, 'C': 4}
# recipes of covisitation_candidate_generation.py:127,133,138
CLICK_RECIPE = (('time_weighted', 'U'), ('click_weighted', 'CC'), ('cart_weighted', 'CC'), ('click_cart', 'CC'), ('cart_order', 'CC'))
CART_RECIPE = (('time_weighted', 'U'), ('cart_weighted', 'CC'), ('cart_order', 'CC'))
ORDER_RECIPE = CART_RECIPE
# recipes of the standalone model (src/covisitation/inference.py:227,231,235; regular_candidate_generation.py:162-176 with
# n_common = 100): the same lists + the nearest neighbours of the session's last aid. 'neighbours' is one more matrix the
# caller supplies: (int32 [n_aids, 45], int32 [n_aids]) -- the reference takes them from fastText vectors + Annoy (:223-224)
INFERENCE_CLICK_RECIPE = CLICK_RECIPE + (('neighbours', 'LAST'),)
INFERENCE_CART_RECIPE = CART_RECIPE + (('neighbours', 'LAST'),)
INFERENCE_ORDER_RECIPE = INFERENCE_CART_RECIPE


def _events(who, aid, typ, sess_off):
    """The device of the event arrays ``aid`` int32 / ``typ`` uint8 / ``sess_off`` int64, checked."""
    import torch
    dev = aid.device
    if dev.type != 'cuda':
        raise _lib.OttoError(f'{who} needs a ROCm device (no CPU fallback)')
    for name, x, dt in (('aid', aid, torch.int32), ('type', typ, torch.uint8), ('sess_off', sess_off, torch.int64)):
        _lib.need(x, name, dt, device=dev)
    return dev


def candidate_lookup(aid, typ, sess_off, matrices, recipe, n_common=100, self_counts=False):
    """``matrices``: {kind: (aid_y int32 [n_aids,k], W, n int32 [n_aids])} as returned by ``CovisBuilder.finalize``.
    Returns (cand int32 [S, n_common] (-1 padded), count int32 [S, n_common], n int32 [S]) on the device.
    ``self_counts``: the session's own aids leave the selection BEFORE most_common and their Counter counts come back as a
    fourth tensor int32 [E] (one value per event; ``otto_cand_lookup_self``, used by :func:`recency_predictions`)."""
    import torch
    dev = _events('candidate_lookup', aid, typ, sess_off)
    kinds = []
    for kind, _ in recipe:
        if kind not in kinds:
            kinds.append(kind)
    p = _lib.CandParams()
    y0 = matrices[kinds[0]][0]
    widths = [int(matrices[kd][0].shape[1]) for kd in kinds]
    p.n_aids, p.n_matrices = int(y0.shape[0]), len(kinds)
    p.k = min(max(set(widths), key=widths.count), 32)          # the common row length; other matrices carry their own (mat_k)
    keep = []
    for i, kind in enumerate(kinds):
        y, n = matrices[kind][0], matrices[kind][-1]
        if y.dtype != torch.int32 or n.dtype != torch.int32 or not y.is_contiguous() or not n.is_contiguous() or y.shape[0] != y0.shape[0]:
            raise ValueError(f'matrix {kind}: expected contiguous int32 [n_aids, k] / [n_aids]')
        keep.append((y, n))
        p.d_mat_y[i], p.d_mat_n[i] = _lib.ptr(y, dev, f'matrix {kind}'), _lib.ptr(n, dev, f'matrix {kind}')
        p.mat_k[i] = 0 if widths[i] == p.k else widths[i]
    p.n_terms = len(recipe)
    for t, (kind, src) in enumerate(recipe):
        p.term_matrix[t], p.term_source[t] = kinds.index(kind), SOURCES[src]
    p.n_common = int(n_common)
    S = sess_off.numel() - 1
    cand = torch.empty((S, n_common), dtype=torch.int32, device=dev)
    count = torch.empty((S, n_common), dtype=torch.int32, device=dev)
    n_out = torch.empty(S, dtype=torch.int32, device=dev)
    if self_counts:
        own = torch.zeros(max(aid.numel(), 1), dtype=torch.int32, device=dev)
        _lib.call('otto_cand_lookup_self', dev, C.byref(p), aid, typ, sess_off, S, cand, count, n_out, own)
        return cand, count, n_out, own[:aid.numel()]
    _lib.call('otto_cand_lookup', dev, C.byref(p), aid, typ, sess_off, S, cand, count, n_out)
    return cand, count, n_out


def predictions(aid, sess_off, cand, n_cand, most_frequent, n_pred=20):
    """Final predictions of the standalone model (``src/covisitation/inference.py:236-241``): the session's unique aids
    (most recent first) + the candidates + the global most frequent aids of the type (``data/aid_frequencies/*.json``), cut
    at ``n_pred``. ``cand`` / ``n_cand``: output of :func:`candidate_lookup` with ``n_common <= 64``. Returns (pred int32
    [S, n_pred] (-1 padded), n int32 [S])."""
    import torch
    dev = aid.device
    if dev.type != 'cuda':
        raise _lib.OttoError('predictions needs a ROCm device (no CPU fallback)')
    S = sess_off.numel() - 1
    freq = torch.as_tensor(list(most_frequent), dtype=torch.int32, device=dev).contiguous()
    pred = torch.empty((S, n_pred), dtype=torch.int32, device=dev)
    n_out = torch.empty(S, dtype=torch.int32, device=dev)
    _lib.call('otto_cand_predictions', dev, aid, sess_off, S, cand, n_cand, int(cand.shape[1]), freq if freq.numel() else None,
              int(freq.numel()), int(n_pred), pred, n_out)
    return pred, n_out


def ranker_table(aid, sess_off, cand, count, n_cand, labels=None, session_ids=None):
    """The ranker's candidate table (``src/ranker/regular_candidate_generation.py:160-193,236-244``) from the outputs of
    :func:`candidate_lookup` (``INFERENCE_*_RECIPE``, ``n_common=100``), on the device: per session the unique aids, most
    recent first, scored ``u, u-1, .., 1``, then the candidates scored with their Counter counts; ``labels`` = CSR pair
    ``(label_off int64 [S+1], label_aid int32)`` of the type's ground truth (None: no label column, test mode);
    ``session_ids`` int64 [S] = the values of the ``session`` column (None: the session's index).
    Returns a dict of device tensors ``session`` int64, ``candidates`` int32, ``candidate_scores`` float32,
    ``candidate_labels`` uint8 (or None) -- one row per (session, candidate) -- and ``row_off`` int64 [S+1]; this is the
    frame ``ranker.interaction_feature_engineering.interaction_features_rows`` takes."""
    import torch
    dev = aid.device
    if dev.type != 'cuda':
        raise _lib.OttoError('ranker_table needs a ROCm device (no CPU fallback)')
    for name, x, dt in (('aid', aid, torch.int32), ('sess_off', sess_off, torch.int64), ('cand', cand, torch.int32),
                        ('count', count, torch.int32), ('n_cand', n_cand, torch.int32)):
        _lib.need(x, name, dt, device=dev)
    S, n_common = sess_off.numel() - 1, int(cand.shape[1])
    if cand.shape != count.shape or cand.shape[0] != S or n_cand.numel() != S:
        raise ValueError('cand / count / n_cand shapes disagree with sess_off')
    l_off, l_aid = (None, None) if labels is None else labels
    if labels is not None:
        _lib.need(l_off, 'labels: the offsets of the (int64 [S+1], int32) CSR lists', torch.int64, device=dev, numel=S + 1)
        _lib.need(l_aid, 'labels: the aids of the (int64 [S+1], int32) CSR lists', torch.int32, device=dev)
    if session_ids is not None:
        _lib.need(session_ids, 'session_ids', torch.int64, device=dev, numel=S)
    p = lambda t: t if t is not None and t.numel() else None        # an empty array goes in as NULL
    ws_b = int(_lib.lib().otto_cand_ranker_workspace(S))
    ws = _lib.workspace(ws_b, dev)
    row_off = torch.empty(S + 1, dtype=torch.int64, device=dev)
    n_rows = C.c_int64()
    _lib.call('otto_cand_ranker_rows', dev, p(aid), p(sess_off), S, p(n_cand), n_common, row_off, C.byref(n_rows), ws, ws_b)
    R = int(n_rows.value)
    out = {'session': torch.empty(R, dtype=torch.int64, device=dev), 'candidates': torch.empty(R, dtype=torch.int32, device=dev),
           'candidate_scores': torch.empty(R, dtype=torch.float32, device=dev),
           'candidate_labels': torch.empty(R, dtype=torch.uint8, device=dev) if labels is not None else None, 'row_off': row_off}
    _lib.call('otto_cand_ranker_table', dev, p(aid), p(sess_off), S, p(cand), p(count), p(n_cand), n_common, row_off, p(l_off), p(l_aid),
              p(session_ids), p(out['session']), p(out['candidates']), p(out['candidate_scores']), p(out['candidate_labels']))
    return out


# curves and type coefficients of src/ranker/recency_weighted_candidate_generator.py:24,68-70
RECENCY_CURVES = ((0.1, 1.0), (0.5, 1.0))            # clicks; carts and orders
RECENCY_TYPE_COEFFICIENT = (1.0, 6.0, 1.0)


def recency_candidates(aid, typ, sess_off, curves=RECENCY_CURVES, type_coef=RECENCY_TYPE_COEFFICIENT):
    """Recency-weighted candidates of every session (the loop of
    ``src/ranker/recency_weighted_candidate_generator.py:61-93``).  Returns (cand int32 [n_curves, E], weight float64
    [n_curves, E], n int32 [S]): session s owns ``[sess_off[s], sess_off[s] + n[s])`` of every curve's row, in
    ``Counter.most_common`` order."""
    import torch
    dev = _events('recency_candidates', aid, typ, sess_off)
    p = _lib.RecencyParams()
    p.n_curves = len(curves)
    for c, (a0, a1) in enumerate(curves):
        p.start[c], p.stop[c] = float(a0), float(a1)
    for t in range(3):
        p.type_coef[t] = float(type_coef[t])
    S, E = sess_off.numel() - 1, aid.numel()
    cand = torch.full((len(curves), E), -1, dtype=torch.int32, device=dev)
    w = torch.zeros((len(curves), E), dtype=torch.float64, device=dev)
    n_out = torch.zeros(S, dtype=torch.int32, device=dev)
    _lib.call('otto_recency_candidates', dev, C.byref(p), aid, typ, sess_off, S, E, cand, w, n_out)
    return cand, w, n_out


# the recency branch of the standalone model (src/covisitation/inference.py:143-199): per target the recency curve, the bump of
# a neighbour / list entry, the list matrix and the source aids whose lists are concatenated; type coefficients of :72
INFERENCE_RECENCY_TARGETS = (
    {'curve': (0.1, 1.0), 'bump': 0.05, 'matrix': 'time_weighted', 'source': 'C'},      # clicks  (:152,168,174-179)
    {'curve': (0.5, 1.0), 'bump': 0.05, 'matrix': 'cart_weighted', 'source': 'CC'},     # carts   (:153,169,182-187)
    {'curve': (0.5, 1.0), 'bump': 0.15, 'matrix': 'cart_order', 'source': 'CO'},        # orders  (:154,170,190-195)
)
INFERENCE_TYPE_COEFFICIENT = (1.0, 9.0, 6.0)


def recency_predictions(aid, typ, sess_off, matrices, targets=INFERENCE_RECENCY_TARGETS, type_coef=INFERENCE_TYPE_COEFFICIENT,
                        neighbours='neighbours', min_unique=20, n_pred=20, n_common=None):
    """Predictions of the sessions the reference routes to its recency branch (at least ``min_unique`` unique aids,
    ``src/covisitation/inference.py:128-131,143-199``): recency-weighted Counter of the session's aids, + bump for the
    nearest neighbours of the last aid (``matrices[neighbours]``; None: no neighbour term) and for every entry of the
    target's concatenated top lists, ``most_common(n_pred)``. Returns (pred int32 [T, S, n_pred] (-1 padded), weight float64
    [T, S, n_pred], n int32 [T, S]; n = -1 for sessions with fewer unique aids, which the covisitation branch predicts)."""
    import torch
    dev = aid.device
    if dev.type != 'cuda':
        raise _lib.OttoError('recency_predictions needs a ROCm device (no CPU fallback)')
    if not 1 <= len(targets) <= 3:
        raise ValueError('1 to 3 targets')
    n_common = int(n_common or n_pred)
    S = sess_off.numel() - 1
    p = _lib.RecencyPredParams()
    p.n_targets, p.n_common, p.n_pred, p.min_unique = len(targets), n_common, int(n_pred), int(min_unique)
    for i in range(3):
        p.type_coef[i] = float(type_coef[i])
    keep = []
    for t, tg in enumerate(targets):
        recipe = ((neighbours, 'LAST'),) if neighbours is not None else ()
        recipe = recipe + ((tg['matrix'], tg['source']),)
        cand, count, n_c, own = candidate_lookup(aid, typ, sess_off, matrices, recipe, n_common=n_common, self_counts=True)
        keep.append((cand, count, n_c, own))
        p.start[t], p.stop[t], p.bump[t] = float(tg['curve'][0]), float(tg['curve'][1]), float(tg['bump'])
        p.d_cand[t], p.d_count[t], p.d_n_cand[t], p.d_self_count[t] = (_lib.ptr(x, dev, f'target {t}') for x in (cand, count, n_c, own))
    T = len(targets)
    pred = torch.empty((T, S, n_pred), dtype=torch.int32, device=dev)
    weight = torch.empty((T, S, n_pred), dtype=torch.float64, device=dev)
    n_out = torch.empty((T, S), dtype=torch.int32, device=dev)
    _lib.call('otto_recency_predictions', dev, C.byref(p), aid, typ, sess_off, S, pred, weight, n_out)
    return pred, weight, n_out
