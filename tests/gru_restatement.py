"""SPEC-GRU4REC (include/otto_gru.h) in NumPy -- TEST INFRASTRUCTURE, NOT PRODUCT. Every function takes ``dtype``: float64 is
the reference the device is judged against, float32 the same arithmetic in the device's precision; the distance between the
two is what tests/golden/gru_bounds.json records. The backward pass is written out by hand (no autograd); tests/test_gru_cpu.py
checks it against torch.nn.GRU + autograd.

Parameters travel as a dict under RecBole's state_dict keys: item_embedding.weight [n_aids + 1, De], gru_layers.weight_ih_l0
[3H, De], gru_layers.weight_hh_l0 [3H, H], dense.weight [De, H], dense.bias [De]."""
import numpy as np

from mf_oracle import MASK, _adam_rows, _coalesced, bpr_negative, mix64

KEYS = ('item_embedding.weight', 'gru_layers.weight_ih_l0', 'gru_layers.weight_hh_l0', 'dense.weight', 'dense.bias')
DENSE = KEYS[1:]
GAMMA = 1e-10


def order_key(seed, epoch, p):
    return mix64(mix64(seed ^ ((epoch * 0xD1342543DE82EF95) & MASK)) ^ ((p * 0xA0761D6478BD642F) & MASK)) >> 1


def check(aid, sess_off, n_aids):
    """(index, kind) of the plan's refusal -- kind 1: offsets, 2: aid -- or (-1, 0)."""
    off = np.asarray(sess_off, dtype=np.int64)
    E, S = len(aid), len(off) - 1
    for i in range(S + 1):
        if (i == 0 and off[0] != 0) or (i < S and off[i] > off[i + 1]) or (i == S and off[S] != E):
            return i, 1
    bad = np.flatnonzero((np.asarray(aid) < 0) | (np.asarray(aid) >= n_aids))
    return (int(bad[0]), 2) if len(bad) else (-1, 0)


def plan(aid, sess_off, n_aids, seed, epoch, max_len):
    """-> (p, seq_lo, seq_len, target, neg), int32 each, in epoch order."""
    rows = []
    for s in range(len(sess_off) - 1):
        lo, hi = int(sess_off[s]), int(sess_off[s + 1])
        for p in range(lo + 1, hi):
            n = min(max_len, p - lo)
            rows.append((order_key(seed, epoch, p), p, p - n, n, int(aid[p])))
    rows.sort()
    out = np.array([r[1:] for r in rows], dtype=np.int64).reshape(-1, 4)
    neg = negatives(seed, epoch, out[:, 0], out[:, 3], n_aids)
    return tuple(out[:, c].astype(np.int32) for c in range(4)) + (neg,)


def negatives(seed, epoch, p, target, n_aids):
    return np.array([bpr_negative(seed, epoch, int(q), int(t), n_aids) for q, t in zip(p, target)], dtype=np.int32)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _rows(aid, seq_lo, seq_len):
    """item rows of the batch's steps, [B, T] left-aligned, 0 (PAD) behind a sequence's end"""
    B, T = len(seq_lo), int(max(seq_len, default=0))
    rows = np.zeros((B, T), dtype=np.int64)
    for b, (lo, n) in enumerate(zip(seq_lo, seq_len)):
        rows[b, :n] = np.asarray(aid[lo:lo + n], dtype=np.int64) + 1
    return rows


def _forward(P, rows, seq_len, dtype):
    """the batch's recurrence -> (h_T [B, H], the steps' (rows, active, h_prev, r, z, n, hn)); a finished sequence keeps its h"""
    E, Wi, Wh = (P[k].astype(dtype) for k in KEYS[:3])
    H = Wh.shape[1]
    h = np.zeros((rows.shape[0], H), dtype=dtype)
    n_steps = np.asarray(seq_len)
    steps = []
    for t in range(rows.shape[1]):
        act = (n_steps > t)[:, None]
        gi, gh = E[rows[:, t]] @ Wi.T, h @ Wh.T
        r = _sigmoid(gi[:, :H] + gh[:, :H])
        z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        nn = np.tanh(gi[:, 2 * H:] + r * hn)
        steps.append((rows[:, t], act, h, r, z, nn, hn))
        h = np.where(act, (1 - z) * nn + z * h, h).astype(dtype)
    return h, steps


def encode(P, aid, seq_lo, seq_len, dtype=np.float64):
    """o [B, De] = dense(h_T) of every sequence"""
    h, _ = _forward(P, _rows(aid, seq_lo, seq_len), seq_len, dtype)
    return (h @ P[KEYS[3]].astype(dtype).T + P[KEYS[4]].astype(dtype)).astype(dtype)


def grad(P, aid, seq_lo, seq_len, target, neg, dtype=np.float64):
    """-> (grads: dict under KEYS, the item gradient dense [n_aids + 1, De]; loss_sum; o). Gradients of the batch MEAN."""
    E, Wi, Wh, Wd, bd = (P[k].astype(dtype) for k in KEYS)
    H, B = Wh.shape[1], len(seq_lo)
    G = {k: np.zeros(P[k].shape, dtype=dtype) for k in KEYS}
    gE = G[KEYS[0]]
    one, gamma = dtype(1), dtype(GAMMA)
    h, steps = _forward(P, _rows(aid, seq_lo, seq_len), seq_len, dtype)
    o = (h @ Wd.T + bd).astype(dtype)
    pr, nr = np.asarray(target, dtype=np.int64) + 1, np.asarray(neg, dtype=np.int64) + 1
    diff = E[pr] - E[nr]
    sg = _sigmoid((o * diff).sum(axis=1, dtype=dtype))
    loss_sum = (-np.log(gamma + sg)).sum(dtype=dtype)
    c = (-(sg * (one - sg)) / (gamma + sg) / dtype(max(B, 1)))[:, None]
    do = c * diff
    np.add.at(gE, pr, c * o)
    np.add.at(gE, nr, -(c * o))
    G[KEYS[3]] += do.T @ h
    G[KEYS[4]] += do.sum(axis=0, dtype=dtype)
    dh = do @ Wd
    for rows_t, act, hp, r, z, nn, hn in reversed(steps):
        dn, dz = dh * (one - z), dh * (hp - nn)
        dan = dn * (one - nn * nn)
        daz = dz * z * (one - z)
        dar = dan * hn * r * (one - r)
        gi = np.where(act, np.concatenate([dar, daz, dan], axis=1), 0).astype(dtype)
        gh = np.where(act, np.concatenate([dar, daz, dan * r], axis=1), 0).astype(dtype)
        G[KEYS[1]] += gi.T @ E[rows_t]
        G[KEYS[2]] += gh.T @ hp
        np.add.at(gE, rows_t[act[:, 0]], (gi @ Wi)[act[:, 0]])
        dh = np.where(act, dh * z + gh @ Wh, dh).astype(dtype)
    return G, loss_sum, o


def export_list(gE, aid, seq_lo, seq_len, target, neg):
    """the rows a batch touches, ascending: what the device's list must name"""
    rows = [np.asarray(target) + 1, np.asarray(neg) + 1]
    rows += [np.asarray(aid[lo:lo + n]) + 1 for lo, n in zip(seq_lo, seq_len)]
    ids = np.unique(np.concatenate(rows)).astype(np.int32) if len(seq_lo) else np.zeros(0, dtype=np.int32)
    return ids, gE[ids]


def new_state(P, dtype=np.float64):
    """parameters in ``dtype`` with zeroed Adam moments: {'p': ..., 'm': ..., 'v': ...}"""
    return {'p': {k: P[k].astype(dtype).copy() for k in KEYS}, 'm': {k: np.zeros(P[k].shape, dtype=dtype) for k in KEYS},
            'v': {k: np.zeros(P[k].shape, dtype=dtype) for k in KEYS}}


def adam_dense(p, m, v, g, lr, betas, eps, t, dtype):
    """torch.optim.Adam (no amsgrad, no weight decay), in place: scalars in double on the host, cast to the tensors' type"""
    b1, b2 = betas
    step_size = dtype(lr / (1 - b1 ** t))
    bc2_sqrt = dtype(np.sqrt(1 - b2 ** t))
    m += (g - m) * dtype(1 - b1)
    v *= dtype(b2)
    v += (dtype(1 - b2) * g) * g
    p += -step_size * (m / (np.sqrt(v) / bc2_sqrt + dtype(eps)))


def adam_rows(E, m, v, ids, rows, lr, betas, eps, t, dtype):
    """Adam on the listed rows: _adam_rows of oracle/mf_oracle.py in float32, the same arithmetic in float64"""
    if dtype == np.float32:
        return _adam_rows(E, m, v, ids, rows, lr, betas, eps, t)
    b1, b2 = betas
    mu = (rows - m[ids]) * (1 - b1)
    vu = (rows * rows - v[ids]) * (1 - b2)
    m[ids] += mu
    v[ids] += vu
    E[ids] += -(lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)) * (m[ids] / (np.sqrt(v[ids]) + eps))


def apply(state, dense_grads, ids, rows, lr, betas, eps, t, dtype=np.float64):
    """SPEC UPDATE in place. ``dense_grads``: the four dense gradients under DENSE; ``ids`` / ``rows``: the item list."""
    for k in DENSE:
        adam_dense(state['p'][k], state['m'][k], state['v'][k], dense_grads[k].astype(dtype), lr, betas, eps, t, dtype)
    ids = np.asarray(ids, dtype=np.int64)
    keep = ids > 0
    adam_rows(state['p'][KEYS[0]], state['m'][KEYS[0]], state['v'][KEYS[0]], ids[keep], rows[keep].astype(dtype), lr, betas, eps, t, dtype)


def train(P, aid, sess_off, n_aids, batch, lr, betas, eps, seed, epoch, max_len, steps=None, dtype=np.float64, t0=0, state=None):
    """One epoch (or its first ``steps`` batches) -> (state, losses). ``state``: carried from the epoch before, with t0 = the
    steps taken so far; None: a fresh one from ``P``."""
    state = new_state(P, dtype) if state is None else state
    p, lo, n, tgt, neg = plan(aid, sess_off, n_aids, seed, epoch, max_len)
    losses = []
    n_batches = -(-len(p) // batch)
    for q in range(n_batches if steps is None else min(steps, n_batches)):
        sl = slice(q * batch, (q + 1) * batch)
        G, loss_sum, _ = grad(state['p'], aid, lo[sl], n[sl], tgt[sl], neg[sl], dtype)
        ids, rows = export_list(G[KEYS[0]], aid, lo[sl], n[sl], tgt[sl], neg[sl])
        apply(state, G, ids, rows, lr, betas, eps, t0 + q + 1, dtype)
        losses.append(float(loss_sum) / len(lo[sl]))
    return state, losses


def coalesce(n_rows, De, ids, rows):
    """``_coalesced`` of oracle/mf_oracle.py under this module's name"""
    return _coalesced(n_rows, De, ids, rows)
