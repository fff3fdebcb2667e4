"""NumPy restatement of SPEC-DOC2VEC-INFER (include/otto_sgns.h): the checker of otto_sgns_infer.
Float32 arithmetic throughout, as the device does it (`dtype=np.float64` states what the same loop gives in float64: the noise
floor of the long-chain test). The keys, the draw and the sigmoid are sgns_restatement's, the Huffman tables
sgns_hs_restatement's, the arch and variant numbers sgns_cbow_restatement's. Nothing is written to the model."""
import numpy as np

import sgns_cbow_restatement as cr
import sgns_hs_restatement as hr          # noqa: F401  (the `hs` argument below is hr.huffman's dict)
import sgns_restatement as sr

MAX_PASSES = 64                           # OTTO_SGNS_MAX_INFER_PASSES
INIT_STREAM = 5
U32 = 2**32 - 1


def keep_table(keep_q):
    """the plan's keep table at inference: 2^32 - 1 where the training corpus kept the aid at all, 0 elsewhere"""
    return np.where(np.asarray(keep_q) != 0, U32, 0).astype(np.uint32)


def tokens(aid, sess_off, keep_q):
    """(tok_aid int32 [T], tok_off int64 [S+1]): the events with keep_q[aid] != 0, in order; nothing is sub-sampled"""
    aid = np.asarray(aid)
    kept = np.asarray(keep_q)[aid] != 0
    pos = np.concatenate(([0], np.cumsum(kept))).astype(np.int64)
    return aid[kept].astype(np.int32), pos[np.asarray(sess_off)]


def rates(alpha, min_alpha, passes):
    return np.array([alpha - (alpha - min_alpha) * p / max(passes - 1, 1) for p in range(passes)], dtype=np.float64).astype(np.float32)


def session_base(seed, p, key):
    """sb(p, s) = sg_ev(sg_base(seed, p), sess_key[s])"""
    return sr.ev_key(sr.base_key(seed, p), int(key))


def init_row(seed, key, d):
    """float32 [d]: ((float)(2r + 1) * 2^-24 - 0.5f) * (2.0f / d), r the top 23 bits of key(sb(0, s), 5, j)"""
    sb0 = session_base(seed, 0, key)
    r = np.array([sr.key(sb0, INIT_STREAM, j) >> 41 for j in range(d)], dtype=np.int64)
    v = (2 * r + 1).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)
    return v * (np.float32(2.0) / np.float32(d))


def radius(ev, ws):
    return 1 + (((sr.key(ev, 2, 0) >> 32) * ws) >> 32)


def negatives(cum, ev, neg, a, n_aids):
    """SPEC-CBOW's negatives of the token with event key ev and aid a (stream 4)"""
    out = []
    for j in range(neg):
        pick = (a + 1) % n_aids
        for att in range(16):
            n = sr.draw(cum, sr.key(ev, 4, (j << 4) | att))
            if n != a:
                pick = n
                break
        out.append(pick)
    return out


def _targets(model, hs, a, negs):
    """(rows float32 [n, d], labels float32 [n]) in SPEC-CBOW's order: the path of a on Syn1, a on Out, the negatives"""
    rows, labels = [], []
    if hs is not None:
        lo, hi = int(hs['path_off'][a]), int(hs['path_off'][a + 1])
        code = int(hs['code'][a])
        for j, n in enumerate(hs['path_node'][lo:hi]):
            rows.append(model['Syn1'][int(n)])
            labels.append(1.0 - ((code >> j) & 1))
    rows.append(model['Out'][a])
    labels.append(1.0)
    for t in negs:
        rows.append(model['Out'][int(t)])
        labels.append(0.0)
    return np.array(rows), np.array(labels)


def token_grad(rows, labels, h, lr, dtype=np.float32):
    """(grad [d], loss): x = <h, row>, g = lr * (label - sigmoid(x)), grad += g * row, target by target in order. h is fixed
    over the targets and no row is written, so the targets are independent; the accumulation order is still the list's."""
    f = np.dtype(dtype).type
    grad, loss = np.zeros(len(h), dtype=dtype), 0.0
    lr = f(lr)
    for o, label in zip(rows.astype(dtype), labels):
        x = f(np.sum(h * o, dtype=dtype))
        g = lr * (f(label) - sr._sigmoid(x))
        loss += float(sr._softplus(-x if label else x))
        grad = grad + g * o
    return grad, loss


def pvdm_hidden(model, ctx, h_doc, variant, dtype=np.float32):
    """(h, n): the float32 sum of In[x_k] in order, then the doc row last; the mean variants divide by (float)n"""
    h = np.zeros(len(h_doc), dtype=dtype)
    for x in ctx:
        h = h + model['In'][x].astype(dtype)
    h = h + h_doc
    n = len(ctx) + 1
    if variant != cr.SUM:
        h = h / np.dtype(dtype).type(n)
    return h, n


def infer(tok_aid, tok_off, model, cum, hs, seed, neg, ws, arch, variant, lr, sess_key=None, dtype=np.float32, rows=None):
    """SPEC-DOC2VEC-INFER over the sessions `rows` (default: all). model: dict of the float32 tables In (PV-DM), Out, Syn1
    (with hs); lr: float32 [P]. Returns dict(Doc float32 [S, d], loss float64 [S, 2], negs int32 [P, T, neg], radius uint8
    [P, T]); rows that were not asked for stay zero."""
    assert arch in (cr.PVDM, cr.DBOW)
    n_aids, d = model['Out'].shape
    S, T, P = len(tok_off) - 1, len(tok_aid), len(lr)
    f = np.dtype(dtype).type
    Doc, loss = np.zeros((S, d), dtype=np.float32), np.zeros((S, 2), dtype=np.float64)
    negs, rad = np.zeros((P, T, max(neg, 0)), dtype=np.int32), np.zeros((P, T), dtype=np.uint8)
    for s in (range(S) if rows is None else rows):
        key = s if sess_key is None else int(sess_key[s])
        lo, hi = int(tok_off[s]), int(tok_off[s + 1])
        h_doc = init_row(seed, key, d).astype(dtype)
        for p in range(P):
            sb, ls = session_base(seed, p, key), 0.0
            for c in range(lo, hi):
                a = int(tok_aid[c])
                ev = sr.ev_key(sb, c - lo)
                ng = negatives(cum, ev, neg, a, n_aids)
                negs[p, c] = ng
                tr, labels = _targets(model, hs, a, ng)
                if arch == cr.DBOW:
                    grad, l1 = token_grad(tr, labels, h_doc, lr[p], dtype)
                    h_doc = h_doc + grad
                else:
                    r = radius(ev, ws)
                    rad[p, c] = r
                    ctx = [int(tok_aid[x]) for x in list(range(max(lo, c - r), c)) + list(range(c + 1, min(hi, c + r + 1)))]
                    h, n = pvdm_hidden(model, ctx, h_doc, variant, dtype)
                    grad, l1 = token_grad(tr, labels, h, lr[p], dtype)
                    h_doc = h_doc + (grad / f(n) if variant == cr.MEAN else grad)
                ls += l1
            if p == 0:
                loss[s, 0] = ls
            if p == P - 1:
                loss[s, 1] = ls
        Doc[s] = h_doc.astype(np.float32)
    return dict(Doc=Doc, loss=loss, negs=negs, radius=rad)
