"""NumPy / scalar-Python restatement of SPEC-CBOW and SPEC-DOC2VEC (include/otto_sgns.h): the checker
of otto_sgns_cbow_step. Like tests/sgns_restatement.py: float64 arithmetic on the float32 tables, rounded to float32 at each
stored row. The plan, the keys and the draw are sgns_restatement's; the Huffman tables sgns_hs_restatement's."""
import numpy as np

import sgns_restatement as sr

CBOW, PVDM, DBOW = 0, 1, 2                  # OTTO_SGNS_ARCH_*
SUM, MEAN, FASTTEXT = 0, 1, 2               # OTTO_SGNS_CBOW_*


def negatives(p, cum, seed, epoch, neg, t0, t1, n_aids):
    """int32 [t1 - t0, neg]: negative j of centre c is draw(key(ev, 4, (j << 4) | att)) for the first att in 0..15 whose
    draw differs from the centre's aid, else (aid + 1) % n_aids. A function of the token alone."""
    base = sr.base_key(seed, epoch)
    out = np.zeros((t1 - t0, neg), dtype=np.int32)
    for c in range(t0, t1):
        ev = sr.ev_key(base, int(p['tok_src'][c]))
        a = int(p['tok_aid'][c])
        for j in range(neg):
            pick = (a + 1) % n_aids
            for att in range(16):
                n = sr.draw(cum, sr.key(ev, 4, (j << 4) | att))
                if n != a:
                    pick = n
                    break
            out[c - t0, j] = pick
    return out


def session_of(p, c):
    """the last s with tok_off[s] <= c"""
    return int(np.searchsorted(p['tok_off'], c, side='right')) - 1


def context_aids(p, c):
    return [int(p['tok_aid'][ct]) for ct in sr.context_tokens(p, c)]


def n_inputs(p, c, arch):
    return int(p['pair_off'][c + 1] - p['pair_off'][c]) + (1 if arch == PVDM else 0)


def targets_of(p, hs, c, neg_row):
    """[(table name, row, label)] of centre c in SPEC-CBOW's order: its own path on Syn1, itself on Out, the negatives"""
    a = int(p['tok_aid'][c])
    out = []
    if hs is not None:
        lo, hi = int(hs['path_off'][a]), int(hs['path_off'][a + 1])
        code = int(hs['code'][a])
        out += [('Syn1', int(n), 1.0 - ((code >> j) & 1)) for j, n in enumerate(hs['path_node'][lo:hi])]
    out.append(('Out', a, 1.0))
    out += [('Out', int(t), 0.0) for t in neg_row]
    return out


def count_targets(p, hs, neg, t0, t1, arch):
    """the number of targets the centres [t0, t1) train: a CBOW centre without context trains none"""
    total = 0
    for c in range(t0, t1):
        if arch == CBOW and n_inputs(p, c, arch) == 0:
            continue
        a = int(p['tok_aid'][c])
        total += 1 + neg + (0 if hs is None else int(hs['path_off'][a + 1] - hs['path_off'][a]))
    return total


def _train_targets(tabs, targets, h, lr):
    """SPEC-SGNS's inner loop in place: (grad, loss). Distinct rows are done in one vectorised step (h is fixed over the
    targets, so the rows are independent); a row named twice takes the sequential loop, where it sees its own update."""
    grad, loss = np.zeros_like(h), 0.0
    keys = [(name, t) for name, t, _ in targets]
    if len(set(keys)) == len(keys):
        for name in ('Syn1', 'Out'):
            sel = [(t, lab) for nm, t, lab in targets if nm == name]
            if not sel:
                continue
            ids, label = np.array([t for t, _ in sel], dtype=np.int64), np.array([lab for _, lab in sel])
            o = tabs[name][ids].astype(np.float64)
            x = o @ h
            e = np.exp(-np.abs(x))
            g = lr * (label - np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
            z = np.where(label > 0, -x, x)
            loss += float(np.sum(np.maximum(z, 0.0) + np.log1p(e)))
            grad += g @ o
            tabs[name][ids] = (o + g[:, None] * h[None, :]).astype(np.float32)
        return grad, loss
    for name, t, label in targets:
        o = tabs[name][t].astype(np.float64)
        x = float(h @ o)
        g = lr * (label - sr._sigmoid(x))
        loss += float(sr._softplus(-x if label else x))
        grad += g * o
        tabs[name][t] = (o + g * h).astype(np.float32)
    return grad, loss


def step_sequential(p, cum, tabs, hs, seed, epoch, neg, lr, t0, t1, arch, variant=MEAN):
    """Hogwild without races: centres (DBOW: sessions, and their tokens) in order, in place. tabs: dict of the float32 tables
    In, Out, Syn1 (with hs), Doc (PV-DM, DBOW). Returns the loss sum."""
    n_aids = tabs['Out'].shape[0]
    negs = negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    lr = float(np.float32(lr))
    loss = 0.0
    if arch == DBOW:
        c = t0
        while c < t1:
            s = session_of(p, c)
            hi = min(int(p['tok_off'][s + 1]), t1)
            h = tabs['Doc'][s].astype(np.float64)
            for cc in range(c, hi):
                grad, ls = _train_targets(tabs, targets_of(p, hs, cc, negs[cc - t0]), h, lr)
                loss += ls
                h = h + grad
            tabs['Doc'][s] = h.astype(np.float32)
            c = hi
        return loss
    for c in range(t0, t1):
        ctx = context_aids(p, c)
        n = len(ctx) + (1 if arch == PVDM else 0)
        if n == 0:
            continue
        s = session_of(p, c)
        h = np.zeros(tabs['Out'].shape[1], dtype=np.float64)
        for x in ctx:
            h = h + tabs['In'][x].astype(np.float64)
        if arch == PVDM:
            h = h + tabs['Doc'][s].astype(np.float64)
        if variant != SUM:
            h = h / n
        grad, ls = _train_targets(tabs, targets_of(p, hs, c, negs[c - t0]), h, lr)
        loss += ls
        u = grad / n if variant == MEAN else grad
        for x in ctx:                                               # an aid named m times: m sequential read-modify-writes
            tabs['In'][x] = (tabs['In'][x].astype(np.float64) + u).astype(np.float32)
        if arch == PVDM:
            tabs['Doc'][s] = (tabs['Doc'][s].astype(np.float64) + u).astype(np.float32)
    return loss


def step_batch(p, cum, tabs, hs, seed, epoch, neg, lr, t0, t1, arch, variant=MEAN):
    """Every x and g from the pre-launch tables, contributions summed per row in float64, applied once. Returns the loss."""
    n_aids = tabs['Out'].shape[0]
    negs = negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    lr = float(np.float32(lr))
    pre = {k: v.astype(np.float64) for k, v in tabs.items() if v is not None}
    acc = {k: np.zeros(v.shape, dtype=np.float64) for k, v in pre.items()}
    loss = 0.0

    def train(c, h):
        nonlocal loss
        grad = np.zeros_like(h)
        for name, t, label in targets_of(p, hs, c, negs[c - t0]):
            o = pre[name][t]
            x = float(h @ o)
            g = lr * (label - sr._sigmoid(x))
            loss += float(sr._softplus(-x if label else x))
            grad += g * o
            acc[name][t] += g * h
        return grad

    for c in range(t0, t1):
        s = session_of(p, c)
        if arch == DBOW:
            acc['Doc'][s] += train(c, pre['Doc'][s])
            continue
        ctx = context_aids(p, c)
        n = len(ctx) + (1 if arch == PVDM else 0)
        if n == 0:
            continue
        h = np.zeros(pre['Out'].shape[1], dtype=np.float64)
        for x in ctx:
            h = h + pre['In'][x]
        if arch == PVDM:
            h = h + pre['Doc'][s]
        if variant != SUM:
            h = h / n
        grad = train(c, h)
        u = grad / n if variant == MEAN else grad
        for x in ctx:
            acc['In'][x] += u
        if arch == PVDM:
            acc['Doc'][s] += u
    for k in pre:
        tabs[k][:] = (pre[k] + acc[k]).astype(np.float32)
    return loss


def train_sequential(seed, arch, variant, epochs, vocab_tables, init_tables, init_doc, learning_rate):
    """sgns_inputs.train_sequential for the new archs on the planted sessions (negative sampling alone): the tables dict and
    the per-epoch mean loss per trained target."""
    import sgns_inputs as si
    aid, sess_off, _ = si.planted_sessions()
    _, keep_q, weight = vocab_tables(aid, si.N_AIDS, si.MIN_COUNT, si.T, si.NS_EXPONENT)
    cum = sr.cum_table(weight)
    In, Out = init_tables(si.N_AIDS, si.DIM, seed)
    tabs = dict(In=In, Out=Out)
    if arch != CBOW:
        tabs['Doc'] = init_doc(len(sess_off) - 1, si.DIM, seed)
    losses = []
    for ep in range(epochs):
        p = sr.plan(aid, sess_off, keep_q, seed, ep, si.WS)
        T_ = len(p['tok_aid'])
        loss = 0.0
        for t0 in range(0, T_, si.TOKENS_PER_LAUNCH):
            lr = learning_rate(si.LR, ep * len(aid) + int(p['tok_src'][t0]), epochs * len(aid))
            loss += step_sequential(p, cum, tabs, None, seed, ep, si.NEG, lr, t0, min(t0 + si.TOKENS_PER_LAUNCH, T_), arch, variant)
        losses.append(loss / count_targets(p, None, si.NEG, 0, T_, arch))
    return tabs, losses
