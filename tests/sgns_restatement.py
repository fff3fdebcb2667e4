"""NumPy / scalar-Python restatement of SPEC-SGNS (include/otto_sgns.h): the checker of the device
code. One centre at a time, float64 arithmetic on the float32 tables, rounded to float32 at each stored row."""
import numpy as np

M64 = (1 << 64) - 1
C_EPOCH, C_EVENT, C_KEY = 0xD1342543DE82EF95, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def base_key(seed, epoch):
    return mix64(seed ^ ((epoch * C_EPOCH) & M64))


def ev_key(base, e):
    return mix64(base ^ ((e * C_EVENT) & M64))


def key(ev, stream, w):
    return mix64(ev ^ ((((stream << 20) | w) * C_KEY) & M64))


def key_neg(ev, k, j, att):
    return key(ev, 3, (k << 10) | (j << 4) | att)


def cum_table(weight):
    return np.cumsum(np.asarray(weight, dtype=np.uint64), dtype=np.uint64)


def draw(cum, k):
    """upper_bound(cum, mulhi64(key, total))"""
    total = int(cum[-1])
    u = (k * total) >> 64
    return int(np.searchsorted(cum, np.uint64(u), side='right'))


def keep_flags(aid, keep_q, seed, epoch, event0=0):
    base = base_key(seed, epoch)
    out = np.zeros(len(aid), dtype=bool)
    for e, a in enumerate(aid):
        q = int(keep_q[a])
        out[e] = q != 0 and (key(ev_key(base, event0 + e), 1, 0) >> 32) <= q
    return out


def plan(aid, sess_off, keep_q, seed, epoch, ws, event0=0):
    """dict of tok_aid int32, tok_src int64, tok_off int64 [S+1], radius uint8, tok_left uint8, pair_off int64 [T+1]"""
    keep = keep_flags(aid, keep_q, seed, epoch, event0)
    base = base_key(seed, epoch)
    tok_aid, tok_src, radius, left, npairs, tok_off = [], [], [], [], [], [0]
    for s in range(len(sess_off) - 1):
        ev = [e for e in range(int(sess_off[s]), int(sess_off[s + 1])) if keep[e]]
        n = len(ev)
        for i, e in enumerate(ev):
            r = 1 + (((key(ev_key(base, event0 + e), 2, 0) >> 32) * ws) >> 32)
            lf, rt = min(r, i), min(r, n - 1 - i)
            tok_aid.append(int(aid[e])); tok_src.append(event0 + e); radius.append(r); left.append(lf); npairs.append(lf + rt)
        tok_off.append(len(tok_aid))
    return dict(tok_aid=np.array(tok_aid, dtype=np.int32), tok_src=np.array(tok_src, dtype=np.int64),
                tok_off=np.array(tok_off, dtype=np.int64), radius=np.array(radius, dtype=np.uint8),
                tok_left=np.array(left, dtype=np.uint8),
                pair_off=np.concatenate(([0], np.cumsum(np.array(npairs, dtype=np.int64)))).astype(np.int64))


def context_tokens(p, c):
    lf = int(p['tok_left'][c])
    n = int(p['pair_off'][c + 1] - p['pair_off'][c])
    return [c - lf + k if k < lf else c + 1 + (k - lf) for k in range(n)]


def negatives(p, cum, seed, epoch, neg, t0, t1, n_aids):
    """(ctx int32 [pairs], negs int32 [pairs, neg]) of the centres [t0, t1): the sampler alone. A function of the plan and
    the token, never of how the epoch is cut into launches."""
    base = base_key(seed, epoch)
    ctx_out, neg_out = [], []
    for c in range(t0, t1):
        ev = ev_key(base, int(p['tok_src'][c]))
        for k, ct in enumerate(context_tokens(p, c)):
            ctx = int(p['tok_aid'][ct])
            row = []
            for j in range(neg):
                pick = None
                for att in range(16):
                    n = draw(cum, key_neg(ev, k, j, att))
                    if n != ctx:
                        pick = n
                        break
                row.append((ctx + 1) % n_aids if pick is None else pick)
            ctx_out.append(ctx)
            neg_out.append(row)
    return np.array(ctx_out, dtype=np.int32), np.array(neg_out, dtype=np.int32).reshape(len(ctx_out), neg)


def _sigmoid(x):
    one = type(x)(1)                    # the arithmetic stays in the type of x (a Python float, np.float64 or np.float32)
    return one / (one + np.exp(-x)) if x >= 0 else np.exp(x) / (one + np.exp(x))


def _softplus(z):
    return max(z, type(z)(0)) + np.log1p(np.exp(-abs(z)))


def step_sequential(p, cum, In, Out, seed, epoch, neg, lr, t0, t1, dtype=np.float64):
    """Hogwild without races: centres in order, in place. Returns the loss sum; In / Out (float32) are updated.
    dtype: the type of h, o, x, g and grad (np.float32 states what a float32 run of this loop gives: the noise floor of
    tests/test_sgns_hogwild_cpu.py); the loss is summed in float64 either way."""
    n_aids = In.shape[0]
    ctx_all, neg_all = negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    f = float if np.dtype(dtype) == np.float64 else np.dtype(dtype).type
    lr = f(np.float32(lr))
    loss, q = 0.0, 0
    for c in range(t0, t1):
        ca = int(p['tok_aid'][c])
        npair = int(p['pair_off'][c + 1] - p['pair_off'][c])
        if npair == 0:
            continue
        h = In[ca].astype(dtype)
        for _ in range(npair):
            grad = np.zeros_like(h)
            for m, t in enumerate([int(ctx_all[q])] + [int(x) for x in neg_all[q]]):
                o = Out[t].astype(dtype)
                x = f(h @ o)
                label = f(1.0 if m == 0 else 0.0)
                g = lr * (label - _sigmoid(x))
                loss += float(_softplus(-x if m == 0 else x))
                grad += g * o
                Out[t] = (o + g * h).astype(np.float32)
            h = h + grad
            q += 1
        In[ca] = h.astype(np.float32)
    return loss


def step_batch(p, cum, In, Out, seed, epoch, neg, lr, t0, t1):
    """Every g from the pre-launch tables, contributions summed per row in float64, applied once."""
    n_aids = In.shape[0]
    ctx_all, neg_all = negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    lr = float(np.float32(lr))
    gin, gout = np.zeros(In.shape, dtype=np.float64), np.zeros(Out.shape, dtype=np.float64)
    In64, Out64 = In.astype(np.float64), Out.astype(np.float64)
    loss, q = 0.0, 0
    for c in range(t0, t1):
        ca = int(p['tok_aid'][c])
        h = In64[ca]
        for _ in range(int(p['pair_off'][c + 1] - p['pair_off'][c])):
            tg = np.concatenate(([ctx_all[q]], neg_all[q])).astype(np.int64)
            x = Out64[tg] @ h
            label = np.zeros(len(tg)); label[0] = 1.0
            sg = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
            g = lr * (label - sg)
            z = np.where(label > 0, -x, x)
            loss += float(np.sum(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))))
            gin[ca] += g @ Out64[tg]
            np.add.at(gout, tg, g[:, None] * h[None, :])
            q += 1
    In[:] = (In64 + gin).astype(np.float32)
    Out[:] = (Out64 + gout).astype(np.float32)
    return loss
