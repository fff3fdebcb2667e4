"""Plain Python / NumPy restatement of SPEC-SGNS-HS (include/otto_sgns.h): the word2vec.c Huffman
tree, the path tables, and the two loops of tests/sgns_restatement.py with the path half in front of every pair's targets.
The checker of otto_sgns_hs_tree and otto_sgns_step_hs."""
import numpy as np

import sgns_restatement as sr


def huffman(count, min_count=1):
    """dict of V, n_inner, path_off int64 [n_aids+1], path_node int32 [sum L], code (a list of Python ints, bit j = the
    bit below path node j, so that paths longer than 64 can still be stated), lens int64 [n_aids], max_len, and
    inner_count (the int counts of the V - 1 inner nodes). Nothing is refused here."""
    count = [int(c) for c in count]
    n_aids = len(count)
    leaves = sorted((a for a in range(n_aids) if count[a] >= max(int(min_count), 1)), key=lambda a: (-count[a], a))
    V = len(leaves)
    paths, codes = [[] for _ in range(n_aids)], [0] * n_aids
    inner_count = []
    if V >= 2:
        sentinel = sum(count) + 1
        cnt = [count[a] for a in leaves] + [sentinel] * (V - 1)
        parent, bit = [-1] * (2 * V - 1), [0] * (2 * V - 1)
        p1, p2 = V - 1, V
        for a in range(V - 1):
            mins = []
            for _ in range(2):
                if p1 >= 0 and cnt[p1] < cnt[p2]:
                    mins.append(p1)
                    p1 -= 1
                else:
                    mins.append(p2)
                    p2 += 1
            cnt[V + a] = cnt[mins[0]] + cnt[mins[1]]
            parent[mins[0]] = parent[mins[1]] = V + a
            bit[mins[1]] = 1
        inner_count = cnt[V:]
        for i, t in enumerate(leaves):
            nodes, bits, n = [], [], i
            while n != 2 * V - 2:
                bits.append(bit[n])
                n = parent[n]
                nodes.append(n - V)
            paths[t] = nodes[::-1]
            codes[t] = sum(b << j for j, b in enumerate(bits[::-1]))
    lens = np.array([len(p) for p in paths], dtype=np.int64)
    return dict(V=V, n_inner=max(V - 1, 1), path_off=np.concatenate(([0], np.cumsum(lens))).astype(np.int64),
                path_node=np.array([n for p in paths for n in p], dtype=np.int32), code=codes, lens=lens,
                max_len=int(lens.max()) if n_aids else 0, inner_count=inner_count)


def _path(hs, ctx):
    lo, hi = int(hs['path_off'][ctx]), int(hs['path_off'][ctx + 1])
    code = int(hs['code'][ctx])
    return [int(n) for n in hs['path_node'][lo:hi]], [1.0 - ((code >> j) & 1) for j in range(hi - lo)]


def step_sequential_hs(p, cum, In, Out, Syn1, hs, seed, epoch, neg, lr, t0, t1, dtype=np.float64):
    """Hogwild without races: centres in order, in place; per pair the path of the context on Syn1, then the 1 + neg
    targets on Out, then h += grad. Returns the loss sum; In / Out / Syn1 (float32) are updated. dtype: as in
    sgns_restatement.step_sequential."""
    n_aids = In.shape[0]
    ctx_all, neg_all = sr.negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
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
            nodes, labels = _path(hs, int(ctx_all[q]))
            targets = [(Syn1, n, lab) for n, lab in zip(nodes, labels)]
            targets += [(Out, int(t), 1.0 if m == 0 else 0.0) for m, t in enumerate([ctx_all[q], *neg_all[q]])]
            for tab, t, label in targets:
                o = tab[t].astype(dtype)
                x = f(h @ o)
                g = lr * (f(label) - sr._sigmoid(x))
                loss += float(sr._softplus(-x if label else x))
                grad += g * o
                tab[t] = (o + g * h).astype(np.float32)
            h = h + grad
            q += 1
        In[ca] = h.astype(np.float32)
    return loss


def step_batch_hs(p, cum, In, Out, Syn1, hs, seed, epoch, neg, lr, t0, t1):
    """Every g from the pre-launch tables, contributions summed per row in float64, applied once to all three tables."""
    n_aids = In.shape[0]
    ctx_all, neg_all = sr.negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    lr = float(np.float32(lr))
    gin, gout, gsyn = (np.zeros(M.shape, dtype=np.float64) for M in (In, Out, Syn1))
    In64, Out64, Syn64 = In.astype(np.float64), Out.astype(np.float64), Syn1.astype(np.float64)
    loss, q = 0.0, 0
    for c in range(t0, t1):
        ca = int(p['tok_aid'][c])
        h = In64[ca]
        for _ in range(int(p['pair_off'][c + 1] - p['pair_off'][c])):
            nodes, labels = _path(hs, int(ctx_all[q]))
            tg = np.concatenate(([ctx_all[q]], neg_all[q])).astype(np.int64)
            for tab, gtab, ids, label in ((Syn64, gsyn, np.array(nodes, dtype=np.int64), np.array(labels)),
                                          (Out64, gout, tg, np.array([1.0] + [0.0] * neg))):
                if len(ids) == 0:
                    continue
                x = tab[ids] @ h
                e = np.exp(-np.abs(x))
                g = lr * (label - np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
                z = np.where(label > 0, -x, x)
                loss += float(np.sum(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))))
                gin[ca] += g @ tab[ids]
                np.add.at(gtab, ids, g[:, None] * h[None, :])
            q += 1
    In[:] = (In64 + gin).astype(np.float32)
    Out[:] = (Out64 + gout).astype(np.float32)
    Syn1[:] = (Syn64 + gsyn).astype(np.float32)
    return loss


def train_sequential_hs(seed, vocab_tables, init_tables, learning_rate):
    """sgns_inputs.train_sequential with the path half: the restatement's hs + ns trainer on the planted sessions."""
    import sgns_inputs as si
    aid, sess_off, _ = si.planted_sessions()
    count, keep_q, weight = vocab_tables(aid, si.N_AIDS, si.MIN_COUNT, si.T, si.NS_EXPONENT)
    hs = huffman(count, si.MIN_COUNT)
    cum = sr.cum_table(weight)
    In, Out = init_tables(si.N_AIDS, si.DIM, seed)
    Syn1 = np.zeros((hs['n_inner'], si.DIM), dtype=np.float32)
    losses = []
    for ep in range(si.EPOCHS):
        p = sr.plan(aid, sess_off, keep_q, seed, ep, si.WS)
        T_ = len(p['tok_aid'])
        loss, path_targets = 0.0, 0
        for t0 in range(0, T_, si.TOKENS_PER_LAUNCH):
            lr = learning_rate(si.LR, ep * len(aid) + int(p['tok_src'][t0]), si.EPOCHS * len(aid))
            loss += step_sequential_hs(p, cum, In, Out, Syn1, hs, seed, ep, si.NEG, lr, t0, min(t0 + si.TOKENS_PER_LAUNCH, T_))
        for c in range(T_):
            path_targets += sum(int(hs['lens'][p['tok_aid'][ct]]) for ct in sr.context_tokens(p, c))
        losses.append(loss / (int(p['pair_off'][-1]) * (1 + si.NEG) + path_targets))
    return In, Out, Syn1, losses
