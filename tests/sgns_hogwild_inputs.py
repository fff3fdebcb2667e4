"""Inputs of the hogwild skip-gram step tests (tests/test_sgns_hogwild_cpu.py, tests/test_sgns_hogwild_gpu.py; DESIGN.md
section 3i), the launch cutter, and three deliberately wrong restatements.

The hogwild step is deterministic when a launch holds one centre, or when the centres of a launch share no row. Three launch
shapes use that, each compared with tests/sgns_restatement.py's sequential loop run over the same cut:
  A  one centre per launch: any input (tiny_vocab, long_chain);
  B  maximal race-free launches (wide_vocab cut by race_free_cut);
  C  neg = 0 on a permutation in two-token sessions: the whole epoch is race-free (permutation).

Everything here is seeded NumPy; the seeds below were searched once on the host and are pinned by the CPU test."""
import numpy as np

import sgns_restatement as sr

RTOL, ATOL = 1e-4, 1e-6             # the project's fp32 band (test_sgns_gpu.py)
U32 = 2**32 - 1
NEGS = (0, 1, 3, 4, 5, 40, 64)      # nt = 1 + neg = 1, 2, 4, 5, 6, 41, 65: one four, a tail of 1 and 2, OTTO_SGNS_MAX_NEG
DIMS = (4, 8, 16, 32, 64, 128)      # G = d/4 = 1 .. 32
SG_GRID = 2048                      # csrc/otto_sgns.hip


def gpb(d):
    """lane groups (centres) per workgroup: the workgroup is min(256, 64 * G) threads of G = d/4 lanes per centre"""
    G = d // 4
    return 256 // G if G >= 4 else 64


def band_ratio(got, want):
    """largest |got - want| / (ATOL + RTOL |want|): <= 1 is inside the band"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want))))


def tables(n_rows, d, seed):
    """float32 [n_rows, d] uniform in [-0.5, 0.5)"""
    return np.random.default_rng(seed).random((n_rows, d), dtype=np.float32) - np.float32(0.5)


# ---------------------------------------------------------------------------
# shape A
# ---------------------------------------------------------------------------
TINY_SEED = 0
TINY_WS, TINY_AIDS = 3, 7


def tiny_vocab():
    """7 aids, sessions of 9, 3 and 2 events, nothing subsampled, ws = 3. Aid 1 holds 40/60 of the negative table and aid 3
    none of it, so at neg >= 3 most fours of a pair name a row more than once; tokens 1 and 2 are both aid 3, so a context
    equals its centre's aid."""
    aid = np.array([1, 3, 3, 0, 6, 1, 2, 5, 4, 6, 1, 0, 2, 6], dtype=np.int32)
    sess_off = np.array([0, 9, 12, 14], dtype=np.int64)
    weight = (np.array([9, 40, 3, 0, 5, 2, 1], dtype=np.uint32) * np.uint32(65536))
    keep_q = np.full(TINY_AIDS, U32, dtype=np.uint32)
    plans = [sr.plan(aid, sess_off, keep_q, TINY_SEED, ep, TINY_WS) for ep in (0, 1)]
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight), n_aids=TINY_AIDS,
                count=np.bincount(aid, minlength=TINY_AIDS).astype(np.int64), ws=TINY_WS, seed=TINY_SEED, plans=plans)


PATTERNS = (('four', 0, 1), ('four', 0, 3), ('four', 1, 2), ('four', 2, 3), 'three_in_a_four', 'across_fours',
            'negative_is_centre', 'context_is_centre')


def possible_patterns(neg):
    """The members of PATTERNS a target list of 1 + neg rows can show at all. Target 0 is the context, which no negative
    equals (the redraw rule), so position 0 of the first four never repeats: (0, b) needs a second four with more than b
    entries, three equal rows need three negatives in one four, and two fours need nt >= 5."""
    nt = 1 + neg
    sizes = [min(4, nt - m0) for m0 in range(0, nt, 4)]
    out = {'context_is_centre'}
    if neg >= 1:
        out.add('negative_is_centre')
    for a, b in ((0, 1), (0, 3), (1, 2), (2, 3)):
        if any(s > b and (j > 0 or a > 0) for j, s in enumerate(sizes)):
            out.add(('four', a, b))
    if any(s - (j == 0) >= 3 for j, s in enumerate(sizes)):
        out.add('three_in_a_four')
    if nt >= 5:
        out.add('across_fours')
    return out


def duplicate_patterns(p, ctx, negs, t0, t1):
    """The members of PATTERNS that the pairs of the centres [t0, t1) show; ctx / negs are sr.negatives over [t0, t1)."""
    seen, q = set(), 0
    for c in range(t0, t1):
        ca = int(p['tok_aid'][c])
        for _ in range(int(p['pair_off'][c + 1] - p['pair_off'][c])):
            tg = [int(ctx[q])] + [int(x) for x in negs[q]]
            if tg[0] == ca:
                seen.add('context_is_centre')
            if ca in tg[1:]:
                seen.add('negative_is_centre')
            fours = [tg[m0:m0 + 4] for m0 in range(0, len(tg), 4)]
            for j, four in enumerate(fours):
                for a, b in ((0, 1), (0, 3), (1, 2), (2, 3)):
                    if b < len(four) and four[a] == four[b]:
                        seen.add(('four', a, b))
                if max(four.count(t) for t in four) >= 3:
                    seen.add('three_in_a_four')
                if any(set(four) & set(other) for other in fours[j + 1:]):
                    seen.add('across_fours')
            q += 1
    return seen


CHAIN_SEED = 4
CHAIN_TOKENS, CHAIN_AIDS, CHAIN_WS, CHAIN_NEG = 80, 400, 32, 64


def long_chain():
    """One session of 80 kept tokens over 400 aids, ws = 32, neg = 64. `centres`: the first token, the last token and a
    centre with 2 * OTTO_SGNS_MAX_WS = 64 pairs (k runs to 63 in the negatives' keys); only these three are launched."""
    rng = np.random.default_rng(CHAIN_SEED)
    aid = np.minimum(rng.zipf(1.3, CHAIN_TOKENS) - 1, CHAIN_AIDS - 1).astype(np.int32)
    sess_off = np.array([0, CHAIN_TOKENS], dtype=np.int64)
    count = np.bincount(aid, minlength=CHAIN_AIDS).astype(np.int64)
    weight = np.floor(np.sqrt(count + 1.0) * 65536.0).astype(np.uint32)          # every aid can be drawn
    keep_q = np.full(CHAIN_AIDS, U32, dtype=np.uint32)
    p = sr.plan(aid, sess_off, keep_q, CHAIN_SEED, 0, CHAIN_WS)
    npairs = np.diff(p['pair_off'])
    full = np.flatnonzero(npairs == 2 * CHAIN_WS)
    centres = [0, CHAIN_TOKENS - 1] + [int(c) for c in full[:1]]
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight), n_aids=CHAIN_AIDS,
                count=count, ws=CHAIN_WS, neg=CHAIN_NEG, seed=CHAIN_SEED, plan=p, centres=centres)


# ---------------------------------------------------------------------------
# shape B
# ---------------------------------------------------------------------------
WIDE_NEGS = (2, 5)
WIDE_WS = 3
# seed per (d, neg): searched so that race_free_cut holds a launch with at least 2 * gpb(d) + 1 centres that have pairs
WIDE_SEEDS = {(d, neg): 0 for d in DIMS for neg in WIDE_NEGS}
WIDE_SEEDS[(16, 5)] = 1


def wide_n_aids(d):
    return min((1 << 24) // d, 1 << 21)          # a table stays at or below 64 MiB


def sparse_plan(p, active):
    """The plan p with the pair count of every token outside `active` set to zero. The step takes the plan as arrays, and a
    token without pairs is skipped, as the lone token of a one-token session is; tok_src, hence every key, is unchanged."""
    npairs = np.diff(p['pair_off']) * active
    q = dict(p)
    q['pair_off'] = np.concatenate(([0], np.cumsum(npairs))).astype(np.int64)
    q['tok_left'] = np.where(active, p['tok_left'], 0).astype(np.uint8)
    return q


def wide_vocab(d, neg, seed=None):
    """Sessions of 2 .. 7 tokens over a vocabulary of wide_n_aids(d) uniformly weighted aids, no aid twice, ws = 3.

    Centres c and c + 2 of one session both update the Out row of token c + 1, so a launch of consecutive centres of a real
    plan is race-free only across sessions of at most two tokens, where every centre has one pair. To put centres with
    1 .. 6 pairs side by side in one wave, one token per session keeps its pairs and the others get a pair count of zero
    (sparse_plan): `plan` is the real plan, `sparse` the one that is launched. The centres of a launch then meet only in
    their negatives, which race_free_cut sees."""
    seed = WIDE_SEEDS[(d, neg)] if seed is None else seed
    n_aids = wide_n_aids(d)
    rng = np.random.default_rng(1000 + seed)
    S = 3 * 129                                 # sessions: enough at every d for a centre with 6 pairs and for the long launch
    lens = rng.integers(2, 8, S)
    sess_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    aid = rng.permutation(n_aids)[:sess_off[-1]].astype(np.int32)
    active = np.zeros(sess_off[-1], dtype=bool)
    active[sess_off[:-1] + rng.integers(0, lens)] = True
    keep_q = np.full(n_aids, U32, dtype=np.uint32)
    weight = np.full(n_aids, 65536, dtype=np.uint32)
    p = sr.plan(aid, sess_off, keep_q, seed, 0, WIDE_WS)
    sparse = sparse_plan(p, active)
    cum = sr.cum_table(weight)
    T = len(p['tok_aid'])
    ctx, negs = sr.negatives(sparse, cum, seed, 0, neg, 0, T, n_aids)
    cut = race_free_cut(sparse, ctx, negs)
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=cum, n_aids=n_aids, ws=WIDE_WS, neg=neg,
                seed=seed, plan=p, sparse=sparse, active=active, ctx=ctx, negs=negs, cut=cut)


def race_free_cut(p, ctx, negs):
    """[(t0, t1)] covering the plan: each launch is extended greedily while the In rows of its centres are pairwise distinct
    and the Out-row sets of different centres are disjoint (a row may repeat inside one centre; a centre without pairs
    touches nothing). ctx / negs: sr.negatives over the whole plan, so the rows come from the restatement alone."""
    T = len(p['tok_aid'])
    cuts, t0, used_in, used_out = [], 0, set(), set()
    for c in range(T):
        lo, hi = int(p['pair_off'][c]), int(p['pair_off'][c + 1])
        rows_in = {int(p['tok_aid'][c])} if hi > lo else set()
        rows_out = set(ctx[lo:hi].tolist()) | set(negs[lo:hi].ravel().tolist())
        if (rows_in & used_in) or (rows_out & used_out):
            cuts.append((t0, c))
            t0, used_in, used_out = c, set(), set()
        used_in |= rows_in
        used_out |= rows_out
    if T > t0:
        cuts.append((t0, T))
    return cuts


def active_in(p, t0, t1):
    """the number of centres of [t0, t1) that have pairs"""
    return int((np.diff(p['pair_off'][t0:t1 + 1]) > 0).sum())


# ---------------------------------------------------------------------------
# shape C
# ---------------------------------------------------------------------------
PERM_DIMS = (128, 16)
PERM_LR = 0.05


def permutation(d):
    """T = SG_GRID * gpb + gpb + 3 tokens, every aid once, two-token sessions (T is odd: the last session has one token and
    no pair), ws = 1, neg = 0. Centre 2s touches In[a] and Out[b], centre 2s + 1 In[b] and Out[a]: no row is shared in the
    whole epoch, in HOGWILD or BATCH, so one launch sweeps the grid once and starts a ragged second sweep."""
    T = SG_GRID * gpb(d) + gpb(d) + 3
    aid = np.random.default_rng(d).permutation(T).astype(np.int32)
    sess_off = np.concatenate((np.arange(0, T, 2), [T])).astype(np.int64)
    return dict(aid=aid, sess_off=sess_off, keep_q=np.full(T, U32, dtype=np.uint32), weight=np.full(T, 65536, dtype=np.uint32),
                n_aids=T, ws=1, neg=0, seed=9, T=T)


def permutation_plan(pm, n_tokens=None):
    """The plan of permutation() in closed form (nothing is subsampled, ws = 1 makes every radius 1); n_tokens: a prefix."""
    T = pm['T'] if n_tokens is None else n_tokens
    sess_off = pm['sess_off'][pm['sess_off'] < T]
    sess_off = np.concatenate((sess_off, [T])).astype(np.int64)
    left = (np.arange(T) & 1).astype(np.uint8)
    npairs = np.ones(T, dtype=np.int64)
    if T & 1:
        npairs[-1] = 0
    return dict(tok_aid=pm['aid'][:T].copy(), tok_src=np.arange(T, dtype=np.int64), tok_off=sess_off,
                radius=np.ones(T, dtype=np.uint8), tok_left=left,
                pair_off=np.concatenate(([0], np.cumsum(npairs))).astype(np.int64))


def permutation_step(pm, In, Out, lr, n_tokens=None):
    """One step over the first n_tokens (an even number, or all) centres, vectorised: every In and Out row is touched by at
    most one pair, so the sequential loop and the batch step are the same expression per row. Returns (loss, ctx)."""
    T = pm['T'] if n_tokens is None else n_tokens
    pairs = pm['aid'][:T - (T & 1)].astype(np.int64).reshape(-1, 2)
    centre, ctx = pairs.ravel(), pairs[:, ::-1].ravel()
    lr = float(np.float32(lr))
    h, o = In[centre].astype(np.float64), Out[ctx].astype(np.float64)
    x = np.einsum('ij,ij->i', h, o)
    e = np.exp(-np.abs(x))
    g = lr * (1.0 - np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
    loss = float(np.sum(np.maximum(-x, 0.0) + np.log1p(e)))
    In[centre] = (h + g[:, None] * o).astype(np.float32)
    Out[ctx] = (o + g[:, None] * h).astype(np.float32)
    return loss, ctx.astype(np.int32)


# ---------------------------------------------------------------------------
# planted defects (plain NumPy, CPU test only)
# ---------------------------------------------------------------------------
def step_variant(p, cum, In, Out, seed, epoch, neg, lr, t0, t1, stale=False, carry=True, tail=True):
    """sr.step_sequential restated over fours of targets, with three switches that each plant one bug:
    stale     the rows of a four are read before its first update and never re-read (the DUP reload is missing);
    not carry every pair uses the In row from before the launch, the grads are summed at the end;
    not tail  the targets beyond the last full four are skipped.
    With the defaults it is the sequential loop itself."""
    n_aids = In.shape[0]
    ctx_all, neg_all = sr.negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    lr = float(np.float32(lr))
    loss, q = 0.0, 0
    for c in range(t0, t1):
        ca = int(p['tok_aid'][c])
        npair = int(p['pair_off'][c + 1] - p['pair_off'][c])
        if npair == 0:
            continue
        h0 = In[ca].astype(np.float64)
        h, total = h0, np.zeros_like(h0)
        for _ in range(npair):
            grad = np.zeros_like(h)
            tg = [int(ctx_all[q])] + [int(x) for x in neg_all[q]]
            n = len(tg) if tail else len(tg) // 4 * 4
            for m0 in range(0, n, 4):
                four = tg[m0:min(m0 + 4, n)]
                snap = [Out[t].astype(np.float64) for t in four]
                for i, t in enumerate(four):
                    o = snap[i] if stale else Out[t].astype(np.float64)
                    x = float(h @ o)
                    g = lr * ((1.0 if m0 + i == 0 else 0.0) - sr._sigmoid(x))
                    loss += sr._softplus(-x if m0 + i == 0 else x)
                    grad += g * o
                    Out[t] = (o + g * h).astype(np.float32)
            if carry:
                h = h + grad
            else:
                total += grad
            q += 1
        In[ca] = (h if carry else h0 + total).astype(np.float32)
    return loss


planted_defects = {
    'stale duplicate': dict(stale=True),
    'no carry': dict(carry=False),
    'dropped tail': dict(tail=False),
}
