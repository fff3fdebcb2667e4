"""Inputs shared by the SPEC-CBOW / SPEC-DOC2VEC tests (tests/test_sgns_cbow_cpu.py, tests/test_sgns_cbow_gpu.py) and
tests/golden/make_sgns_cbow_golden.py: the edge input, the permutation input with its Huffman tree, and the constants of the
learning test. Seeded NumPy; EDGE_SEED was searched once on the host and is pinned by the CPU test."""
import numpy as np

import sgns_cbow_restatement as cr
import sgns_hs_restatement as hr
import sgns_restatement as sr

U32 = 2**32 - 1
ARCHS = (('cbow-sum', cr.CBOW, cr.SUM), ('cbow-mean', cr.CBOW, cr.MEAN), ('cbow-fasttext', cr.CBOW, cr.FASTTEXT),
         ('pvdm-sum', cr.PVDM, cr.SUM), ('pvdm-mean', cr.PVDM, cr.MEAN), ('pvdm-fasttext', cr.PVDM, cr.FASTTEXT),
         ('dbow', cr.DBOW, cr.MEAN))

# the learning test: sgns_inputs' constants; three epochs teach CBOW, the two Doc2Vec archs need ten (a session's row is
# trained by its own six tokens alone)
EPOCHS_CBOW, EPOCHS_DOC = 3, 10
LEARN = (('cbow_mean', cr.CBOW, cr.MEAN, EPOCHS_CBOW), ('pvdm_mean', cr.PVDM, cr.MEAN, EPOCHS_DOC), ('dbow', cr.DBOW, cr.MEAN, EPOCHS_DOC))

# ---------------------------------------------------------------------------
# the edge input
# ---------------------------------------------------------------------------
EDGE_AIDS, EDGE_WS, EDGE_MIN_COUNT, EDGE_SEED = 40, 32, 2, 6
EDGE_KEPT = (1, 2, 3, 9, 70)                # kept tokens per session


def edge_input(seed=None):
    """40 aids: 0..29 occur at least twice, 30..35 once (dropped by min_count = 2), 36..39 never. t = 0, so nothing else is
    subsampled; ws = 32. Sessions of 1, 2, 3, 9 and 70 kept tokens, each with one or two dropped singletons inside. Session 2
    is (4, 4, 9): the window of centre 9 holds aid 4 twice, and centre 4 has a context equal to its own aid. In the 70-token
    session a centre near the middle with radius 32 has the maximal 64 contexts."""
    seed = EDGE_SEED if seed is None else seed
    rng = np.random.default_rng(77)
    long = np.concatenate((np.arange(30), np.arange(30)[::-1], rng.integers(0, 30, 10)))
    sessions = [[5, 30], [3, 31, 7], [4, 4, 32, 9], list(rng.integers(0, 30, 4)) + [33] + list(rng.integers(0, 30, 5)),
                list(long[:20]) + [34] + list(long[20:50]) + [35] + list(long[50:])]
    aid = np.array([a for s in sessions for a in s], dtype=np.int32)
    sess_off = np.concatenate(([0], np.cumsum([len(s) for s in sessions]))).astype(np.int64)
    count = np.bincount(aid, minlength=EDGE_AIDS).astype(np.int64)
    in_vocab = count >= EDGE_MIN_COUNT
    keep_q = np.where(in_vocab, U32, 0).astype(np.uint32)
    weight = np.where(in_vocab, np.floor(np.sqrt(count.astype(np.float64)) * 65536.0), 0).astype(np.uint32)
    plans = [sr.plan(aid, sess_off, keep_q, seed, ep, EDGE_WS) for ep in (0, 1)]
    return dict(aid=aid, sess_off=sess_off, count=count, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight), n_aids=EDGE_AIDS,
                ws=EDGE_WS, seed=seed, plans=plans, hs=hr.huffman(count, EDGE_MIN_COUNT))


# ---------------------------------------------------------------------------
# two-token sessions over a permutation (sgns_hogwild_inputs.permutation's shape, any size)
# ---------------------------------------------------------------------------
def permutation_tables(pm, d, seed=3):
    import sgns_hogwild_inputs as hi
    T = pm['T']
    return dict(In=hi.tables(T, d, seed), Out=hi.tables(T, d, seed + 1))


def permutation_cbow_step(pm, tabs, lr, n_tokens=None):
    """One CBOW step (any variant: every centre has one context, n = 1) with neg = 0 and no tree over the first n_tokens
    centres, vectorised: centre 2s reads and writes In[b] and Out[a], centre 2s + 1 In[a] and Out[b]; no row is shared, so
    the sequential loop and the batch step are the same expression per row. Returns the loss."""
    T = pm['T'] if n_tokens is None else n_tokens
    pairs = pm['aid'][:T - (T & 1)].astype(np.int64).reshape(-1, 2)
    centre, ctx = pairs.ravel(), pairs[:, ::-1].ravel()
    lr = float(np.float32(lr))
    h, o = tabs['In'][ctx].astype(np.float64), tabs['Out'][centre].astype(np.float64)
    x = np.einsum('ij,ij->i', h, o)
    e = np.exp(-np.abs(x))
    g = lr * (1.0 - np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
    tabs['In'][ctx] = (h + g[:, None] * o).astype(np.float32)
    tabs['Out'][centre] = (o + g[:, None] * h).astype(np.float32)
    return float(np.sum(np.maximum(-x, 0.0) + np.log1p(e)))


# ---------------------------------------------------------------------------
# the learning test
# ---------------------------------------------------------------------------
def doc_clusters(aid, sess_off, cluster):
    """a session's cluster is its first aid's cluster"""
    return cluster[aid[sess_off[:-1]]]


def knn_gram(E, k=10):
    """sgns_inputs.knn_numpy through the Gram matrix, for tables of a few thousand rows"""
    E = E.astype(np.float64)
    sq = (E * E).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * (E @ E.T)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind='stable')[:, :k]
