"""Inputs shared by the SGNS tests and tests/golden/make_sgns_golden.py: the planted-cluster sessions of the "hogwild
learns" test, the purity figure, and the restatement's trainer over them."""
import numpy as np

import sgns_restatement as sr

N_AIDS, N_CLUSTERS, N_SESSIONS, SESSION_LEN = 600, 12, 1500, 6
DIM, WS, NEG, EPOCHS, LR, T, MIN_COUNT, NS_EXPONENT = 32, 3, 3, 3, 0.25, 0.0, 1, 0.5
GOLDEN_SEEDS = (1, 2, 3, 4, 5)
# centres of one hogwild launch run side by side and do not see each other's updates: on 9,000 tokens a launch has to be
# much smaller than the epoch for the epoch to be a sequence of steps at all
TOKENS_PER_LAUNCH = 16


def planted_sessions(seed=2024):
    """(aid int32 [E], sess_off int64 [S+1], cluster int64 [N_AIDS]): every session draws its 6 aids from one cluster."""
    rng = np.random.default_rng(seed)
    cluster = np.arange(N_AIDS) % N_CLUSTERS
    members = [np.flatnonzero(cluster == c) for c in range(N_CLUSTERS)]
    aid = np.concatenate([rng.choice(members[rng.integers(N_CLUSTERS)], SESSION_LEN) for _ in range(N_SESSIONS)]).astype(np.int32)
    sess_off = (np.arange(N_SESSIONS + 1, dtype=np.int64) * SESSION_LEN)
    return aid, sess_off, cluster


def purity_from_ids(ids, cluster):
    """mean share of each aid's listed neighbours (ids [N, k], -1 = none) that lie in its own cluster"""
    ids = np.asarray(ids)
    same = (cluster[np.maximum(ids, 0)] == cluster[:, None]) & (ids >= 0)
    return float(same.mean())


def knn_numpy(E, k=10):
    """k nearest other rows under the euclidean distance (ties: the lower id)"""
    E = E.astype(np.float64)
    d2 = ((E[:, None, :] - E[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind='stable')[:, :k]


def train_sequential(seed, vocab_tables, init_tables, learning_rate):
    """The restatement's trainer on the planted sessions, in launches of TOKENS_PER_LAUNCH tokens (the cut only sets the
    learning rate of each stretch: the sequential loop itself does not depend on it). The host-side table builders are passed
    in (otto_amd.gensim_fasttext.skipgram's): they are checked on their own in test_sgns_cpu.py."""
    aid, sess_off, _ = planted_sessions()
    _, keep_q, weight = vocab_tables(aid, N_AIDS, MIN_COUNT, T, NS_EXPONENT)
    cum = sr.cum_table(weight)
    In, Out = init_tables(N_AIDS, DIM, seed)
    losses = []
    for ep in range(EPOCHS):
        p = sr.plan(aid, sess_off, keep_q, seed, ep, WS)
        T_ = len(p['tok_aid'])
        loss = 0.0
        for t0 in range(0, T_, TOKENS_PER_LAUNCH):
            lr = learning_rate(LR, ep * len(aid) + int(p['tok_src'][t0]), EPOCHS * len(aid))
            loss += sr.step_sequential(p, cum, In, Out, seed, ep, NEG, lr, t0, min(t0 + TOKENS_PER_LAUNCH, T_))
        losses.append(loss / (int(p['pair_off'][-1]) * (1 + NEG)))
    return In, Out, losses
