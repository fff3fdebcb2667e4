"""Inputs of the TF-IDF tests: session corpora with the edges SPEC-TFIDF names, as (aid int32 [E], typ uint8 [E], sess_off
int64 [S + 1]). Functions of their arguments alone."""
import numpy as np


def from_lists(sessions, seed=0):
    """list of aid lists -> (aid, typ, sess_off); the event types are drawn from the seed"""
    lens = np.array([len(s) for s in sessions], dtype=np.int64)
    off = np.zeros(len(sessions) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    aid = np.array([a for s in sessions for a in s], dtype=np.int32)
    typ = np.random.default_rng(seed).choice(3, size=len(aid), p=(0.8, 0.15, 0.05)).astype(np.uint8)
    return aid, typ, off


def random_lists(n_sessions, n_aids, seed, max_len=9, min_len=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sessions):
        n = int(rng.integers(min_len, max_len + 1))
        # a skewed draw: small aids are popular, so rows share columns and every aid below 10 occurs
        out.append(np.minimum((rng.random(n) ** 2 * n_aids).astype(np.int64), n_aids - 1).tolist())
    return out


def sklearn_corpus(common_aid=None, n_sessions=240, n_aids=60, seed=5):
    """A few hundred random sessions over about 60 aids with: aids 0..9, a session of one-digit aids only, a session that
    repeats one aid three times, two identical sessions, a session of 25 distinct aids (the recency branch). With
    ``common_aid`` that aid is put into every session (and no session is left with one-digit aids alone)."""
    lists = random_lists(n_sessions, n_aids, seed)
    lists[3] = [4, 7, 4, 9]                                  # one-digit aids only: an all-zero row under min_aid = 10
    lists[5] = [23, 23, 23]
    lists[8] = [31, 12, 45, 12]
    lists[9] = list(lists[8])                                # identical to session 8
    lists[11] = [17]
    lists[14] = list(range(30, 55))                          # 25 distinct aids
    lists[15] = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    if common_aid is not None:
        lists = [s + [common_aid] for s in lists]
    return from_lists(lists, seed), n_aids


def shape_case(D, n_aids, seed=0):
    """D documents over n_aids aids: lengths 0..8, an empty document and a document of one token where D allows"""
    lists = random_lists(D, n_aids, seed + 31 * D + n_aids, max_len=8, min_len=0)
    if D >= 2:
        lists[1] = []
    if D >= 3:
        lists[2] = [n_aids - 1]
    if D >= 5:
        lists[4] = list(lists[3])                            # identical rows: ties go to the smaller id
    return from_lists(lists, seed)


def long_document(length=20000, n_aids=200, seed=1):
    """one document of ``length`` tokens between short ones (longer than a radix tile of 4096 keys and than the 16384
    keys one sorting workgroup takes)"""
    rng = np.random.default_rng(seed)
    lists = random_lists(6, n_aids, seed, max_len=8, min_len=0)
    lists.insert(3, rng.integers(0, n_aids, size=length).tolist())
    return from_lists(lists, seed)


def hub_corpus(H, n_other=30, seed=2):
    """Aid ``hub`` occurs in H documents. Document 0 holds it alone: its candidate bound in the session direction is H.
    Documents 1..H-1 hold it 1 to 3 times next to an aid of their own (bound H + 1; repeated patterns: ties). ``n_other``
    small documents over other aids follow. Returns ((aid, typ, sess_off), n_aids, hub)."""
    hub = 10
    lists = [[hub]]
    for d in range(1, H):
        lists.append([hub] * (1 + d % 3) + [hub + d])
    first_other = hub + H
    rng = np.random.default_rng(seed)
    for _ in range(n_other):
        lists.append((first_other + rng.integers(0, 12, size=int(rng.integers(1, 5)))).tolist())
    return from_lists(lists, seed), first_other + 12, hub
