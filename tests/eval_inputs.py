"""Seeded inputs of the SPEC-EVAL tests. A session is (aids, types, cutoff); ``pack`` lays sessions out as the SoA columns
and the CSR offsets the library takes. The capacities named here are the ones csrc/otto_eval.hip stages by."""
import numpy as np

EVAL_SHORT = 8          # sessions up to this long run on an 8-lane group
EVAL_WAVE = 64          # up to this long on one wave, longer on a workgroup
EVAL_LDS_KEYS = 2048    # cart / order events of a tail a workgroup sorts in LDS; more are sorted in global memory
AID_MAX = 2 ** 31 - 1

S_SIZES = (0, 1, 63, 64, 65, 257)
LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 128, 129)


def pack(sessions):
    """[(aids, types, cutoff)] -> aid int32, ts int32, typ uint8, sess_off int64, cutoff int32."""
    aid = np.concatenate([np.asarray(a, dtype=np.int64) for a, _, _ in sessions] + [np.zeros(0, np.int64)]).astype(np.int32)
    typ = np.concatenate([np.asarray(t, dtype=np.int64) for _, t, _ in sessions] + [np.zeros(0, np.int64)]).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(a) for a, _, _ in sessions])]).astype(np.int64)
    ts = (1_659_000_000 + np.arange(len(aid)) * 7 % 1000 + np.arange(len(aid))).astype(np.int32)
    cutoff = np.asarray([c for _, _, c in sessions], dtype=np.int32)
    return aid, ts, typ, off, cutoff


def random_session(rng, n, n_aids=50, p=(0.6, 0.25, 0.15), cutoff=None):
    aids = rng.integers(0, n_aids, n)
    types = rng.choice(3, n, p=p)
    if cutoff is None:
        cutoff = int(rng.integers(0, n)) if n else 0
    return aids, types, cutoff


def sized_case(S, seed=0):
    """S sessions of OTTO-like lengths (mostly a few events, some past every group size)."""
    rng = np.random.default_rng(1000 + 31 * S + seed)
    out = []
    for s in range(S):
        r = rng.random()
        n = int(rng.integers(0, 9)) if r < 0.7 else int(rng.integers(9, 65)) if r < 0.93 else int(rng.integers(65, 400))
        out.append(random_session(rng, n, n_aids=int(rng.choice((3, 40, 100000)))))
    return out


def length_cases():
    """Every length of LENGTHS with the cutoff at 0, in the middle and at n - 1: the tail takes every length too."""
    rng = np.random.default_rng(77)
    out = []
    for n in LENGTHS:
        for cut in sorted({0, n // 2, max(n - 2, 0), max(n - 1, 0)}):
            out.append(random_session(rng, n, n_aids=max(n // 3, 2), cutoff=cut))
            out.append(random_session(rng, n, n_aids=1000, cutoff=cut))
    return out


def tail_cases():
    """Every length of LENGTHS as the TAIL length n - cutoff - 1, behind kept parts of 1 event and of 71 events (so the
    session is on the group, the wave or the workgroup path), with mixed types and with cart / order events only: then
    the number of keys the workgroup sorts is the tail length itself (65, 128 and 129 among them)."""
    rng = np.random.default_rng(99)
    out = []
    for tail in LENGTHS:
        for kept in (1, 71):
            n = kept + tail
            for n_aids in (max(tail // 3, 2), AID_MAX):
                out.append((rng.integers(0, n_aids, n), rng.choice(3, n, p=(0.5, 0.3, 0.2)), kept - 1))
                out.append((rng.integers(0, n_aids, n), np.r_[np.zeros(kept, np.int64), rng.integers(1, 3, tail)], kept - 1))
    # tails of 65 and 129 once more on sessions of 66, 130 and 200 events, cart / order only and mixed
    for n, cut in ((66, 0), (130, 0), (200, 134), (200, 70)):
        out.append((rng.integers(0, 1000, n), np.r_[np.zeros(cut + 1, np.int64), rng.integers(1, 3, n - cut - 1)], cut))
        out.append((rng.integers(0, 1000, n), rng.choice(3, n), cut))
    return out


def edge_cases():
    rng = np.random.default_rng(5)
    out = []
    for n in (1, 2, 5, 8, 9, 40, 64, 65, 300):
        for t in (0, 1, 2):                                              # one type only
            out.append((rng.integers(0, 9, n), np.full(n, t), 0))
        no_click = rng.integers(1, 3, n)
        out.append((rng.integers(0, 9, n), no_click, 0))                 # no click at all
        first = no_click.copy()
        first[0] = 0
        out.append((rng.integers(0, 9, n), first, 0))                    # a click only at index 0
        last = no_click.copy()
        last[-1] = 0
        out.append((rng.integers(0, 9, n), last, 0))                     # a click only at n - 1
        out.append((np.full(n, 12345), rng.integers(1, 3, n), 0))        # the tail is one aid repeated
        out.append((rng.choice([0, AID_MAX], n), rng.integers(0, 3, n), 0))   # the smallest and the largest aid
        out.append((rng.choice([0, 1, AID_MAX - 1, AID_MAX], n), rng.integers(1, 3, n), max(n - 1, 0)))   # cutoff at n - 1
    return out


def capacity_cases():
    """Tails whose cart / order events number one below, at and one above EVAL_LDS_KEYS, all distinct and with heavy
    repeats, and one tail of several thousand events with more distinct aids than the LDS buffer holds."""
    rng = np.random.default_rng(11)
    out = []
    for m in (EVAL_LDS_KEYS - 1, EVAL_LDS_KEYS, EVAL_LDS_KEYS + 1):
        for n_aids in (AID_MAX, 300):
            aids = np.concatenate([[7, 8, 9], rng.integers(0, n_aids, m)])
            types = np.concatenate([[0, 0, 0], rng.integers(1, 3, m)])   # m label events after cutoff 2
            out.append((aids, types, 2))
    n = 6000
    aids = rng.permutation(n).astype(np.int64) * 357_913 % AID_MAX       # ~6000 distinct aids, far apart
    types = rng.choice(3, n, p=(0.1, 0.5, 0.4))
    out.append((aids, types, 10))
    out.append((rng.integers(0, 5000, 9000), rng.choice(3, 9000, p=(0.05, 0.05, 0.9)), 0))   # one list takes nearly all
    return out


def split_cases():
    cases = {f'S_{S}': sized_case(S) for S in S_SIZES}
    cases['lengths'] = length_cases()
    cases['tails'] = tail_cases()
    cases['edges'] = edge_cases()
    cases['capacities'] = capacity_cases()
    cases['empty_sessions'] = [((), (), 0)] * 70
    return cases


def label_lists(rng, S, n_aids, long_every=0):
    """S label lists: mostly 0..3 aids, duplicates allowed; every ``long_every``-th longer than 20."""
    out = []
    for s in range(S):
        n = int(rng.integers(0, 4))
        if long_every and s % long_every == 1:
            n = int(rng.integers(21, 60))
        out.append([int(v) for v in rng.integers(0, n_aids, n)])
    return out


def to_csr(lists):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.asarray([v for x in lists for v in x], dtype=np.int32)
    return off, flat


def padded_case(S, k, seed=0):
    """(labels lists, pred int32 [S, k] with -1 padding at the end and in the middle, pred_n int32 [S])."""
    rng = np.random.default_rng(400 + S * 7 + k + seed)
    n_aids = 3 * k + 5
    labels = label_lists(rng, S, n_aids, long_every=9)
    pred = rng.integers(0, n_aids, (S, k)).astype(np.int32)          # few aids: duplicates within a row are common
    n = rng.integers(0, k + 1, S).astype(np.int32)
    n[::5] = 0
    n[1::5] = k
    for s in range(S):
        pred[s, n[s]:] = -1
        if n[s] > 2 and s % 3 == 0:
            pred[s, int(rng.integers(0, n[s] - 1))] = -1             # padding in the middle of a row
    return labels, pred, n


def csr_case(S, seed=0):
    """(label lists, prediction rows of 0, 1, 64, 65 and about 1,000 entries)."""
    rng = np.random.default_rng(900 + S + seed)
    lens = [0, 1, 64, 65, 1000, 1023, 20, 21, 19]
    labels = label_lists(rng, S, 1500, long_every=4)
    rows = []
    for s in range(S):
        row = rng.integers(0, 1500, lens[s % len(lens)])
        if len(row) > 3:
            row[int(rng.integers(0, len(row)))] = -1
        rows.append([int(v) for v in row])
    return labels, rows


def subset_ids(S, seed=0):
    """(label_session int32 [S] ascending with gaps, the positions of a strict subset)."""
    rng = np.random.default_rng(seed + S)
    ids = np.cumsum(rng.integers(1, 5, S)).astype(np.int32) + 11098528
    take = np.flatnonzero(rng.random(S) < 0.6)
    return ids, take
