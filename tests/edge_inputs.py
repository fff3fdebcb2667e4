"""Input generators, references and bounds shared by the edge-shape parity tests (test_events_sort_gpu, test_pairs_gpu,
test_inter_gpu, test_score_gpu). Plain NumPy; nothing here touches a device. ``tests/test_edge_cases_cpu.py`` asserts that
every generator has the property its name claims, so that the GPU tests cannot pass vacuously.

Kernel geometry restated here (so that the inputs can be aimed at it):
    radix sort (csrc/otto_events.hip)   wave 64, block 256, tile 4096 keys, workgroup span 4 tiles = 16384 keys,
                                        key = session << 32 | seconds, eight 8-bit passes, constant digits skipped
    scoring (csrc/otto_mf.hip)          row tile 128, item tile 32, item range split by ``score_split`` below
"""
import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of float32

# ---------------------------------------------------------------------------------------------------------------------
# 1. radix sort
# ---------------------------------------------------------------------------------------------------------------------
WAVE, BLOCK, TILE, SPAN = 64, 256, 4096, 16384
SORT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 1, 65536 + 17)
SORT_PATTERN_SIZES = (3001, 5 * 16384 + 77)            # below a tile; several workgroups
SORT_PATTERNS = ('all_equal', 'bit0', 'bit30', 'bit63', 'bytes05', 'high_sessions', 'descending', 'sorted', 'tile_one_digit',
                 'ts_extremes', 'ms_remainders', 'seconds_div1')
TIE_PATTERNS = ('ties3', 'all_equal', 'bit0', 'bit30', 'bit63', 'ts_extremes', 'ms_remainders')
TIES3_KEYS = ((5, 100), (5, 200), (9, 100))            # (session, seconds)


def sort_case(pattern, n, seed=0):
    """(session uint32 [n], ts int64 [n], ts_div) of one key pattern."""
    rng = np.random.default_rng([seed, n, sum(map(ord, pattern))])
    i = np.arange(n, dtype=np.int64)
    div = 1
    if pattern == 'generic':                       # sparse session ids, coarse millisecond stamps with remainders
        sess = rng.integers(0, n // 8 + 1, n) * 7 + 11_000_000
        sec = 1_659_304_800 + rng.integers(0, 3000, n) * 40
        ts, div = sec * 1000 + rng.integers(0, 1000, n), 1000
    elif pattern == 'ties3':                       # three distinct keys
        pick = rng.integers(0, 3, n)
        k = np.array(TIES3_KEYS, dtype=np.int64)
        sess, ts = k[pick, 0], k[pick, 1]
    elif pattern == 'all_equal':                   # no byte varies: no pass runs
        sess, ts = np.full(n, 12_345_678), np.full(n, 1_659_304_800)
    elif pattern == 'bit0':
        sess, ts = np.full(n, 77), 1000 + rng.integers(0, 2, n)
    elif pattern == 'bit30':                       # the highest bit of the seconds that the range check lets vary
        sess, ts = np.full(n, 77), 5 + (rng.integers(0, 2, n) << 30)
    elif pattern == 'bit63':                       # = bit 31 of the session id
        sess, ts = 9 + (rng.integers(0, 2, n) << 31), np.full(n, 1000)
    elif pattern == 'bytes05':                     # key bytes 0 and 5 vary; 1-4, 6, 7 constant (skips in the middle and on top)
        sess = 0x12340056 | (rng.integers(0, 256, n) << 8)
        ts = 0x62E70000 | 0x4200 | rng.integers(0, 256, n)
    elif pattern == 'high_sessions':               # ids in [2^31, 2^32) mixed with small ones
        hi = rng.integers(0, 2, n).astype(bool)
        sess = np.where(hi, (1 << 31) + rng.integers(0, 1 << 31, n), rng.integers(0, 50, n))
        if n >= 2:
            sess[0], sess[1] = (1 << 32) - 1, 1 << 31
        ts = 1_659_304_800 + rng.integers(0, 100, n)
    elif pattern in ('descending', 'sorted'):      # distinct keys, strictly monotone
        r = i if pattern == 'sorted' else n - 1 - i
        sess, ts = 1000 + r // 1000, 500 + r % 1000
    elif pattern == 'tile_one_digit':              # pass 0: every key of a tile holds ONE digit value (byte 0 = tile number;
        b0 = (i // TILE) % 255                     # the last row one more, so the byte varies even below a tile); byte 1 varies
        if n:
            b0[-1] += 1
        sess, ts = np.full(n, 3), 0x01000000 | (rng.integers(0, 256, n) << 8) | b0
    elif pattern == 'ts_extremes':
        sess = rng.integers(0, 4, n)
        ts = np.array([0, 1, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.int64)[rng.integers(0, 4, n)]
        if n >= 2:
            ts[0], ts[1] = 2 ** 31 - 1, 0
    elif pattern == 'ms_remainders':               # remainders DEscend inside every key: leaking into the key reverses ties
        sess = rng.integers(0, 5, n)
        sec = 1_659_304_800 + rng.integers(0, 3, n)
        ts, div = sec * 1000 + (999 - i % 1000), 1000
    elif pattern == 'seconds_div1':
        sess = rng.integers(0, n // 4 + 1, n)
        ts = 1_659_304_800 + rng.integers(0, 5000, n)
    else:
        raise ValueError(pattern)
    return np.asarray(sess, dtype=np.int64).astype(np.uint32), np.asarray(ts, dtype=np.int64), div


def sort_reference(sess, ts, div):
    """Stable (session, seconds) order and the CSR it implies, int64 NumPy."""
    s64 = sess.astype(np.int64)
    sec = ts // div
    order = np.lexsort((sec, s64))
    ss = s64[order]
    head = np.r_[True, ss[1:] != ss[:-1]] if len(ss) else np.zeros(0, dtype=bool)
    off = np.r_[np.flatnonzero(head), len(ss)].astype(np.int64)
    return order, sec[order], ss[head], off


def key_bytes_varying(sess, ts, div):
    """Which of the eight bytes of session << 32 | seconds differ somewhere in the input (bool [8], byte 0 = lowest)."""
    key = (sess.astype(np.uint64) << np.uint64(32)) | (ts // div).astype(np.uint64)
    var = np.bitwise_or.reduce(key) ^ np.bitwise_and.reduce(key)
    return np.array([(int(var) >> (8 * b)) & 255 != 0 for b in range(8)])


# ---------------------------------------------------------------------------------------------------------------------
# 2. aid pairs
# ---------------------------------------------------------------------------------------------------------------------
MAX_AID = 1_855_602
T0 = 1_659_304_800
DT_NAMES = ('max_dt', 'max_dt+1', '0', '-1', '86400', '90000')
AID_DT_SHARED = (2000, 2001)           # one pair of aids that meets all six dt values
AID_DT_EACH = 2100                     # pair (2100 + 2 q, 2101 + 2 q) meets dt number q only
AID_HALF = (3000, 3001)                # 3 of 6 labels are ones: mean 0.5 -> 1
AID_BELOW_HALF = (3002, 3003)          # 2 of 6 -> 0
TIME_BIG = dict(n_sess=40_000, n_aids=5000, max_len=60, p=0.12, seed=31)      # the 'time' builder at size


def stream_to_frame(sessions):
    """sessions: list of (aids, ts) per CSR row -> (aid int32, ts int32, sess_off int64, pandas frame for the oracle). A
    session's rows are put in (ts, position) order, as the sorted stream holds them; empty sessions get no frame rows."""
    import pandas as pd
    aid, ts, sid, off = [], [], [], [0]
    for s, (a, t) in enumerate(sessions):
        a, t = np.asarray(a, dtype=np.int64), np.asarray(t, dtype=np.int64)
        o = np.argsort(t, kind='stable')
        aid.append(a[o]); ts.append(t[o]); sid.append(np.full(len(a), s, dtype=np.int64))
        off.append(off[-1] + len(a))
    aid, ts, sid = np.concatenate(aid), np.concatenate(ts), np.concatenate(sid)
    fr = pd.DataFrame({'session': sid, 'aid': aid, 'ts': ts, 'type': np.zeros(len(aid), dtype=np.uint8)})
    return aid.astype(np.int32), ts.astype(np.int32), np.array(off, dtype=np.int64), fr


def time_edge_sessions(max_dt, seed=0):
    """The hand-built 'time' stream of the issue: empty sessions at the start, between sessions, two in a row and at the
    end; sessions of 1, 2, 3 (a repeated aid, equal stamps), 64, 65 and 300 events; dt edges; a 0.5 mean; extreme aids."""
    rng = np.random.default_rng(seed)
    dts = (max_dt, max_dt + 1, 0, -1, 86_400, 90_000)
    S = [([], [])]                                                    # empty at the start
    S.append(([41], [T0]))
    S.append(([], []))                                                # empty between
    S.append(([42, 43], [T0, T0 + 7]))
    S += [([], []), ([], [])]                                         # two in a row
    S.append(([44, 44, 45], [T0 + 3, T0 + 3, T0 + 3]))                # repeated aid, equal stamps
    for n in (64, 65, 300):
        S.append((rng.integers(100, 130, n), T0 + np.sort(rng.integers(0, 3 * max_dt, n))))
    for q, dt in enumerate(dts):
        S.append(([AID_DT_SHARED[0], AID_DT_SHARED[1]], [T0 + 100_000, T0 + 100_000 + dt]))
        S.append(([AID_DT_EACH + 2 * q, AID_DT_EACH + 2 * q + 1], [T0 + 100_000, T0 + 100_000 + dt]))
    for pair, ones in ((AID_HALF, 3), (AID_BELOW_HALF, 2)):
        for r in range(6):
            S.append(([pair[0], pair[1]], [T0, T0 + (10 if r < ones else max_dt + 5)]))
    S.append(([0, MAX_AID], [T0, T0 + 5]))                            # aid 0 and the largest aid, as x1 and as x2
    S.append(([], []))                                                # empty at the end
    return S


def random_sessions(n_sess, n_aids, max_len, p, seed, t_spread=4000):
    """Sessions of 1 + geometric(p) events capped at ``max_len``; stamps ascending inside a session."""
    rng = np.random.default_rng(seed)
    ln = np.minimum(rng.geometric(p, n_sess), max_len)
    return [(rng.integers(0, n_aids, n), T0 + np.sort(rng.integers(0, t_spread, n))) for n in ln]


def raw_time_slots(sess_off):
    n = np.diff(sess_off)
    return int((n * (n - 1)).sum())


def diff_edge_stream():
    """Hand-built 'diff' stream: (sessions, shuffle_keys). Sessions of 1, 2, 3 events, one repeated aid, keys 0 and
    2^31 - 1, and the pair (10, 11) positive in one session and negative in another."""
    big = 2 ** 31 - 1
    S = [([7], [T0]),
         ([8, 9], [T0, T0 + 1]),
         ([10, 11, 12], [T0, T0 + 1, T0 + 2]),          # keys (2, 3, 1): shuffled [12, 10, 11] -> (10, 11) positive
         ([10, 13, 11], [T0, T0 + 1, T0 + 2]),          # keys (2, 3, 1): shuffled [11, 10, 13] -> (10, 11) negative
         ([33, 33, 33, 33], [T0, T0 + 1, T0 + 2, T0 + 3]),   # one repeated aid: nothing survives
         ([20, 21, 22, 23], [T0, T0 + 1, T0 + 2, T0 + 3]),   # keys (big, 0, big, 0): shuffled [21, 23, 20, 22]
         ([50, 51, 52], [T0, T0 + 1, T0 + 2])]          # keys (1, 0, 2): shuffled [51, 50, 52]: row 0 x2 == x3, row 1 x1 == x3
    keys = [5, 1, 2, 2, 3, 1, 2, 3, 1, 4, 4, 4, 4, big, 0, big, 0, 1, 0, 2]
    return S, np.array(keys, dtype=np.uint64)


def pair_rows(cols):
    """(x1, x2, target) columns -> int64 rows sorted by (x1, x2)."""
    a = np.stack([np.asarray(c, dtype=np.int64) for c in cols], 1) if len(cols[0]) else np.zeros((0, 3), dtype=np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


# ---------------------------------------------------------------------------------------------------------------------
# 3. interaction features
# ---------------------------------------------------------------------------------------------------------------------
INTER_LONG_CYCLE = (1, 3, 4, 5, 509, 510, 511, 512)
SCORE_KINDS = ('fractional', 'negative', 'mixed', 'counts')


def inter_scores(kind, shape, rng):
    """float32 scores whose float64 sums are exact: multiples of 2^-10 of small magnitude, or small integer counts."""
    if kind == 'fractional':
        v = rng.integers(1, 4 * 1024 + 1, shape) / 1024.0                  # recency weights in (0, 4]
    elif kind == 'negative':
        v = -rng.integers(1, 8 * 1024, shape) / 1024.0
    elif kind == 'mixed':
        v = rng.integers(-8 * 1024, 8 * 1024, shape) / 1024.0
    elif kind == 'counts':
        v = rng.integers(1, 200, shape).astype(np.float64)
    else:
        raise ValueError(kind)
    return v.astype(np.float32)


def one_pass_std(x, rng=None):
    """The kernels' formula in float64: sqrt((sum x^2 - n mean^2) / (n - 1)), summed in the order ``rng`` shuffles to."""
    x = np.asarray(x, dtype=np.float64)
    if rng is not None:
        x = x[rng.permutation(len(x))]
    n = float(len(x))
    s = sq = 0.0
    for v in x.tolist():
        s += v
        sq += v * v
    mean = s / n
    return float(np.sqrt(max((sq - n * mean * mean) / (n - 1.0), 0.0)))


def one_pass_error(x, orders=5, seed=0):
    """Largest relative error of ``one_pass_std`` over several summation orders against the two-pass float64 std."""
    rng = np.random.default_rng(seed)
    want = float(np.std(np.asarray(x, dtype=np.float64), ddof=1))
    return max(abs(one_pass_std(x, rng) - want) / want for _ in range(orders))


def inter_sessions(lengths, n_aids, seed):
    """(aid int32, type uint8, sess_off int64) of sessions with the given lengths; aids repeat inside long sessions."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    aid = rng.integers(0, n_aids, int(off[-1])).astype(np.int32)
    typ = rng.integers(0, 3, int(off[-1])).astype(np.uint8)
    return aid, typ, off


def events_frame(aid, typ, off):
    import pandas as pd
    n = np.diff(off)
    sid = np.repeat(np.arange(len(n)), n)
    pos = np.arange(len(aid)) - np.repeat(off[:-1], n)
    return pd.DataFrame({'session': sid.astype(np.int64), 'aid': aid.astype(np.int64), 'ts': pos.astype(np.int64), 'type': typ})


def unique_candidates(rng, own, n_aids, n):
    """n distinct candidate aids: about half from the session's own aids, the rest from the catalogue."""
    own = np.unique(own)
    take = rng.permutation(own)[:min(len(own), (n + 1) // 2)]
    rest = np.setdiff1d(rng.permutation(n_aids)[:n + len(take) + 8], take, assume_unique=False)
    out = np.r_[take, rng.permutation(rest)][:n]
    assert len(out) == n and len(np.unique(out)) == n
    return rng.permutation(out).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 4. scoring
# ---------------------------------------------------------------------------------------------------------------------
SCORE_D = (8, 16, 32, 64, 128)
SCORE_K = (1, 2, 19, 20, 31, 32)
SCORE_B = (1, 31, 32, 33, 127, 128, 129, 300)
SCORE_N = (1, 31, 32, 33, 1023, 1024, 1025, 2049, 40_000)
SCORE_PAD = ('none', 'first', 'last', 'split', 'mid')
SC_BM, SC_BN = 128, 32


def score_split(B, N):
    """(number of splits, items per split) of ``score_nsplit`` and its caller, restated."""
    row_tiles = (B + SC_BM - 1) // SC_BM
    ns = max(1, min((1024 + row_tiles - 1) // row_tiles, (N + 32 * SC_BN - 1) // (32 * SC_BN)))
    per = ((N + ns - 1) // ns + SC_BN - 1) // SC_BN * SC_BN
    return ns, per


def pad_col_of(kind, B, N):
    """The masked column of a pad kind; None where the kind does not exist at this shape ('split' needs two splits)."""
    ns, per = score_split(B, N)
    if kind == 'none':
        return -1
    if kind == 'first':
        return 0
    if kind == 'last':
        return N - 1
    if kind == 'split':
        return per if ns > 1 and per < N else None           # first item of the second split
    if kind == 'mid':
        return min(N - 1, SC_BN * (N // (2 * SC_BN)) + 13)    # inside an item tile, not on its edge (when N allows)
    raise ValueError(kind)


def score_cases(seed=7):
    """A pairwise cover of SCORE_D x SCORE_K x SCORE_B x SCORE_N x SCORE_PAD: every pair of values of two different
    parameters that can occur together occurs in some case. Deterministic greedy choice among seeded random draws."""
    axes = (SCORE_D, SCORE_K, SCORE_B, SCORE_N, SCORE_PAD)
    ok = lambda c: pad_col_of(c[4], c[2], c[3]) is not None
    rng = np.random.default_rng(seed)
    need = set()
    for i in range(5):
        for j in range(i + 1, 5):
            for a in axes[i]:
                for b in axes[j]:
                    need.add((i, a, j, b))
    # drop the pairs no valid case can hold ('split' where the item range is not split)
    for i, a, j, b in list(need):
        fixed = {i: a, j: b}
        if not any(ok((0, 0, B, N, fixed.get(4, 'none'))) for B in ([fixed[2]] if 2 in fixed else SCORE_B)
                   for N in ([fixed[3]] if 3 in fixed else SCORE_N)):
            need.discard((i, a, j, b))
    pairs_of = lambda c: {(i, c[i], j, c[j]) for i in range(5) for j in range(i + 1, 5)}
    cases = []
    while need:
        best, gain = None, 0
        for _ in range(300):
            c = tuple(ax[int(rng.integers(0, len(ax)))] for ax in axes)
            if not ok(c):
                continue
            g = len(pairs_of(c) & need)
            if g > gain:
                best, gain = c, g
        if best is None:                              # a rare leftover pair: complete it directly
            i, a, j, b = sorted(need)[0]
            while True:
                c = list(ax[int(rng.integers(0, len(ax)))] for ax in axes)
                c[i], c[j] = a, b
                if ok(tuple(c)):
                    best = tuple(c)
                    break
        cases.append(best)
        need -= pairs_of(best)
    return cases


def exact_inputs(B, N, d, seed):
    """Integers in [-4, 4] as float32: every product and partial sum is an integer below 2^24 in magnitude, so the fp32 dot
    product is exact in any order. The N item rows are drawn (with repetition) from N // 4 distinct vectors, so every score
    of a row occurs about four times, at unrelated ids: ties at every place of the list, across tiles and splits."""
    rng = np.random.default_rng([seed, B, N, d])
    pool = rng.integers(-4, 5, (max(1, N // 4), d)).astype(np.float32)
    return rng.integers(-4, 5, (B, d)).astype(np.float32), pool[rng.integers(0, len(pool), N)]


def float_inputs(B, N, d, seed):
    rng = np.random.default_rng([seed, B, N, d, 1])
    return rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)


def dot_bound(U, V):
    """(S64, bound): the float64 scores and the forward error bound of an fp32 dot product of length d in ANY summation order,
    gamma_(d+1) sum_i |U_bi V_ni| (one rounding per product and d - 1 per sum, Higham, Accuracy and Stability, section 3.1; d + 1
    covers a fused or unfused accumulate either way)."""
    d = U.shape[1]
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    gamma = (d + 1) * U32 / (1.0 - (d + 1) * U32)
    return U64 @ V64.T, gamma * (np.abs(U64) @ np.abs(V64).T)


def topk_padded(score_topk, U, V, k, pad_col):
    """``mf_oracle.score_topk`` where fewer than k items are valid: the oracle is asked for min(k, N), masked entries
    (score -inf) and the missing tail become id -1 / score -inf, which is what the kernel writes there."""
    N = V.shape[0]
    kk = min(k, N)
    wi, ws = score_topk(U, V, k=kk, pad_col=pad_col)
    ids = np.full((U.shape[0], k), -1, dtype=np.int32)
    sc = np.full((U.shape[0], k), -np.inf)
    ids[:, :kk], sc[:, :kk] = wi, ws
    ids[np.isneginf(sc)] = -1
    return ids, sc


def merge_lists(n_lists, B, k, seed):
    """Partial top-k lists [n_lists, B, k] as item-sharded scoring leaves them: per list sorted by (score desc, id asc),
    ids distinct across lists, scores from a handful of values (ties across lists), empty slots at the tail written as
    -1 in even lists and 0x7FFFFFFF in odd ones, with score -inf; some lists wholly empty."""
    rng = np.random.default_rng([seed, n_lists, B, k])
    ps = np.full((n_lists, B, k), -np.inf, dtype=np.float32)
    pi = np.empty((n_lists, B, k), dtype=np.int32)
    for w in range(n_lists):
        pi[w] = -1 if w % 2 == 0 else 0x7FFFFFFF
        for b in range(B):
            n = int(rng.integers(0, k + 1)) if (b + w) % 4 else (k if w % 2 else 0)
            ids = np.sort(rng.permutation(4 * k)[:n]) * n_lists + w            # distinct across lists
            sc = rng.integers(-2, 3, n).astype(np.float32)
            o = np.lexsort((ids, -sc))
            ps[w, b, :n], pi[w, b, :n] = sc[o], ids[o]
    return ps, pi


def merge_reference(ps, pi, k):
    """NumPy lexsort of the union of the non-empty slots, (score desc, id asc), padded with id -1 / score -inf."""
    W, B, _ = ps.shape
    ids = np.full((B, k), -1, dtype=np.int32)
    sc = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        s, i = ps[:, b].ravel().astype(np.float64), pi[:, b].ravel().astype(np.int64)
        keep = (i >= 0) & (i != 0x7FFFFFFF)
        s, i = s[keep], i[keep]
        o = np.lexsort((i, -s))[:k]
        ids[b, :len(o)], sc[b, :len(o)] = i[o], s[o]
    return ids, sc
