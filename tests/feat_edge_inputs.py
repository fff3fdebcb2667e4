"""Event sets aimed at the sizes the feature-table kernels branch on (tests/test_feat_edge_inputs_cpu.py asserts what
each one claims, tests/test_feat_edges_gpu.py runs them on the device). Plain NumPy. Every generator returns its arrays
and a dict of the facts it claims.

Aid-table and session-table cases return (aid int32, ts int32, type uint8, sess_off int64, n_aids, facts)."""
import datetime

import numpy as np

import feat_inputs as fi

SPAN_AIDS = 16384            # aids (or sessions) one launch of the per-aid (per-session) kernel covers without its stride loop
HOT = 1024                   # an aid segment above this gets a workgroup
SORT_TILE, SORT_SPAN = 4096, 16384
RANKED = 13
MAX_SESSION = 512


def _ts_of(date, seconds=0):
    """ts whose reference clock (ts + 2 h) reads `seconds` after midnight of `date`."""
    return (date.toordinal() - datetime.date(1970, 1, 1).toordinal()) * 86400 - 7200 + seconds


# ---------------------------------------------------------------------------------------------------------------------
# aid table
# ---------------------------------------------------------------------------------------------------------------------
def stride():
    """16,391 aids (4 * 4096 workgroups' worth plus 7), most with 0 to 2 events, so the per-aid kernel takes its stride
    loop, the event sort crosses a workgroup span and the rank sort crosses 13 of them."""
    n_aids = SPAN_AIDS + 4 + 3
    rng = np.random.default_rng(41)
    counts = rng.integers(0, 3, n_aids)
    counts[0] = 0
    counts[-5:] = 0
    counts[SPAN_AIDS - 1:SPAN_AIDS + 2] = (3, 4, 5)
    counts[777], counts[9000] = HOT, HOT + 1
    aid, ts, typ, off, _ = fi.events(counts.tolist(), 28, seed=42, n_aids=n_aids)
    facts = {'counts': counts, 'absent': np.flatnonzero(counts == 0), 'hot': [9000], 'at_1024': 777,
             'around_the_span': {SPAN_AIDS - 1: 3, SPAN_AIDS: 4, SPAN_AIDS + 1: 5}}
    return aid, ts, typ, off, n_aids, facts


def stride_bad_aid():
    """`stride` with one event's aid equal to n_aids."""
    aid, ts, typ, off, n_aids, facts = stride()
    aid = aid.copy()
    aid[len(aid) // 2] = n_aids
    return aid, ts, typ, off, n_aids, facts


def hot_stride():
    """1,026 aids of 1,025 events (more hot aids than the hot kernel has workgroups) and five cold ones."""
    counts = [3, 0] + [HOT + 1] * 1026 + [1, 64, HOT, 0, 2]
    aid, ts, typ, off, n_aids = fi.events(counts, 14, seed=43, max_len=40)
    counts = np.asarray(counts)
    return aid, ts, typ, off, n_aids, {'counts': counts, 'absent': np.flatnonzero(counts == 0), 'n_hot': 1026}


def hot_edges():
    """Segments on both sides of the hot threshold and of a whole number of chunks per wave of the hot kernel. 4 * 64 * 4
    is 1,024, the largest one-wave segment, so the hot segments whose four waves get the same number of full chunks are
    4 * 64 * 8 and, with one partial chunk more, that plus 1."""
    sizes = [HOT - 1, HOT, HOT + 1, 4 * 64 * 4, 4 * 64 * 4 + 1, HOT + 1 + 63, 4 * 64 * 8, 4 * 64 * 8 + 1]
    counts = [0] + sizes + [1, 2, 2, 65, 0, 7, 0]
    aid, ts, typ, off, n_aids = fi.events(counts, 21, seed=44, max_len=30)
    counts = np.asarray(counts)
    return aid, ts, typ, off, n_aids, {'counts': counts, 'sizes': sizes, 'absent': np.flatnonzero(counts == 0),
                                       'n_hot': sum(s > HOT for s in sizes)}


RUN_COLD, RUN_HOT = 0, 1     # the two aids of `runs`; aids 2 .. 8 are filler
# start position in the aid's segment -> (length, name); every other position is a run of one event
_RUNS = {60: (11, 'straddle'), 128: (64, 'sixty_four'), 192: (2, 'head_lane_0'), 255: (3, 'head_lane_63'), 320: (200, 'types'),
         520: (150, 'last_week')}
_CART_AT, _ORDER_AT = 130, 199                       # positions inside the run 'types'


def sessions_per_aid(aid, typ, off, n_aids):
    """int64 [n_aids, 4]: the distinct sessions of every aid, and those in which it has a click, a cart, an order."""
    sess = np.repeat(np.arange(len(off) - 1), np.diff(off))
    out = np.zeros((n_aids, 4), dtype=np.int64)
    out[:, 0] = np.bincount(np.unique(np.stack([aid, sess]), axis=1)[0], minlength=n_aids)
    for k in range(3):
        out[:, 1 + k] = np.bincount(np.unique(np.stack([aid[typ == k], sess[typ == k]]), axis=1)[0], minlength=n_aids)
    return out


def _run_list(total):
    """[(start, length, name)] covering [0, total): the runs of _RUNS, a run of three before the end, a single event last."""
    special = dict(_RUNS)
    special[total - 4] = (3, 'before_last')
    runs, p = [], 0
    while p < total:
        length, name = special.get(p, (1, 'last' if p == total - 1 else ''))
        runs.append((p, length, name))
        p += length
    assert p == total
    return runs


def runs():
    """Hand-built: a cold aid (1,000 events) and a hot one (1,300), both with the same-session runs of _RUNS at the same
    positions of their segments. Session k holds run k of both aids, interleaved, and sometimes a filler event. Days 0
    (week 30) and 1 .. 7 (week 31) hold everything except some single events and the last events of the run 'last_week',
    which fall on day 8 (week 32, the last week). Aids 9 and up are the shadows explained below."""
    rng = np.random.default_rng(45)
    lists = {RUN_COLD: _run_list(1000), RUN_HOT: _run_list(1300)}
    n_sess = max(len(v) for v in lists.values())
    aid, ts, typ, lens = [], [], [], []
    for k in range(n_sess):
        mine = {a: lists[a][k] for a in lists if k < len(lists[a])}
        name = next(iter(mine.values()))[2] if len({v[2] for v in mine.values()}) == 1 else ''
        longest = max(v[1] for v in mine.values())
        ev = []                                       # (aid, position inside its run)
        for j in range(longest):
            ev += [(a, j) for a, v in mine.items() if j < v[1]]
        if k % 3 == 0 and name != 'last_week':
            ev.insert(int(rng.integers(0, len(ev) + 1)), (2 + k % 7, -1))
        n = len(ev)
        if name == 'last_week':
            day = np.full(n, 7)
            day[-len(mine):] = 8                     # the last event of the run of either aid, and nothing else of it
        elif name == 'types' or longest > 1:
            day = np.full(n, int(rng.integers(0, 8)))
        else:
            day = np.full(n, int(rng.integers(0, 9)))          # single events reach the last week too
        t = fi.SUNDAY + day * 86400 + np.sort(rng.choice(86400, n, replace=False))
        if name == 'types':
            ty = [1 if j == _CART_AT else 2 if j == _ORDER_AT else 0 for _, j in ev]
        elif name == 'straddle':                     # its only order is its last event, behind the chunk edge
            ty = [2 if j == 10 else 0 for _, j in ev]
        elif name == 'head_lane_63':                 # click on lane 63, then a cart and an order in the next chunk
            ty = [max(j, 0) for _, j in ev]
        else:
            ty = rng.choice(3, n, p=[0.7, 0.2, 0.1]).tolist()
        aid += [a for a, _ in ev]
        ts += t.tolist()
        typ += ty
        lens.append(n)
    # The aid table shows an aid's session counts only as ranks, and a rank moves only when a count passes another aid's.
    # So every session count of the two aids gets a shadow aid one below it and one above it, in sessions of their own.
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    per = sessions_per_aid(np.asarray(aid), np.asarray(typ), off, 9)
    shadows = []                                      # (sessions, type) per shadow aid 9, 10, ...
    for a in (RUN_COLD, RUN_HOT):
        shadows += [(int(per[a, 0]) + d, 0) for d in (-1, 1)]
        shadows += [(int(per[a, 1 + k]) + d, k) for k in range(3) for d in (-1, 1)]
    for j in range(max(m for m, _ in shadows)):
        mine = [(9 + i, k) for i, (m, k) in enumerate(shadows) if j < m]
        t = fi.SUNDAY + int(rng.integers(0, 8)) * 86400 + np.sort(rng.choice(86400, len(mine), replace=False))
        aid += [a for a, _ in mine]
        typ += [k for _, k in mine]
        ts += t.tolist()
        lens.append(len(mine))
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    facts = {'runs': {a: {name: (start, length) for start, length, name in v if name} for a, v in lists.items()},
             'cart_at': _CART_AT, 'order_at': _ORDER_AT, 'totals': {RUN_COLD: 1000, RUN_HOT: 1300}, 'shadows': shadows}
    return np.asarray(aid, np.int32), np.asarray(ts, np.int32), np.asarray(typ, np.uint8), off, 9 + len(shadows), facts


WEEK_FIRST = ((0, 50), (1023, 2), (1024, 52), (1025, 48), (3100, 1), (3500, 51), (3900, 49))      # (event index, ISO week)


def weeks():
    """Hand-built ts over 30 Nov 2022 .. 15 Jan 2023: ISO weeks 48 .. 52, 1, 2. The weeks first appear at the event
    indices of WEEK_FIRST, on both sides of the 1,024-event edge of the prep kernel's workgroups and far behind it, in an
    order that is not the calendar's; week 52, the maximum and so the reference's "last week", is the third slot."""
    rng = np.random.default_rng(46)
    n = 4200
    monday = {48: datetime.date(2022, 11, 28), 49: datetime.date(2022, 12, 5), 50: datetime.date(2022, 12, 12),
              51: datetime.date(2022, 12, 19), 52: datetime.date(2022, 12, 26), 1: datetime.date(2023, 1, 2), 2: datetime.date(2023, 1, 9)}
    first = dict(WEEK_FIRST)
    week = np.zeros(n, dtype=np.int64)
    ts = np.zeros(n, dtype=np.int64)
    lens, allowed, i = [], [], 0
    while i < n:
        if i in first:
            allowed.append(first[i])
        stop = min([j for j in first if j > i] + [n])                  # a session ends where a new week has to appear
        m = min(int(rng.integers(1, 12)), stop - i)
        w = first[i] if i in first else allowed[int(rng.integers(0, len(allowed)))]
        d0 = 2 if w == 48 else 0                                       # week 48 starts on Wednesday 30 Nov here
        day = monday[w] + datetime.timedelta(days=int(rng.integers(d0, 7)))
        week[i:i + m] = w
        ts[i:i + m] = _ts_of(day) + np.sort(rng.choice(86400, m, replace=False))
        lens.append(m)
        i += m
    # the two ends of the span are present: 30 Nov and 15 Jan
    ts[1025] = _ts_of(datetime.date(2022, 11, 30), 5)
    ts[1023] = _ts_of(datetime.date(2023, 1, 15), 86399)
    aid = rng.integers(0, 30, n).astype(np.int64)
    typ = rng.choice(3, n, p=[0.6, 0.25, 0.15]).astype(np.int64)

    def take(a, w, count, ty=None):
        free = np.flatnonzero((week == w) & (aid < 30))
        pick = rng.choice(free, count, replace=False)
        aid[pick] = a
        if ty is not None:
            typ[pick] = ty

    take(30, 52, 5)                                                    # week 52 only
    take(31, 1, 3), take(31, 2, 3)                                     # weeks 1 and 2 only: no last-week row
    take(32, 1, 4, 0), take(32, 49, 3, 0)                              # clicks in slots 4 and 6, none in 5: -1, then inf -> NaN
    take(33, 50, 4, 1), take(33, 2, 2, 1), take(33, 48, 3, 1), take(33, 1, 2, 1)   # carts in slots 0, 1, 3, 4: a zero in slot 2
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    facts = {'slots': [w for _, w in WEEK_FIRST], 'first': [i for i, _ in WEEK_FIRST], 'only_52': 30, 'only_1_2': 31,
             'inf_last': 32, 'zero_inside': 33}
    return aid.astype(np.int32), ts.astype(np.int32), typ.astype(np.uint8), off, 36, facts


def tiny():
    """[(aid, ts, type, sess_off, n_aids, facts)]: one aid with one event; three aids and no event at all; five aids with
    events for aid 2 only, between empty sessions."""
    one = (np.array([0], np.int32), np.array([fi.SUNDAY + 5], np.int32), np.array([1], np.uint8), np.array([0, 1], np.int64), 1, {})
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.array([0], np.int64), 3, {})
    only_2 = (np.full(5, 2, np.int32), (fi.SUNDAY + 86400 * np.array([0, 1, 1, 2, 9])).astype(np.int32), np.array([0, 0, 2, 1, 0], np.uint8),
              np.array([0, 0, 3, 3, 5, 5], np.int64), 5, {})
    return [one, none, only_2]


# ---------------------------------------------------------------------------------------------------------------------
# session table: (aid, ts, type, sess_off, n_aids of the aid table, facts)
# ---------------------------------------------------------------------------------------------------------------------
def _session_events(rng, aids_of, n_days=20):
    """Events of sessions whose aids are given per session."""
    lens = [len(a) for a in aids_of]
    n = sum(lens)
    aid = np.concatenate([np.asarray(a, np.int64) for a in aids_of] + [np.zeros(0, np.int64)])
    ts = np.concatenate([fi.SUNDAY + int(rng.integers(0, n_days)) * 86400 + np.sort(rng.choice(86400, m, replace=False)) for m in lens]
                        + [np.zeros(0, np.int64)])
    typ = rng.choice(3, n, p=[0.8, 0.15, 0.05])
    return aid.astype(np.int32), ts.astype(np.int32), typ.astype(np.uint8), np.r_[0, np.cumsum(lens)].astype(np.int64)


def sess_stride():
    """16,390 sessions of 0 to 3 events over the aids of `stride` (absent ones included)."""
    rng = np.random.default_rng(47)
    n_sess, n_aids = SPAN_AIDS + 4 + 2, SPAN_AIDS + 4 + 3
    lens = rng.integers(0, 4, n_sess)
    empty = [0, n_sess - 1, 100, 101, SPAN_AIDS - 1, SPAN_AIDS]
    lens[empty] = 0
    lens[[1, 99, 102, SPAN_AIDS - 2, SPAN_AIDS + 1, n_sess - 2]] = (1, 2, 3, 3, 2, 1)
    aid, ts, typ, off = _session_events(rng, [rng.integers(0, n_aids, m) for m in lens])
    return aid, ts, typ, off, n_aids, {'lens': lens, 'empty': empty}


SESS_TABLE_AIDS, SESS_TABLE_PRESENT = 600, 500       # `sess_lengths`: aids 500 .. 599 have no row in the aid table


def sess_table_events():
    """The smaller event set the aid table of `sess_lengths` is made from: aids 0 .. 499 only."""
    rng = np.random.default_rng(48)
    counts = rng.integers(1, 5, SESS_TABLE_PRESENT).tolist() + [0] * (SESS_TABLE_AIDS - SESS_TABLE_PRESENT)
    return fi.events(counts, 14, seed=49)


def sess_lengths():
    """Sessions at every chunk edge of the session kernel and at its LDS capacity, distinct-aid counts around the uint8
    wrap, and aids whose aid-table row is all NaN."""
    rng = np.random.default_rng(50)
    P, A = SESS_TABLE_PRESENT, SESS_TABLE_AIDS
    aids_of, facts = [], {'lens': [], 'distinct': {}}
    for m in (0, 1, 63, 64, 65, 127, 128, 129, 511, 512):
        aids_of.append(rng.integers(0, P, m))
        facts['lens'].append(m)
    for d in (255, 256, 257):                        # 300 events of exactly d distinct aids
        base = rng.permutation(A)[:d]
        facts['distinct'][len(aids_of)] = d
        aids_of.append(rng.permutation(np.r_[base, rng.choice(base, 300 - d)]))
    facts['distinct'][len(aids_of)] = 512
    aids_of.append(rng.permutation(A)[:512])
    facts['distinct'][len(aids_of)] = 1
    aids_of.append(np.full(512, 17))
    facts['all_nan'] = len(aids_of)
    aids_of.append(rng.integers(P, A, 10))
    facts['nan_last'] = len(aids_of)
    aids_of.append(np.r_[rng.integers(0, P, 9), P + 50])
    aids_of.append(np.zeros(0, np.int64))
    aid, ts, typ, off = _session_events(rng, aids_of, n_days=14)
    return aid, ts, typ, off, A, facts


def sess_errors():
    """{name: (aid, ts, type, sess_off, n_aids of the table)}: a session of 513 events; an aid equal to n_aids."""
    rng = np.random.default_rng(51)
    P, A = SESS_TABLE_PRESENT, SESS_TABLE_AIDS
    long = _session_events(rng, [rng.integers(0, P, 3), rng.integers(0, P, MAX_SESSION + 1), rng.integers(0, P, 2)])
    beyond = [rng.integers(0, P, 3), rng.integers(0, P, 70)]
    beyond[1][66] = A
    return {'too_long': long + (A,), 'aid_beyond_the_table': _session_events(rng, beyond) + (A,)}


# ---------------------------------------------------------------------------------------------------------------------
# matrix
# ---------------------------------------------------------------------------------------------------------------------
MATRIX_ROWS = (255, 256, 257, 512, 513)
MATRIX_F = (1, 2, 3, 4, 32, 63, 64)
BIG_SESSIONS = (0, 256, 0, 600, 1, 255, 0, 0, 257, 0)
MATRIX_AIDS = 997


def matrix_pairs():
    """(n_rows, F) pairs: every F with two row counts and every row count with two or three F, not the full product."""
    return [(MATRIX_ROWS[(i + j) % len(MATRIX_ROWS)], F) for i, F in enumerate(MATRIX_F) for j in (0, 2)]


def matrix_sizes(n_rows):
    """Session sizes below 130 that add up to n_rows, empty sessions at both ends and inside (as tests/test_feat_gpu.py)."""
    rng = np.random.default_rng(200 + n_rows)
    sizes = []
    while sum(sizes) < n_rows:
        sizes.append(min(int(rng.integers(0, 130)), n_rows - sum(sizes)))
    sizes = [0] + sizes + [0, 0]
    sizes.insert(3, 0)
    return sizes


def matrix_case(sizes, F, seed):
    """(inputs of test_feat_gpu._matrix_inputs, F column names drawn from every column there is)."""
    from test_feat_gpu import _all_names, _matrix_inputs
    rng = np.random.default_rng(seed)
    m = _matrix_inputs(rng, list(sizes), n_aids=MATRIX_AIDS)
    return m, rng.permutation(_all_names())[:F].tolist()
