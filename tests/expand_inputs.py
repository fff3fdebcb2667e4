"""Windows aimed at every branch of the covisitation pair-expand (``k_expand_lists`` and ``k_expand<G,TIME,FILT>`` in
``csrc/otto_covis.hip``), shared by tests/test_expand_inputs_cpu.py (which proves that every window is of the kind its
entry claims) and tests/test_covis_expand_edges_gpu.py (which compares the device records with the oracle, window by
window). Plain NumPy, seeded; nothing here touches a device.

``classify`` restates the scheme of DESIGN.md section 2, row "K1 ``k_expand_lists``", from its TEXT: which windows are
cliques, which share component lists, which aids take a private row, which windows take the general row loop. A pull
request that changes that scheme changes section 2 and ``classify`` together.

A window is ``(aids, ts, types)`` of n <= 32 events; the lane group that runs it is G = 8 (n <= 8), 16 (n <= 16) or 32.
"""
import zlib
from dataclasses import dataclass

import numpy as np

from otto_amd.synth import Events

T0 = 1_660_000_000
TS_MAX = 2 ** 31 - 1
GAP = 86400                      # the default max_gap; the library also holds windows for max_gap 0 and 2^31 - 1
N_AIDS = 1024
KINDS = ('clique', 'lists', 'private', 'general')
WPW = {8: 8, 16: 4, 32: 2}       # windows per wave of a lane-group size


def lane_group(n):
    """Lanes per window of a window of n events (None: no window, the session has fewer than two events)."""
    return None if n < 2 else (8 if n <= 8 else (16 if n <= 16 else 32))


# ---------------------------------------------------------------------------------------------------------------------
# classifier
# ---------------------------------------------------------------------------------------------------------------------
def _analyse(aid, ts, max_gap):
    aid = [int(a) for a in aid]
    ts = [int(t) for t in ts]
    n = len(aid)
    comps, descends = [], False
    for i in range(n):
        step = ts[i] - ts[i - 1] if i else 0
        descends |= step < 0
        if i == 0 or step < 0 or step > max_gap:
            comps.append([])
        comps[-1].append(i)
    wide = any(ts[c[-1]] - ts[c[0]] > max_gap for c in comps)
    if descends or wide:
        pairs = {(aid[i], aid[j]) for i in range(n) for j in range(n)
                 if aid[i] != aid[j] and abs(ts[i] - ts[j]) <= max_gap}
        return dict(kind='general', shared_runs=0, row_records=len(pairs), list_words=0, pairs=len(pairs), rows=[], comps=comps)
    shared = records = words = pairs = 0
    rows = []                                        # (component, x, records) of every private row
    held = []                                        # distinct aids of the earlier components
    for ci, c in enumerate(comps):
        D = list(dict.fromkeys(aid[i] for i in c))   # first-occurrence order
        words += len(D)
        for x in D:
            met = set().union(*[h for h in held if x in h]) if held else set()
            if any(y != x and y in met for y in D):
                r = sum(1 for y in D if y != x and y not in met)
                rows.append((ci, x, r))
                records += r
                pairs += r
            elif len(D) > 1:
                shared += 1
                pairs += len(D) - 1
        held.append(set(D))
    kind = 'clique' if len(comps) == 1 else ('private' if rows else 'lists')
    return dict(kind=kind, shared_runs=shared, row_records=records, list_words=words, pairs=pairs, rows=rows, comps=comps)


def classify(aid, ts, max_gap):
    """(kind, shared_runs, row_records, list_words) of one window under the component-list scheme."""
    a = _analyse(aid, ts, max_gap)
    return a['kind'], a['shared_runs'], a['row_records'], a['list_words']


def pair_count(aid, ts, max_gap):
    """Deduped ordered pairs of the window as the scheme counts them: list entries minus the run's own, plus row records."""
    return _analyse(aid, ts, max_gap)['pairs']


def private_rows(aid, ts, max_gap):
    """[(component, x, records)] of the window's private rows (empty for a general window)."""
    return _analyse(aid, ts, max_gap)['rows']


# ---------------------------------------------------------------------------------------------------------------------
# window library
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One window. `kind` is the claim that test_expand_inputs_cpu.py checks with `classify`. `prefix`: events of the session
    in front of the window ('W+1' / '3W': the session has that many events, so the window must have exactly W = `only_window`)."""
    name: str
    aids: np.ndarray
    ts: np.ndarray
    types: np.ndarray
    max_gap: int
    kind: str
    prefix: object = None
    only_window: object = None

    @property
    def n(self):
        return len(self.aids)

    @property
    def G(self):
        return lane_group(self.n)

    def fits(self, window):
        return self.n <= window if self.only_window is None else window == self.only_window


def _types(name, n):
    return np.random.default_rng(zlib.crc32(name.encode())).integers(0, 3, n).astype(np.uint8)


def _fresh(k, start):
    return list(range(start, start + k))


def _case(name, kind, aids, ts, g, types=None, **kw):
    aids = np.asarray(aids, dtype=np.int64)
    ts = np.asarray(ts, dtype=np.int64)
    assert len(aids) == len(ts) and 1 <= len(aids) <= 32 and ts.min() >= 0 and ts.max() <= TS_MAX, name
    assert aids.min() >= 0 and aids.max() < N_AIDS, name
    types = _types(name, len(aids)) if types is None else np.asarray(types, dtype=np.uint8)
    assert len(types) == len(aids)
    return Case(name, aids.astype(np.uint32), ts.astype(np.int32), types, int(g), kind, **kw)


def _comps(name, kind, comps, g, step=1, t0=T0, types=None, **kw):
    """Components `comps` (lists of aids) `g + 1` apart, the events of one `step` apart (the span stays within g)."""
    aids, ts, t = [], [], t0
    for ci, c in enumerate(comps):
        if ci:
            t += g + 1
        assert step * (len(c) - 1) <= g, name
        for k, a in enumerate(c):
            if k:
                t += step
            aids.append(a)
            ts.append(t)
    return _case(name, kind, aids, ts, g, types, **kw)


def _split(n, parts):
    q, r = divmod(n, parts)
    return [q + (1 if i < r else 0) for i in range(parts)]


def _build_library():
    lib = {}

    def add(c):
        assert c.name not in lib, c.name
        lib[c.name] = c

    g = GAP
    # ---- sizes: a gap-free clique of distinct aids and one with repeats (n = 2 with repeats: two equal aids, no pair)
    for n in (2, 7, 8, 9, 15, 16, 17, 30, 31, 32):
        add(_comps(f'clique-distinct-n{n}', 'clique', [_fresh(n, 1)], g))
        d = max(1, n // 2)
        add(_comps(f'clique-repeats-n{n}', 'clique', [[1 + i % d for i in range(n)]], g))
    # a session of W + 1 and of 3 W events: only the tail of W events takes part. The events in front hold the tail's aids
    # with other types, seconds before the tail: an expand that starts at the session's first event gets other records
    for W in (30, 32):
        tail = lib[f'clique-repeats-n{W}']
        for tag in ('W+1', '3W'):
            add(Case(f'long-{tag}-w{W}', tail.aids, tail.ts, tail.types, g, 'clique', prefix=tag, only_window=W))
    add(_comps('list-len32-sp31', 'clique', [[0, N_AIDS - 1] + _fresh(30, 40)], g))

    for G, n in ((8, 8), (16, 16), (32, 30)):
        s = f'-G{G}'
        h = n // 2
        # ---- no pairs
        add(_comps('one-aid' + s, 'clique', [[5] * n], g))
        add(_comps('all-singletons' + s, 'lists', [[a] for a in _fresh(n - 2, 1) + [1, 2]], g))
        # ---- gap edges
        add(_case('span-eq-g' + s, 'clique', _fresh(n, 1), [T0] + [T0 + 1 + i for i in range(n - 2)] + [T0 + g], g))
        add(_case('span-g+1' + s, 'general', _fresh(n, 1), [T0] + [T0 + 1 + i for i in range(n - 2)] + [T0 + g + 1], g))
        add(_case('step-eq-g' + s, 'clique', _fresh(n, 1), [T0] * h + [T0 + g] * (n - h), g))
        add(_case('step-g+1' + s, 'lists', _fresh(n, 1), [T0] * h + [T0 + g + 1] * (n - h), g))
        add(_case('extremes' + s, 'lists', _fresh(n, 1), [0] * h + [TS_MAX] * (n - h), g))
        add(_case('extremes-descending' + s, 'general', _fresh(n, 1), [TS_MAX] * h + [0] * (n - h), g))
        # ---- lists
        add(_comps('two-comps' + s, 'lists', [_fresh(h - 1, 1) + [1], [50] + _fresh(n - h - 1, 50)], g))
        five, a0 = [], 1
        for k in _split(n, 5):
            five.append(_fresh(k, a0))
            a0 += k
        add(_comps('five-comps' + s, 'lists', five, g))
        add(_comps('singleton-between' + s, 'lists', [_fresh(h - 1, 1), [70], _fresh(n - h, 80)], g))
        add(_comps('new-partners' + s, 'lists', [[1] + _fresh(h - 1, 10), [1] + _fresh(n - h - 1, 60)], g))
        add(_comps('comp-type' + s, 'lists', [[1], [2, 2, 1, 2] + _fresh(n - 5, 20)], g,
                   types=[0, 1, 2, 1, 0] + list(_types('comp-type' + s, n - 5))))
        add(_comps('sp-first-mid-last' + s, 'lists', [_fresh(2, 90), _fresh(n - 2, 1)], g))
        # ---- private rows
        add(_comps('repeated-partner' + s, 'private', [[1, 2, 3] + _fresh(h - 3, 10), [1, 2, 4] + _fresh(n - h - 3, 60)], g))
        add(_comps('private-empty' + s, 'private', [_fresh(h, 1), _fresh(h, 1)[::-1] if G > 8 else _fresh(h, 1)], g))
        q = _split(n - 8, 3)
        add(_comps('three-comps' + s, 'private', [[1, 2] + _fresh(q[0], 10), [1, 3] + _fresh(q[1], 40), [1, 2, 3, 4] + _fresh(q[2], 70)], g))
        add(_comps('four-private' + s, 'private', [[1, 2, 3, 4], [1, 2, 3, 4, 5] + _fresh(n - 9, 10)], g) if n > 8 else
            _comps('four-private' + s, 'private', [[1, 2, 3, 4], [1, 2, 3, 4]], g))
        add(_comps('shared-before-private' + s, 'private', [[1, 2], [5, 1, 2, 6] + _fresh(n - 6, 10)], g))
        add(_comps('private-then-new' + s, 'private', [[1, 2], [1, 2, 3], [3] + _fresh(n - 6, 10)], g))
        # ---- general
        m = n - 4
        add(_case('no-cut-at-gap' + s, 'general', _fresh(n, 1), [T0, T0 + 1, T0 + g + 1] + [T0 + g + 2] * (m + 1), g))
        add(_case('nonclique-then-clique' + s, 'general', _fresh(n, 1),
                  [T0, T0 + g, T0 + 2 * g] + [T0 + 3 * g + 1 + i for i in range(n - 3)], g))
        # repeats of x and of y: the first valid (i, j) of (1, 2) is (3, 2), that of (2, 1) is (2, 3); 1 and 2 meet again later
        add(_case('general-repeats' + s, 'general', [1, 5, 2, 1, 2, 1] + _fresh(n - 6, 10),
                  [T0, T0 + g, T0 + 2 * g, T0 + 2 * g, T0 + 2 * g + 1, T0 + 2 * g + 2] + [T0 + 3 * g] * (n - 6), g,
                  types=[0, 1, 2, 1, 0, 2] + list(_types('general-repeats' + s, n - 6))))
        band = g // 4
        add(_case('general-band' + s, 'general', [1 + i % (n - 2) for i in range(n)], [T0 + i * band for i in range(n)], g))
        asc = [T0 + 10 * i for i in range(n)]
        for tag, p in (('1', 1), ('mid', h), ('last', n - 1)):
            t = list(asc)
            t[p] = t[p - 1] - 5
            add(_case(f'descending-{tag}' + s, 'general', [1 + i % (n - 1) for i in range(n)], t, g))
        add(_case('reversed' + s, 'general', [1 + i % (n - 1) for i in range(n)], asc[::-1], g))
        add(_case('reversed-wide' + s, 'general', _fresh(n, 1), [T0 + i * band for i in range(n)][::-1], g))
        # ---- filter kinds: per mask a pair (1, 2) whose first valid (i, j) fails while a later one passes; a pair (1, 2) whose
        # only passing (i, j) is not valid (more than g apart); all nine (type_x, type_y) cells
        pad, tpad = _fresh(n - 4, 10), [T0 + 3] * (n - 4)
        for mask, ty in (('click_cart', [1, 0, 0, 1]), ('click_order', [1, 0, 0, 2]), ('cart_order', [0, 0, 1, 2]), ('click_click', [1, 1, 0, 0])):
            add(_case(f'filter-later-{mask}' + s, 'clique', [1, 2, 1, 2] + pad, [T0, T0 + 1, T0 + 2, T0 + 3] + tpad, g,
                      types=ty + [i % 3 for i in range(n - 4)]))
        add(_case('filter-pass-not-valid' + s, 'private', [1, 2, 2, 1] + pad, [T0, T0, T0 + g + 1, T0 + g + 1] + [T0 + g + 1] * (n - 4), g,
                  types=[0, 0, 1, 1] + [2] * (n - 4)))
        add(_comps('filter-nine-cells' + s, 'clique', [_fresh(n, 1)], g, types=[i % 3 for i in range(n)]))

    # ---- n = 32: the general loop and the largest private rows. A private row needs x and a partner twice, so it holds at
    # most 32 - 4 = 28 records; a row of hits only is largest with two equal components of 16
    add(_case('general-n32', 'general', _fresh(32, 1), [T0 + i * (g // 4) for i in range(32)], g))
    add(_case('general-n32-all-pairs-but-one', 'general', _fresh(32, 1), [T0] + [T0 + 1] * 30 + [T0 + g + 1], g))
    add(_case('reversed-n32', 'general', [1 + i % 29 for i in range(32)], [T0 + 5 * (32 - i) for i in range(32)], g))
    add(_case('descending-last-n32', 'general', _fresh(32, 1), [T0 + i for i in range(31)] + [T0], g))
    add(_comps('private-28-records-n32', 'private', [[1, 2], [1, 2] + _fresh(28, 10)], g))
    add(_comps('private-15-hits-n32', 'private', [_fresh(16, 1), _fresh(16, 1)[::-1]], g))
    add(_comps('private-14-hits-2-records-n32', 'private', [_fresh(15, 1), [40] + _fresh(15, 1) + [41]], g))
    add(_comps('three-comps-n32', 'private', [[1, 2] + _fresh(8, 10), [1, 3] + _fresh(8, 40), [1, 2, 3, 4] + _fresh(8, 70)], g))
    add(_comps('five-comps-n32', 'lists', [_fresh(7, 1), _fresh(6, 10), [1] + _fresh(6, 20), _fresh(6, 30), _fresh(6, 40)], g))

    # ---- the four cases of the table in DESIGN.md section 4, as written there
    add(_comps('repeated-partner', 'private', [[1, 2, 3], [1, 2, 4]], g))
    add(_comps('private-empty', 'private', [[1, 2], [1, 2]], g))
    add(_comps('three-comps', 'private', [[1, 2], [1, 3], [1, 2, 3, 4]], g))
    add(_case('no-cut-at-gap', 'general', [1, 2, 3, 4], [T0, T0 + 1, T0 + 1 + g, T0 + 2 + g], g))
    add(_comps('n2-equal', 'clique', [[9, 9]], g))
    add(_comps('n2-cut', 'lists', [[1], [2]], g))

    # ---- max_gap = 0: blocks of equal stamps are the components; max_gap = 2^31 - 1: nothing ascending is ever cut
    for G, n in ((8, 8), (16, 16), (32, 30)):
        s = f'-G{G}'
        h = n // 2
        add(_comps('gap0-one-block' + s, 'clique', [[1 + i % (n - 1) for i in range(n)]], 0, step=0, t0=5))
        add(_comps('gap0-blocks' + s, 'private', [[1, 2, 3], [1, 2, 4], [5]] + [_fresh(n - 7, 10)], 0, step=0, t0=0))
        add(_comps('gap0-lists' + s, 'lists', [_fresh(h, 1), _fresh(n - h, 40)], 0, step=0, t0=TS_MAX - 1))
        add(_case('gap0-descending' + s, 'general', _fresh(n, 1), [9] * h + [8] * (n - h), 0))
        add(_case('gapmax-extremes' + s, 'clique', [1 + i % (n - 1) for i in range(n)], [0] + [T0 + i for i in range(n - 2)] + [TS_MAX], TS_MAX))
        add(_case('gapmax-descending' + s, 'general', _fresh(n, 1), [TS_MAX] + [0] * (n - 2) + [TS_MAX], TS_MAX))
        add(_comps('gap0-all-singletons' + s, 'lists', [[a] for a in _fresh(n - 2, 1) + [1, 2]], 0, t0=7))
    return lib


LIBRARY = _build_library()


def names(max_gap=GAP, window=32, G=None, kind=None):
    """Library entries of one max_gap that fit the window, in library order."""
    return [c.name for c in LIBRARY.values() if c.max_gap == max_gap and c.fits(window)
            and (G is None or c.G == G) and (kind is None or c.kind == kind)]


# ---------------------------------------------------------------------------------------------------------------------
# stream composer
# ---------------------------------------------------------------------------------------------------------------------
EMPTY, SINGLE = '<0>', '<1>'     # sessions of 0 and of 1 event in a list of names


def session_events(name, window):
    """(aid, ts, type) of the whole session of a library entry: the window behind its prefix."""
    if name == EMPTY:
        z = np.zeros(0, np.int64)
        return z.astype(np.uint32), z.astype(np.int32), z.astype(np.uint8)
    if name == SINGLE:
        return np.array([3], np.uint32), np.array([T0], np.int32), np.array([1], np.uint8)
    c = LIBRARY[name]
    assert c.fits(window), f'{name} does not fit window {window}'
    if c.prefix is None:
        return c.aids, c.ts, c.types
    assert c.n == window
    k = {'W+1': window + 1, '3W': 3 * window}[c.prefix] - c.n
    idx = np.arange(k) % c.n
    return (np.r_[c.aids[idx][::-1], c.aids], np.r_[np.full(k, int(c.ts[0]) - 2, np.int32), c.ts],
            np.r_[((c.types[idx] + 1) % 3).astype(np.uint8), c.types])


def stream(name_list, window=32):
    """Concatenate library windows, one session each, into Events."""
    parts = [session_events(nm, window) for nm in name_list]
    off = np.r_[0, np.cumsum([len(p[0]) for p in parts])].astype(np.int64)
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    return Events(cat(0, np.uint32), cat(1, np.int32), cat(2, np.uint8), off, N_AIDS)


def _cycle(pool, k, start=0):
    return [pool[(start + i) % len(pool)] for i in range(k)]


def tile(c8, c16, c32, window, salt=0):
    """64 session names: c8 / c16 / c32 windows of the three lane-group sizes, the rest sessions of 0 and 1 events,
    interleaved (the kernel sorts a tile's sessions by class itself)."""
    assert c8 + c16 + c32 <= 64
    pools = {G: names(GAP, window, G) for G in (8, 16, 32)}
    out = _cycle(pools[8], c8, salt) + _cycle(pools[16], c16, 3 * salt) + _cycle(pools[32], c32, 5 * salt)
    out += [EMPTY if i % 2 else SINGLE for i in range(64 - len(out))]
    order = np.random.default_rng(1000 + salt).permutation(64)
    return [out[i] for i in order]


def tile_mixes():
    """{name: (c8, c16, c32)}: per lane-group size the counts 0, 1, WPW - 1, WPW, WPW + 1 and 64 in a tile of 64 sessions."""
    mixes = {}
    for qi, G in enumerate((8, 16, 32)):
        for k in (0, 1, WPW[G] - 1, WPW[G], WPW[G] + 1, 64):
            cnt = [0, 0, 0]
            cnt[qi] = k
            others = [i for i in range(3) if i != qi]
            if k == 0:                                  # the class is empty, the others and the short sessions share the tile
                cnt[others[0]], cnt[others[1]] = 20, 23
            elif k < 64 and k % 2:                      # odd: one other class only (with k = 1 also the `c == 0` chains)
                cnt[others[qi % 2]] = 9
            elif k < 64:
                cnt[others[0]], cnt[others[1]] = WPW[(8, 16, 32)[others[0]]] + 1, 1
            mixes[f'tile-G{G}-x{k}-is-{cnt[0]}-{cnt[1]}-{cnt[2]}'] = tuple(cnt)
    mixes['tile-only-G32-is-0-0-64'] = (0, 0, 64)
    mixes['tile-G32-after-empty-classes-is-0-0-3'] = (0, 0, 3)
    mixes['tile-G16-only-is-0-5-0'] = (0, 5, 0)
    mixes['tile-short-sessions-only-is-0-0-0'] = (0, 0, 0)
    return mixes


def _private_pairs(window):
    """Private rows in neighbouring windows of one wave step, for every lane-group size: 8 / 4 / 2 windows per step, so a run of
    private windows of one size puts several of them into the same step."""
    out = []
    for G in (8, 16, 32):
        pool = names(GAP, window, G, 'private')
        full = [nm for nm in pool if classify(LIBRARY[nm].aids, LIBRARY[nm].ts, GAP)[2] > 0]       # rows that hold records
        out += _cycle(full, 2 * WPW[G] + 1) + [nm for nm in pool if nm not in full]
    return out


def streams(window=32):
    """{stream name: (session names, max_gap)} of every named stream, a few thousand windows at most each."""
    out = {}
    for g, tag in ((GAP, 'g86400'), (0, 'g0'), (TS_MAX, 'gmax')):
        out[f'library-{tag}'] = (names(g, window), g)
    mixes = tile_mixes()
    seq = []
    for i, cnt in enumerate(mixes.values()):
        seq += tile(*cnt, window, salt=i)
    out['tile-mixes'] = (seq, GAP)
    out['private-neighbours'] = (_private_pairs(window), GAP)
    base = names(GAP, window)
    for n_sess in (1, 63, 64, 65, 257):
        out[f'n-sess-{n_sess}'] = (_cycle(base, n_sess, start=7 * n_sess), GAP)
    return out


CORE_TABLE = {                       # name: (kind, shared runs, row records, list words, pairs)
    'repeated-partner': ('private', 4, 2, 6, 10),
    'private-empty': ('private', 2, 0, 4, 2),
    'three-comps': ('private', 5, 5, 8, 12),
    'no-cut-at-gap': ('general', 0, 6, 0, 6),
}
