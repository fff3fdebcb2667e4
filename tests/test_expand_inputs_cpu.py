"""Every window of ``tests/expand_inputs.py`` is of the kind its entry claims (no GPU needed). tests/test_covis_expand_edges_gpu.py
compares the pair-expand kernels with the oracle on these windows; if a window lost its edge -- a step one second shorter,
a partner that is no longer repeated -- those tests would still pass and prove nothing. The conditions are states of the
INPUTS, so they are checked here, with the classifier written from DESIGN.md section 2 and the oracle's per-window expansion,
never on the device's output."""
import re
from collections import Counter

import numpy as np
import pytest

import covis_oracle as co
import expand_inputs as ei

CASES = list(ei.LIBRARY.values())


def _oracle(c, filter_kinds=()):
    sp = co.CovisSpec(window=32, max_gap=c.max_gap)
    return co.expand_window_python(c.aids, c.ts, c.types, 0, c.n, sp, filter_kinds, 0, 0)


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_entry_is_of_the_kind_it_claims_and_pairs_equal_the_oracle(c):
    kind, shared, rows, words = ei.classify(c.aids, c.ts, c.max_gap)
    assert kind == c.kind
    assert ei.pair_count(c.aids, c.ts, c.max_gap) == len(_oracle(c))
    assert 0 <= int(c.ts.min()) and int(c.ts.max()) <= ei.TS_MAX and c.types.max() <= 2 and c.aids.max() < ei.N_AIDS
    if kind == 'general':
        assert shared == 0 and words == 0 and rows == len(_oracle(c))
    else:
        assert words <= c.n and shared <= words


@pytest.mark.parametrize('name', list(ei.CORE_TABLE))
def test_core_cases_have_the_counts_of_the_table(name):
    c = ei.LIBRARY[name]
    assert ei.classify(c.aids, c.ts, c.max_gap) + (ei.pair_count(c.aids, c.ts, c.max_gap),) == ei.CORE_TABLE[name]
    assert len(_oracle(c)) == ei.CORE_TABLE[name][4]


def test_core_windows_are_the_ones_written_in_the_table():
    L, g = ei.LIBRARY, ei.GAP
    assert L['repeated-partner'].aids.tolist() == [1, 2, 3, 1, 2, 4] and np.diff(L['repeated-partner'].ts).tolist() == [1, 1, g + 1, 1, 1]
    assert L['private-empty'].aids.tolist() == [1, 2, 1, 2] and np.diff(L['private-empty'].ts).tolist() == [1, g + 1, 1]
    assert L['three-comps'].aids.tolist() == [1, 2, 1, 3, 1, 2, 3, 4] and np.diff(L['three-comps'].ts).tolist() == [1, g + 1, 1, g + 1, 1, 1, 1]
    assert L['no-cut-at-gap'].aids.tolist() == [1, 2, 3, 4] and np.diff(L['no-cut-at-gap'].ts).tolist() == [1, g, 1]


def test_library_covers_every_kind_and_lane_group():
    cells = Counter((c.kind, c.G) for c in CASES if c.max_gap == ei.GAP and c.fits(30))
    for kind in ei.KINDS:
        for G in (8, 16, 32):
            assert cells[(kind, G)] >= 3, (kind, G)
    # the other two gaps: every kind that can exist there (nothing ascending is cut at max_gap 2^31 - 1)
    for G in (8, 16, 32):
        assert {c.kind for c in CASES if c.max_gap == 0 and c.G == G} == set(ei.KINDS)
        assert {c.kind for c in CASES if c.max_gap == ei.TS_MAX and c.G == G} == {'clique', 'general'}
    sizes = {c.n for c in CASES}
    assert {2, 7, 8, 9, 15, 16, 17, 30, 31, 32} <= sizes


def _shape(name):
    return re.sub(r'-G(8|16|32)$', '', name)


def test_every_sized_shape_exists_for_all_three_lane_groups():
    by_shape = {}
    for c in CASES:
        if re.search(r'-G(8|16|32)$', c.name):
            by_shape.setdefault(_shape(c.name), set()).add(c.G)
            assert c.G == int(c.name.rsplit('-G', 1)[1]), c.name
    assert len(by_shape) >= 40
    for shape, gs in by_shape.items():
        assert gs == {8, 16, 32}, shape


def test_windows_without_pairs():
    L = ei.LIBRARY
    for name in ('one-aid-G8', 'one-aid-G16', 'one-aid-G32', 'n2-equal', 'clique-repeats-n2', 'n2-cut',
                 'all-singletons-G8', 'all-singletons-G16', 'all-singletons-G32', 'gap0-all-singletons-G16'):
        assert _oracle(L[name]) == [], name
    for G in (8, 16, 32):
        c = L[f'all-singletons-G{G}']
        assert (np.diff(c.ts) == c.max_gap + 1).all() and len(set(c.aids.tolist())) < c.n


def test_gap_edges_sit_on_the_second():
    L, g = ei.LIBRARY, ei.GAP
    for G in (8, 16, 32):
        a, b = L[f'span-eq-g-G{G}'], L[f'span-g+1-G{G}']
        assert a.ts[-1] - a.ts[0] == g and b.ts[-1] - b.ts[0] == g + 1 and np.diff(b.ts).max() <= g
        assert len(_oracle(a)) == a.n * (a.n - 1) and len(_oracle(b)) == b.n * (b.n - 1) - 2
        a, b = L[f'step-eq-g-G{G}'], L[f'step-g+1-G{G}']
        assert np.diff(a.ts).max() == g and np.diff(b.ts).max() == g + 1
        e = L[f'extremes-G{G}']
        assert e.ts.min() == 0 and e.ts.max() == ei.TS_MAX
        e = L[f'gapmax-extremes-G{G}']
        assert e.ts.min() == 0 and e.ts.max() == ei.TS_MAX and e.max_gap == ei.TS_MAX
        e = L[f'gap0-blocks-G{G}']
        assert e.max_gap == 0 and (np.diff(e.ts) >= 0).all() and (np.diff(e.ts) == 0).any()


def test_list_geometry_cases():
    L = ei.LIBRARY
    c = L['list-len32-sp31']
    assert c.n == 32 and len(set(c.aids.tolist())) == 32 and ei.classify(c.aids, c.ts, c.max_gap)[1:] == (32, 0, 32)
    assert 0 in c.aids and ei.N_AIDS - 1 in c.aids
    for G in (8, 16, 32):
        c = L[f'comp-type-G{G}']
        assert c.aids[:5].tolist() == [1, 2, 2, 1, 2] and c.types[:5].tolist() == [0, 1, 2, 1, 0]
        assert c.ts[1] - c.ts[0] > c.max_gap and c.types[3] != c.types[0]
        want = dict(((x, y), ty) for x, y, ty, _, _ in _oracle(c))
        assert want[(2, 1)] == c.types[3] and want[(1, 2)] == c.types[1]
        c = L[f'new-partners-G{G}']                              # x re-occurs, every run stays shared
        k = ei.classify(c.aids, c.ts, c.max_gap)
        assert k[0] == 'lists' and k[1] == k[3] == c.n and (c.aids == 1).sum() == 2
        c = L[f'sp-first-mid-last-G{G}']                         # a second list of at least three entries: sp = 0, mid, len - 1
        assert len(ei._analyse(c.aids, c.ts, c.max_gap)['comps'][1]) >= 3


def test_private_row_cases():
    L = ei.LIBRARY
    rows = lambda name: ei.private_rows(L[name].aids, L[name].ts, L[name].max_gap)
    for G in (8, 16, 32):
        assert all(r == 0 for _, _, r in rows(f'private-empty-G{G}'))
        assert len(rows(f'repeated-partner-G{G}')) == 2 and len(rows(f'four-private-G{G}')) == 4
        assert len({ci for ci, _, _ in rows(f'three-comps-G{G}')}) == 1 and len(rows(f'three-comps-G{G}')) == 3
        c = L[f'shared-before-private-G{G}']
        assert ei.classify(c.aids, c.ts, c.max_gap)[1] >= 3 and len(rows(c.name)) == 2
    assert max(r for _, _, r in rows('private-28-records-n32')) == 28 and L['private-28-records-n32'].n == 32
    assert len(rows('private-15-hits-n32')) == 16 and all(r == 0 for _, _, r in rows('private-15-hits-n32'))
    assert sorted(r for _, _, r in rows('private-14-hits-2-records-n32')) == [2] * 15


def test_general_cases():
    L = ei.LIBRARY
    for G in (8, 16, 32):
        c = L[f'general-repeats-G{G}']
        want = dict(((x, y), (ty, e)) for x, y, ty, _, e in co.expand_window_python(
            c.aids, c.ts, c.types, 0, c.n, co.CovisSpec(window=32, max_gap=c.max_gap), (), int(c.ts.min()), int(c.ts.max())))
        first = lambda t: (3 * co.Q16 * (int(t) - int(c.ts.min()))) // int(c.ts.max() - c.ts.min())
        assert want[(1, 2)] == (c.types[2], first(c.ts[3])) and first(c.ts[3]) != first(c.ts[0])
        assert want[(2, 1)] == (c.types[3], first(c.ts[2])) and c.types[3] != c.types[0]
        for tag, p in (('1', 1), ('mid', c.n // 2), ('last', c.n - 1)):
            d = L[f'descending-{tag}-G{G}']
            assert np.flatnonzero(np.diff(d.ts) < 0).tolist() == [p - 1]
        assert (np.diff(L[f'reversed-G{G}'].ts) < 0).all()
        c = L[f'nonclique-then-clique-G{G}']
        assert len(ei._analyse(c.aids, c.ts, c.max_gap)['comps']) == 2
    assert L['general-n32'].n == 32 and L['reversed-n32'].n == 32


MASK_BIT = {k: i for i, k in enumerate(('click_cart', 'click_order', 'cart_order', 'click_click'))}


def test_filter_cases():
    L = ei.LIBRARY
    fk = tuple(MASK_BIT)
    for G in (8, 16, 32):
        for mask, f in MASK_BIT.items():
            c = L[f'filter-later-{mask}-G{G}']
            M = co.FILTER_MASKS[mask]
            assert not M[c.types[0]][c.types[1]] and M[c.types[2]][c.types[3]]        # first valid (0, 1) fails, (2, 3) passes
            bits = dict(((x, y), fb) for x, y, _, fb, _ in _oracle(c, fk))
            assert bits[(1, 2)] >> f & 1
            assert any(not fb >> f & 1 for fb in bits.values())                        # a pair where no valid pair passes
        c = L[f'filter-pass-not-valid-G{G}']
        bits = dict(((x, y), fb) for x, y, _, fb, _ in _oracle(c, fk))
        assert co.FILTER_MASKS['click_cart'][c.types[0]][c.types[2]] and c.ts[2] - c.ts[0] > c.max_gap
        assert not bits[(1, 2)] >> MASK_BIT['click_cart'] & 1 and bits[(1, 2)] >> MASK_BIT['click_click'] & 1
        c = L[f'filter-nine-cells-G{G}']
        cells = {(int(c.types[i]), int(c.types[j])) for i in range(c.n) for j in range(c.n) if i != j}
        assert len(cells) == 9


@pytest.mark.parametrize('window', [30, 32])
def test_tile_mixes_have_the_class_counts_their_names_claim(window):
    mixes = ei.tile_mixes()
    per_class = {G: set() for G in (8, 16, 32)}
    for i, (name, cnt) in enumerate(mixes.items()):
        claim = tuple(int(v) for v in re.search(r'-is-(\d+)-(\d+)-(\d+)$', name).groups())
        assert claim == cnt
        sess = ei.tile(*cnt, window, salt=i)
        assert len(sess) == 64
        ev = ei.stream(sess, window)
        n = np.minimum(np.diff(ev.sess_off), window)
        got = Counter(ei.lane_group(int(v)) for v in n)
        assert (got[8], got[16], got[32]) == claim, name
        if sum(claim) < 64:
            assert (np.diff(ev.sess_off) == 0).any() or (np.diff(ev.sess_off) == 1).any()
        for G, k in zip((8, 16, 32), claim):
            per_class[G].add(k)
    for G in (8, 16, 32):
        assert {0, 1, ei.WPW[G] - 1, ei.WPW[G], ei.WPW[G] + 1, 64} <= per_class[G]
    assert (0, 0, 64) in mixes.values()
    ev = ei.stream(ei.streams(window)['tile-mixes'][0], window)
    assert ev.n_sessions == 64 * len(mixes)


@pytest.mark.parametrize('window', [30, 32])
def test_named_streams(window):
    st = ei.streams(window)
    for n_sess in (1, 63, 64, 65, 257):
        assert len(st[f'n-sess-{n_sess}'][0]) == n_sess
    for name, (sess, g) in st.items():
        assert 1 <= len(sess) <= 4000
        assert all(nm in (ei.EMPTY, ei.SINGLE) or ei.LIBRARY[nm].max_gap == g for nm in sess), name
    # every library entry of a gap that fits the window is in that gap's library stream
    for g, tag in ((ei.GAP, 'g86400'), (0, 'g0'), (ei.TS_MAX, 'gmax')):
        assert set(st[f'library-{tag}'][0]) == {c.name for c in CASES if c.max_gap == g and c.fits(window)}
    # private rows in neighbouring windows of one wave step, for every lane-group size
    sess = st['private-neighbours'][0]
    for G in (8, 16, 32):
        run = [nm for nm in sess if ei.LIBRARY[nm].G == G]
        assert len(run) > ei.WPW[G] and all(ei.LIBRARY[nm].kind == 'private' for nm in run)
        assert sum(1 for nm in run[:ei.WPW[G]] if sum(r for _, _, r in ei.private_rows(
            ei.LIBRARY[nm].aids, ei.LIBRARY[nm].ts, ei.LIBRARY[nm].max_gap)) > 0) >= 2


@pytest.mark.parametrize('window', [30, 32])
def test_long_sessions_keep_only_the_tail(window):
    for tag, total in (('W+1', window + 1), ('3W', 3 * window)):
        name = f'long-{tag}-w{window}'
        aid, ts, ty = ei.session_events(name, window)
        c = ei.LIBRARY[name]
        assert len(aid) == total and (np.diff(ts.astype(np.int64)) >= 0).all()
        assert np.array_equal(aid[-window:], c.aids) and np.array_equal(ty[-window:], c.types)
        sp = co.CovisSpec(window=window, max_gap=c.max_gap)
        tail = co.expand_window_python(aid, ts, ty, 0, total, sp)
        assert tail == _oracle(c)
        whole = co.expand_window_python(aid, ts, ty, 0, total, co.CovisSpec(window=total, max_gap=c.max_gap))
        assert sorted(whole) != sorted(tail)                      # the events in front would change the records
        assert not c.fits(62 - window)
