"""What the generators of tests/feat_edge_inputs.py claim, asserted on the CPU, so that the device tests over them
(tests/test_feat_edges_gpu.py) cannot pass without reaching the path they are named for. The restatement runs on every
case here as well: a case that breaks the reference shows up without a device."""
import numpy as np
import pytest

import feat_edge_inputs as fe
import feat_inputs as fi
import feat_restatement as fr


def _segment(aid, off, a):
    """(event indices, session ids) of aid a's segment: the stable sort by aid of the session-sorted stream."""
    order = np.argsort(aid, kind='stable')
    seg = order[aid[order] == a]
    sess = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return seg, sess[seg]


def _valid(aid, ts, typ, off, n_aids):
    assert aid.dtype == np.int32 and ts.dtype == np.int32 and typ.dtype == np.uint8 and off.dtype == np.int64
    assert off[0] == 0 and off[-1] == len(aid) == len(ts) == len(typ) and (np.diff(off) >= 0).all()
    assert len(aid) == 0 or (aid.min() >= 0 and aid.max() < n_aids and typ.max() <= 2)
    for s in np.flatnonzero(np.diff(off) > 1)[:2000]:
        assert (np.diff(ts[off[s]:off[s + 1]].astype(np.int64)) >= 0).all()          # (session, ts) order


@pytest.mark.parametrize('make', [fe.stride, fe.hot_stride, fe.hot_edges])
def test_counts_per_aid_are_the_ones_claimed(make):
    aid, ts, typ, off, n_aids, facts = make()
    _valid(aid, ts, typ, off, n_aids)
    counts = np.bincount(aid, minlength=n_aids)
    assert np.array_equal(counts, facts['counts'])
    assert np.array_equal(np.flatnonzero(counts == 0), facts['absent'])
    assert np.diff(off).max() <= fe.MAX_SESSION


def test_stride_reaches_the_stride_loop_and_the_sort_spans():
    aid, ts, typ, off, n_aids, facts = fe.stride()
    counts = np.bincount(aid, minlength=n_aids)
    assert n_aids == 16384 + 4 + 3 and n_aids % 4 == 3 and n_aids > fe.SPAN_AIDS
    assert counts[0] == 0 and (counts[-5:] == 0).all()
    assert [counts[a] for a in (16383, 16384, 16385)] == [3, 4, 5]
    assert counts[facts['at_1024']] == fe.HOT and np.flatnonzero(counts > fe.HOT).tolist() == facts['hot'] and counts.max() == fe.HOT + 1
    assert np.bincount(counts[(counts < 3)], minlength=3).min() > 4000          # most aids: 0, 1 or 2 events
    assert fe.SORT_SPAN < len(aid) < 20000                                       # the event sort crosses a workgroup span
    n_rank = fe.RANKED * n_aids
    assert n_rank > 13 * fe.SORT_SPAN                                            # the rank sort crosses 13 of them
    starts = [c * n_aids for c in range(1, fe.RANKED)]                           # column c's keys start here, nulls included
    assert all(0 < s % fe.SORT_TILE < fe.SORT_TILE - 1 for s in starts)         # strictly inside a sort tile, every one
    # runs of absent aids for the bounds kernel: before the first key, after the last one and inside
    absent = facts['absent']
    assert absent[0] == 0 and absent[-1] == n_aids - 1 and (np.diff(absent) == 1).sum() > 100


def test_stride_bad_aid_differs_in_one_event():
    good, bad = fe.stride(), fe.stride_bad_aid()
    assert (good[0] != bad[0]).sum() == 1 and bad[0].max() == bad[4] == good[4]
    for g, b in zip(good[1:4], bad[1:4]):
        assert np.array_equal(g, b)


def test_hot_stride_has_more_hot_aids_than_hot_workgroups():
    aid, ts, typ, off, n_aids, facts = fe.hot_stride()
    counts = np.bincount(aid, minlength=n_aids)
    assert (counts > fe.HOT).sum() == facts['n_hot'] == 1026 > 1024 and (counts == fe.HOT + 1).sum() == 1026
    assert (counts == fe.HOT).sum() == 1 and 0 < ((counts > 0) & (counts < fe.HOT)).sum() < 10
    assert n_aids % 4 != 0 and np.diff(off).max() <= 40 and len(aid) > 64 * fe.SORT_SPAN
    day = fr.calendar(ts)[0]
    assert day.max() - day.min() == 13


def test_hot_edges_sit_on_both_sides_of_every_threshold():
    aid, ts, typ, off, n_aids, facts = fe.hot_edges()
    counts = np.bincount(aid, minlength=n_aids)
    assert counts[1:9].tolist() == [1023, 1024, 1025, 1024, 1025, 1088, 2048, 2049] == facts['sizes']
    assert counts[0] == 0 and counts[-1] == 0 and n_aids % 4 == 0
    assert (counts > fe.HOT).sum() == facts['n_hot'] == 5
    assert 2048 % (4 * 64) == 0 and 1024 == 16 * 64 and (1025 + 63) % 64 == 0
    assert 5000 < len(aid) < 12000


def test_runs_sit_where_the_scan_changes_chunk_and_wave():
    aid, ts, typ, off, n_aids, facts = fe.runs()
    _valid(aid, ts, typ, off, n_aids)
    week = fr.calendar(ts)[3]
    last_week = max(fr.week_slots(week))
    assert last_week == 32
    counts = np.bincount(aid, minlength=n_aids)
    assert counts[fe.RUN_COLD] == 1000 <= fe.HOT < counts[fe.RUN_HOT] == 1300 and (counts[2:] > 0).all()
    assert np.diff(off).max() <= fe.MAX_SESSION
    for a in (fe.RUN_COLD, fe.RUN_HOT):
        seg, sess = _segment(aid, off, a)
        total = len(seg)
        heads = np.flatnonzero(np.r_[True, sess[1:] != sess[:-1]])
        length = dict(zip(heads.tolist(), np.diff(np.r_[heads, total]).tolist()))
        r = facts['runs'][a]
        for name, (start, n) in r.items():
            assert length[start] == n, (a, name)
        assert r['straddle'] == (60, 11)                                         # positions 60 .. 70: over the chunk edge at 64
        assert r['head_lane_63'][0] % 64 == 63 and r['head_lane_63'][1] > 1      # the forward walk starts from lane 63
        assert typ[seg[255:258]].tolist() == [0, 1, 2] and typ[seg[60:71]].tolist() == [0] * 10 + [2]   # types only the walk sees
        assert r['head_lane_0'][0] % 64 == 0 and r['head_lane_0'][0] > 0         # the head is found by looking back a chunk
        assert length[r['head_lane_0'][0] - 64] == 64 and r['sixty_four'] == (128, 64)
        start, n = r['types']
        assert n == 200
        ty = typ[seg[start:start + n]]
        cart, order = start + facts['cart_at'], start + facts['order_at']
        assert np.flatnonzero(ty == 1).tolist() == [130] and np.flatnonzero(ty == 2).tolist() == [199]
        assert len({start // 64, cart // 64, order // 64}) == 3
        lw_start, lw_n = r['last_week']
        lw = week[seg[lw_start:lw_start + lw_n]] == last_week
        assert np.flatnonzero(lw).tolist() == [lw_n - 1]
        lw_last = lw_start + lw_n - 1
        assert lw_last // 64 == lw_start // 64 + 2                              # two chunks after its head
        if a == fe.RUN_HOT:                                                      # chunks go round the four waves of the workgroup
            wave = lambda p: (p // 64) % 4
            assert wave(cart) != wave(start) and wave(order) != wave(start) and wave(cart) != wave(order)
            assert wave(lw_last) != wave(lw_start)
            assert wave(59) != wave(64) and wave(255) != wave(256)
        assert r['last'] == (total - 1, 1) and r['before_last'] == (total - 4, 3)
    per = fe.sessions_per_aid(aid, typ, off, n_aids)                             # a session count one off moves a rank
    for a in (fe.RUN_COLD, fe.RUN_HOT):
        for q in range(4):
            others = np.delete(per[:, q], a)
            assert per[a, q] - 1 in others and per[a, q] + 1 in others and per[a, q] > 1, (a, q)
    want = fr.aid_table(aid, ts, typ, off, n_aids)
    assert want[fe.RUN_COLD, 30] > 0 and not np.isnan(want[:2, 8:20]).any()      # both aids have carts, orders and last-week events


def test_weeks_appear_out_of_calendar_order_across_the_prep_workgroups():
    aid, ts, typ, off, n_aids, facts = fe.weeks()
    _valid(aid, ts, typ, off, n_aids)
    day, _, _, week = fr.calendar(ts)
    slots = fr.week_slots(week)
    assert slots == facts['slots'] == [50, 2, 52, 48, 1, 51, 49] and len(slots) == 7 <= 10
    first = [int(np.flatnonzero(week == w)[0]) for w in slots]
    assert first == facts['first'] == [0, 1023, 1024, 1025, 3100, 3500, 3900]
    assert first[1] // 1024 == 0 and first[2] // 1024 == 1 and min(first[4:]) > 3000
    assert max(slots) == 52 and slots.index(52) == 2                             # the "last week" is a middle slot
    assert slots != sorted(slots) and slots != [48, 49, 50, 51, 52, 1, 2]
    assert day.max() - day.min() == 46 and fr.day_table(int(day.min()), int(day.max()))[[0, -1], 2].tolist() == [48, 2]
    want = fr.aid_table(aid, ts, typ, off, n_aids)
    per = lambda a, t: [int(((aid == a) & (typ == t) & (week == w)).sum()) for w in slots]
    assert set(week[aid == facts['only_52']]) == {52} and not np.isnan(want[facts['only_52'], [20, 21, 30]]).any()
    assert set(week[aid == facts['only_1_2']]) == {1, 2} and np.isnan(want[facts['only_1_2'], [19, 20, 21, 30]]).all()
    c = per(facts['inf_last'], 0)
    assert c[4] > 0 and c[5] == 0 and c[6] > 0 and np.isnan(want[facts['inf_last'], 25])       # -1, then inf -> NaN
    c = per(facts['zero_inside'], 1)
    assert c[1] > 0 and c[2] == 0 and c[3] > 0 and want[facts['zero_inside'], 26] == -1.0
    assert want[facts['zero_inside'], 23] == 0.0 and np.isnan(want[-2:]).all()


def test_every_ranked_column_of_stride_holds_ties_and_nulls(stride_table):
    want = stride_table
    for col in fr.RANK_COLUMN.values():
        v = want[:, col]
        assert np.isnan(v).any() and len(np.unique(v[~np.isnan(v)])) < (~np.isnan(v)).sum(), col
    present = ~np.isnan(want[:, 28])
    assert not np.isnan(want[present][:, [0, 28, 29]]).any()


@pytest.fixture(scope='module')
def stride_table():
    return fr.aid_table(*fe.stride()[:5])


def test_tiny_cases():
    one, none, only_2 = fe.tiny()
    for case in (one, none, only_2):
        _valid(*case[:5])
        want = fr.aid_table(*case[:5])
        assert want.shape == (case[4], 31)
        assert fr.session_table(*case[:4], want).shape == (len(case[3]) - 1, 15)
    assert one[4] == 1 and len(one[0]) == 1
    assert none[4] == 3 and len(none[0]) == 0 and np.isnan(fr.aid_table(*none[:5])).all()
    assert only_2[4] == 5 and set(only_2[0]) == {2}
    want = fr.aid_table(*only_2[:5])
    assert np.isnan(want[[0, 1, 3, 4]]).all() and want[2, 28] == 5 and want[2, 8] == 1.0


def test_sess_stride_lengths_and_empty_sessions(stride_table):
    aid, ts, typ, off, n_aids, facts = fe.sess_stride()
    _valid(aid, ts, typ, off, n_aids)
    lens = np.diff(off)
    assert len(lens) == 16384 + 4 + 2 and len(lens) % 4 == 2 and set(lens) == {0, 1, 2, 3}
    assert np.array_equal(lens, facts['lens'])
    for s in (0, len(lens) - 1, 100, 101, 16383, 16384):
        assert lens[s] == 0
    assert lens[1] and lens[99] and lens[102] and lens[16382] and lens[16385] and lens[-2]
    assert n_aids == stride_table.shape[0] and np.isnan(stride_table[aid, 28]).any()          # absent aids are looked up too
    want = fr.session_table(aid, ts, typ, off, stride_table)
    assert (want[lens == 0, 0] == 0).all() and np.isnan(want[lens == 0, 2:]).all()


def test_sess_lengths_and_the_uint8_wrap():
    aid, ts, typ, off, n_aids, facts = fe.sess_lengths()
    _valid(aid, ts, typ, off, n_aids)
    table = fr.aid_table(*fe.sess_table_events())
    assert table.shape[0] == n_aids and np.isnan(table[fe.SESS_TABLE_PRESENT:]).all() and not np.isnan(table[:fe.SESS_TABLE_PRESENT, 28]).any()
    lens = np.diff(off)
    assert lens[:10].tolist() == [0, 1, 63, 64, 65, 127, 128, 129, 511, 512] == facts['lens'] and lens[-1] == 0
    want = fr.session_table(aid, ts, typ, off, table)
    got = {}
    for s, d in facts['distinct'].items():
        assert len(set(aid[off[s]:off[s + 1]])) == d
        got[(int(lens[s]), d)] = int(want[s, 1])
    assert got == {(300, 255): 255, (300, 256): 0, (300, 257): 1, (512, 512): 0, (512, 1): 1}
    s = facts['all_nan']
    assert np.isnan(table[aid[off[s]:off[s + 1]], 28]).all() and np.isnan(want[s, 5:]).all() and want[s, 0] == 10
    s = facts['nan_last']
    rows = table[aid[off[s]:off[s + 1]]]
    assert np.isnan(rows[-1]).all() and not np.isnan(rows[:-1, 28]).any()
    assert want[s, 8] == rows[-2, 28] and want[s, 12] == rows[-2, 29] and want[s, 2] == aid[off[s + 1] - 1]


def test_sess_errors_are_the_two_the_kernel_counts():
    cases = fe.sess_errors()
    aid, ts, typ, off, n_aids = cases['too_long']
    assert np.diff(off).tolist() == [3, 513, 2] and aid.max() < n_aids
    aid, ts, typ, off, n_aids = cases['aid_beyond_the_table']
    assert (aid == n_aids).sum() == 1 and aid.max() == n_aids and np.diff(off).max() <= fe.MAX_SESSION


def test_matrix_cases():
    pairs = fe.matrix_pairs()
    assert {r for r, _ in pairs} == set(fe.MATRIX_ROWS) == {255, 256, 257, 512, 513}
    assert {F for _, F in pairs} == set(fe.MATRIX_F) == {1, 2, 3, 4, 32, 63, 64} and len(pairs) == len(set(pairs)) == 14
    assert [F for F in fe.MATRIX_F if F > 1 and 256 % F == 0] == [2, 4, 32, 64]  # the index walk with no column carry
    for n_rows in fe.MATRIX_ROWS:
        sizes = fe.matrix_sizes(n_rows)
        assert sum(sizes) == n_rows and sizes[0] == 0 and sizes[-1] == 0 and max(sizes) < 130
    off = np.r_[0, np.cumsum(fe.BIG_SESSIONS)]
    assert list(fe.BIG_SESSIONS) == [0, 256, 0, 600, 1, 255, 0, 0, 257, 0]
    tiles = np.arange(0, off[-1], 256)
    owner = lambda r: int(np.searchsorted(off, r, side='right')) - 1
    assert [int(t) for t in tiles if t in off[:-1][np.diff(off) > 0]] == [0, 256]   # tiles that start on a session's first row
    assert any(owner(t) == owner(t + 255) == 3 and off[3] < t for t in tiles)    # a tile wholly inside the 600-row session
    assert off[2] == off[3] == 256 and off[6] == off[7] == off[8] == 1112 and off[-1] == off[-2] == 1369
    m, names = fe.matrix_case(fe.BIG_SESSIONS, 63, seed=1)
    assert len(names) == len(set(names)) == 63 and m['aid_tab'].shape == (997, 31) and np.isnan(m['aid_tab']).mean() > 0.05
    from otto_amd.ranker import interaction_feature_engineering as ife
    prog = fr.resolve(names, ife.ROW_COLUMNS, ife.SESSION_COLUMNS, ife.AID_COLUMNS)
    want = fr.matrix(m['row_off'], m['cand'], m['score'], m['inter_row'], m['inter_sess'], m['inter_aid'], m['aid_tab'], m['sess_tab'], prog)
    assert want.shape == (1369, 63)


def test_the_restatement_runs_on_the_large_cases():
    for make in (fe.hot_stride, fe.hot_edges):
        aid, ts, typ, off, n_aids, facts = make()
        want = fr.aid_table(aid, ts, typ, off, n_aids)
        assert np.isnan(want[facts['absent']]).all() and np.array_equal(want[:, 28][~np.isnan(want[:, 28])], facts['counts'][facts['counts'] > 0])
    aid, ts, typ, off, n_aids, _ = fe.hot_edges()
    assert fr.session_table(aid, ts, typ, off, fr.aid_table(aid, ts, typ, off, n_aids)).shape == (len(off) - 1, 15)
