"""Every case of ``tests/reduce_inputs.py`` has the shape its name claims (no GPU needed). tests/test_covis_reduce_edges_gpu.py
compares the reduce kernel with the oracle on these streams; if a stream lost its edge -- one record more or less, a run too
many, a partner that became a heavy aid of its own -- those tests would still pass and prove nothing. Each stream is expanded
with the oracle, and records, runs, distinct keys, heavy keys and tie classes are recomputed per aid from its pairs."""
import numpy as np
import pytest

import covis_oracle as co
import reduce_inputs as ri

TYPE3 = ('click_weighted', 'cart_weighted', 'order_weighted')
_profiles = {}


def _profile(case):
    """Per-aid facts of a case's stream from the oracle's pair expansion: the three type-weighted sums of a pair,
    c + 6 a + 3 o, c + 9 a + 6 o and c + 3 a + 6 o, give back its click, cart and order records exactly."""
    if case.name in _profiles:
        return _profiles[case.name]
    ev, where = ri.case_stream(case)
    pairs = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(kinds=TYPE3 + ('time_weighted',)))
    x, y, w1 = pairs['click_weighted']
    for kind in TYPE3[1:] + ('time_weighted',):
        assert np.array_equal(pairs[kind][0], x) and np.array_equal(pairs[kind][1], y)
    w1, w2, w3 = (pairs[kind][2].astype(np.int64) for kind in TYPE3)
    assert not (w1 % ri.Q16).any() and not ((w2 - w3) % (6 * ri.Q16)).any() and not ((w1 - w3) % (3 * ri.Q16)).any()
    a = (w2 - w3) // (6 * ri.Q16)
    o = a - (w1 - w3) // (3 * ri.Q16)
    c = w1 // ri.Q16 - 6 * a - 3 * o
    cao = np.c_[c, a, o]
    assert (cao >= 0).all() and (cao.sum(axis=1) >= 1).all()
    xi = x.astype(np.int64)
    sess = np.repeat(np.arange(ev.n_sessions), np.diff(ev.sess_off))
    held = np.unique(np.c_[sess, ev.aid.astype(np.int64)][np.repeat(np.diff(ev.sess_off) >= 2, np.diff(ev.sess_off))], axis=0)
    p = dict(ev=ev, where=where, x=xi, y=y.astype(np.int64), cao=cao, w_click=w1, w_time=pairs['time_weighted'][2].astype(np.int64),
             n=np.bincount(xi, weights=cao.sum(axis=1), minlength=ev.n_aids).astype(np.int64),
             d=np.bincount(xi, minlength=ev.n_aids),
             heavy=np.bincount(xi, weights=~ri.is_light(cao), minlength=ev.n_aids).astype(np.int64),
             runs=np.bincount(held[:, 1], minlength=ev.n_aids))
    _profiles[case.name] = p
    return p


def test_geometry_restated_on_its_own_edges():
    assert [ri.bin_of(n) for n in (1, 384, 385, 3072, 3073)] == ['S', 'S', 'M', 'M', 'L']
    assert ri.kernel_of(6144, 4095) == ('L13x512', 1) and ri.kernel_of(6145, 4095) == ('L14', 1)
    assert ri.kernel_of(12288, 4095) == ('L14', 1) and ri.kernel_of(12289, 4095) == ('L13x512', 4)
    assert ri.kernel_of(12289, 4095, packed_heavy=1) == ('L14', 2) and ri.kernel_of(12289, 4095, packed_heavy=0) == ('Lwide', 4)
    assert ri.kernel_of(6144, 4096) == ('Lwide', 1) and ri.kernel_of(6145, 4096) == ('Lwide', 2)
    assert ri.bucket_cap(13000, 2) == 6756 and ri.bucket_cap(6144, 0) == 0
    assert [ri.dense_certain('M', d) for d in (480, 481, 1920, 1921)] == [True, None, None, False]
    assert ri.ge_kth([3, 2, 2, 2, 1], 2) == 4 and ri.ge_kth([5, 4], 20) == 2


def test_case_table_covers_what_the_kernel_can_get_wrong():
    names = set(ri.CASE_BY_NAME)
    assert {'bin-edges-runs-n', 'bin-edges-packed', 'table-load', 'wide-lcap8000', 'dense-M', 'dense-L13x512', 'dense-L14',
            'dense-Lwide', 'heavy-first-k20', 'heavy-first-k32', 'ties', 'ties-same-ts', 'partitions', 'time-sum-bound',
            'k-sweep'} <= names
    for cap in (ri.S_CAP, ri.M_CAP, ri.L_CAP, 2 * ri.L_CAP):
        assert {cap - 1, cap, cap + 1} <= set(ri.BIN_EDGE_N)
    ids = set(ri.BIN_EDGE_IDS.values())
    assert {ri.ITEM_BLOCK_AIDS - 1, ri.ITEM_BLOCK_AIDS, 2 * ri.ITEM_BLOCK_AIDS - 1, 2 * ri.ITEM_BLOCK_AIDS, 'last'} <= ids
    for name in ('bin-edges-runs-n', 'bin-edges-packed'):
        case = ri.CASE_BY_NAME[name]
        assert [o['packed_heavy'] for o in case.option_sets] == [2, 1, 0]
        # heavy aids on both sides of a block edge and on the last aid
        at = {t.aid: ri.bin_of(t.n) for t in case.targets}
        assert all(at[i] == 'L' for i in (2047, 2048, 4095, 4096, 'last'))
    multi = ('M', 'L13x512', 'L14', 'Lwide')
    for k in (20, 32):
        case = ri.CASE_BY_NAME[f'heavy-first-k{k}']
        assert case.ks == (k,) and sorted(o['hot'] for o in case.option_sets) == [0, 1, 2]
        assert {t.name for t in case.targets} == {f'{kern}-heavy{h}' for kern in multi for h in (k - 1, k, k + 1)}
        assert all(t.d - t.expect['heavy'] >= 1000 for t in case.targets)
    for kern in multi:
        g = ri.KERNELS[kern]
        ds = {t.d for t in ri.CASE_BY_NAME[f'dense-{kern}'].targets} | {t.d for t in ri.CASE_BY_NAME['wide-lcap8000'].targets}
        assert {g['rcap'], g['ocap'], g['ocap'] + 1, g['cap']} <= ds
    load = {t.name: t for t in ri.CASE_BY_NAME['table-load'].targets}
    for kern, g in ri.KERNELS.items():
        assert load[f'{kern}-full'].d == load[f'{kern}-full'].n == g['cap'] and load[f'{kern}-one-key'].n == g['cap']
        assert int(load[f'{kern}-one-key'].counts[0].sum()) == min(g['cap'], ri.PACKED_MAX_RUNS - 1 if kern in ('L13x512', 'L14') else g['cap'])
    part = ri.CASE_BY_NAME['partitions']
    assert sorted((o['guess'], o['part_sized']) for o in part.option_sets) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    dom = part.targets[2]
    assert dom.runs >= ri.PACKED_MAX_RUNS and int(dom.counts[0].sum()) > ri.bucket_cap(dom.n, ri.log2_parts(dom.n, dom.runs))
    assert all(o['part_sized'] == 1 for i, o in enumerate(part.option_sets) if part.min_retries.get(i))
    assert set(ri.CASE_BY_NAME['k-sweep'].ks) == {1, 20, 32} and ri.CASE_BY_NAME['ties-same-ts'].same_ts
    for case in ri.CASES:
        assert max(t.n for t in case.targets) <= 30000 and max(case.ks) <= ri.MAX_K


@pytest.mark.parametrize('case', ri.CASES, ids=lambda c: c.name)
def test_stream_is_built_as_described(case):
    ev, where = ri.case_stream(case)
    length = np.diff(ev.sess_off)
    assert length.min() >= 2 and length.max() <= ri.MAX_SESSION
    sess = np.repeat(np.arange(ev.n_sessions), length)
    assert len(np.unique(np.c_[sess, ev.aid.astype(np.int64)], axis=0)) == ev.n_events, 'an aid twice in a session'
    ts = ev.ts.astype(np.int64)
    inside = np.r_[False, sess[1:] == sess[:-1]]
    assert (np.diff(ts, prepend=ts[0])[inside] >= 0).all() and (np.diff(ts, prepend=ts[0])[inside] <= 1).all()
    assert int(ev.aid.max()) < ev.n_aids < 1 << 26
    if case.same_ts:
        assert ts.min() == ts.max()
    xs = [where[t.name][0] for t in case.targets]
    partners = np.concatenate([where[t.name][1] for t in case.targets])
    assert len(np.unique(partners)) == len(partners) and not np.isin(partners, xs).any() and len(set(xs)) == len(xs)
    for t in case.targets:
        x = where[t.name][0]
        assert x == (ev.n_aids - 1 if t.aid == 'last' else (x if t.aid is None else t.aid))
        own = np.isin(sess, sess[ev.aid == x])
        assert (ev.type[ev.aid == x] == t.x_type).all()
        if t.at_ts_max:
            assert (ts[own] == ts.max()).all() and ts.min() < ts.max()
        elif not case.same_ts:
            assert (ts[own] < ts.max()).all() or not any(u.at_ts_max for u in case.targets)


@pytest.mark.parametrize('case', ri.CASES, ids=lambda c: c.name)
def test_targets_have_the_named_records_runs_keys_and_paths(case):
    p = _profile(case)
    ev, where = p['ev'], p['where']
    n_by_rule, runs_by_rule = ri.records_runs(ev)
    assert np.array_equal(n_by_rule, p['n']) and np.array_equal(runs_by_rule, p['runs'])
    l_cap = case.option_sets[0].get('l_cap', ri.L_CAP)
    for t in case.targets:
        x, pids = where[t.name]
        rows = p['x'] == x
        assert (p['n'][x], p['runs'][x], p['d'][x]) == (t.n, t.runs, t.d), t.name
        assert np.array_equal(p['y'][rows], pids) and np.array_equal(p['cao'][rows], np.asarray(t.counts).reshape(-1, 3)), t.name
        e = t.expect
        if 'heavy' in e:
            assert p['heavy'][x] == e['heavy'], t.name
        for k, count in e.get('ge_kth', {}).items():
            assert ri.ge_kth(p['w_click'][rows], k) == count, t.name
            if case.same_ts:                           # one timestamp: the time weight is 65536 per record of whatever type
                assert np.array_equal(p['w_time'][rows], ri.Q16 * np.asarray(t.counts).sum(axis=1)), t.name
                assert ri.ge_kth(p['w_time'][rows], k) == (300 if t.name == 'S-257-of-300-tie' else count), t.name
        for ph, want in e.get('kernel', {}).items():
            assert ri.kernel_of(t.n, t.runs, ph, l_cap) == want, (t.name, ph)
        if 'dense' in e:
            assert ri.dense_certain(e['kernel'][2][0], t.d) is e['dense'], t.name
        for kind, w in e.get('top_w', {}).items():
            got = {'click_weighted': p['w_click'], 'time_weighted': p['w_time']}[kind][rows]
            assert int(got.max()) == w and (got == w).sum() == 1, t.name
    others = np.ones(ev.n_aids, dtype=bool)
    others[[where[t.name][0] for t in case.targets]] = False
    assert p['n'][others].max() <= case.other_max, f"a partner has {p['n'][others].max()} records"
    if case.other_max <= ri.S_CAP:                     # then the targets are the only aids outside the one-wave bin
        want = ri.expected_items(ev, 2, l_cap)
        assert want['items_s'] == int((p['n'] > 0).sum()) - sum(ri.bin_of(t.n) != 'S' for t in case.targets)


def test_heavy_first_cases_hold_the_single_cart_and_order_keys():
    for k in (20, 32):
        for t in ri.CASE_BY_NAME[f'heavy-first-k{k}'].targets:
            c = np.asarray(t.counts)
            assert ((c == (0, 1, 0)).all(axis=1).sum(), (c == (0, 0, 1)).all(axis=1).sum()) == (1, 1)
            assert (~ri.is_light(c)).sum() == t.expect['heavy']


def test_time_sum_bound_weights_in_python_integers():
    case = ri.CASE_BY_NAME['time-sum-bound']
    ev, _ = ri.case_stream(case)
    t0, t1 = int(ev.ts.min()), int(ev.ts.max())
    per_record = 65536 + (3 * 65536 * (t1 - t0)) // (t1 - t0)
    assert per_record == 4 * 65536
    assert case.targets[1].expect['top_w']['time_weighted'] == 4095 * per_record < 2 ** 30
    assert case.targets[2].expect['top_w']['time_weighted'] == 3072 * per_record < 2 ** 30
    assert 4096 * per_record == 2 ** 30


def test_tie_past_the_candidate_list_ends_on_the_key_that_wins_it():
    """257 cart keys tie in the one-wave bin and 256 fit the candidate list. No two of the 300 keys share a first slot, so
    each sits in its first slot; the smallest aid_y -- rank 1 of the tie -- has the last slot, which the walk reaches last."""
    for name in ('ties', 'ties-same-ts'):
        case = ri.CASE_BY_NAME[name]
        t = {u.name: u for u in case.targets}['S-257-of-300-tie']
        _, pids = ri.case_stream(case)[1][t.name]
        slots = ri.home_slot(pids, ri.KERNELS['S']['log2t'])
        assert len(np.unique(slots)) == len(pids) == 300 and (np.diff(pids) > 0).all()
        assert slots[0] == 511 and tuple(t.counts[0]) == (0, 1, 0)
        assert (np.asarray(t.counts)[:, 1] == 1).sum() == ri.CCAP + 1
