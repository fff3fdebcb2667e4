"""Every case of ``tests/reduce_handover_inputs.py`` has the shape it claims (no GPU needed): the items per kernel fit ONE
workgroup's first reservation, they follow each other in the order claimed, and every item has the runs, heavy keys, ties
and per-partition key classes that put it on its path. Records, runs and keys of every aid are recomputed from the oracle's
pair expansion of the stream (``_profile`` of tests/test_reduce_inputs_cpu.py)."""
import numpy as np
import pytest

import reduce_handover_inputs as hi
import reduce_inputs as ri
from test_reduce_inputs_cpu import _profile


def _opts(case, oi=0):
    o = dict(case.option_sets[oi])
    return o.get('packed_heavy', 2), o.get('l_cap', ri.L_CAP)


def test_restated_pipeline_constants():
    assert hi.FIRST_RESERVE == 8 and hi.SH_MAX_HEAVY == 64 * 4 and hi.WARM_RUNS == 256 and hi.KS == (20, 32)
    assert {c.name for c in hi.CASES} == {'handover-m', 'handover-l512-guess', 'handover-l512-gather-bucket', 'handover-pref',
                                          'handover-ovf'}
    # the fewest runs of an M aid: 29 records per run at most, the bin starts at S_CAP + 1
    assert -(-(ri.S_CAP + 1) // (ri.MAX_SESSION - 1)) == 14
    y = np.arange(50000, dtype=np.int64)
    # the partition bits sit right below the slot bits of the hash
    assert np.array_equal(hi.partition_of(y, 13, 3), ri.home_slot(y, 16).astype(np.int64) & 7)


@pytest.mark.parametrize('case', hi.CASES, ids=lambda c: c.name)
def test_targets_have_their_records_and_every_kernel_fits_one_reservation(case):
    p = _profile(case)
    ev, where = p['ev'], p['where']
    n_by_rule, runs_by_rule = ri.records_runs(ev)
    assert np.array_equal(n_by_rule, p['n']) and np.array_equal(runs_by_rule, p['runs'])
    for t in case.targets:
        x, pids = where[t.name]
        rows = p['x'] == x
        assert (p['n'][x], p['runs'][x], p['d'][x]) == (t.n, t.runs, t.d), t.name
        assert np.array_equal(np.sort(p['y'][rows]), np.sort(pids)), t.name
        order = np.argsort(pids)
        assert np.array_equal(p['cao'][rows], np.asarray(t.counts).reshape(-1, 3)[order]), t.name
        if 'heavy' in t.expect:
            assert p['heavy'][x] == t.expect['heavy'], t.name
        for k, count in t.expect.get('ge_kth', {}).items():
            assert ri.ge_kth(p['w_click'][rows], k) == count, t.name      # ties in WEIGHT; the kernel's keys order them by aid_y
    others = np.ones(ev.n_aids, dtype=bool)
    others[[where[t.name][0] for t in case.targets]] = False
    assert p['n'][others].max() <= ri.S_CAP, 'a partner left the one-wave bin'
    for oi in range(len(case.option_sets)):
        ph, l_cap = _opts(case, oi)
        for t in case.targets:
            want = t.expect['kernel'].get(ph)
            if want is not None:
                assert ri.kernel_of(t.n, t.runs, ph, l_cap) == want, (t.name, oi)
        for kernel in ('M', 'L13x512', 'L14', 'Lwide'):
            assert len(hi.work_order(ev, kernel, ph, l_cap)) <= hi.FIRST_RESERVE, (kernel, oi)


def test_m_items_follow_each_other_as_claimed():
    case = hi.CASE_BY_NAME['handover-m']
    ev, where = ri.case_stream(case)
    order = hi.work_order(ev, 'M')
    assert [x for x, _, _ in order] == [where[t.name][0] for t in case.targets] and len(order) == hi.FIRST_RESERVE
    t = {u.name: u for u in case.targets}
    assert t['m0-fewest-runs'].runs == 14 and ri.bin_of(t['m0-fewest-runs'].n) == 'M'
    assert t['m1-many-runs'].runs > hi.WARM_RUNS and t['m1-many-runs'].runs > 64 * 4 * 4      # several batches per wave too
    for k in hi.KS:
        # sh: the single-wave selection serves the item; two-pass: too many heavy keys for it; redo: fewer than k heavy keys
        path = [('redo' if u.expect['heavy'] < k else ('sh' if u.expect['heavy'] <= hi.SH_MAX_HEAVY else 'two-pass')) for u in case.targets]
        assert path == [u.expect['path'] for u in case.targets]
        assert path == ['sh', 'sh', 'two-pass', 'sh', 'redo', 'sh', 'sh', 'redo']
    tie = np.asarray(t['m5-weight-ties'].counts)
    assert ((tie[:, 0] == 3).sum(), (tie[:, 0] == 2).sum()) == (10, 100) and not tie[:, 1:].any()
    assert t['m6-small-after'].d < t['m5-weight-ties'].d and t['m6-small-after'].n < t['m5-weight-ties'].n
    # at most SHR keys per lane and exactly k lanes at or above the k-th lane best: the SH list of m5 holds at most
    # min(heavy, 4 k) keys, and more than EXCAP of them only if the best keys sit four to a lane -- not controlled by the input
    assert t['m5-weight-ties'].expect['heavy'] == 110 <= hi.SH_MAX_HEAVY
    assert sorted(tuple(sorted(o.items())) for o in case.option_sets) == sorted(
        tuple(sorted(o.items())) for o in ({}, {'guess': 0}, {'hot': 0}, {'hot': 1}, {'hot': 2}))


def test_l512_partitions_hold_every_guess_outcome():
    case = hi.CASE_BY_NAME['handover-l512-guess']
    ev, where = ri.case_stream(case)
    t = case.targets[0]
    x, pids = where[t.name]
    assert all(o['l_cap'] == hi.L512_LCAP for o in case.option_sets)
    order = hi.work_order(ev, 'L13x512', 2, hi.L512_LCAP)
    assert order == [(x, p, hi.L512_LG) for p in range(8)]
    part = hi.partition_of(pids, 13, hi.L512_LG)
    c = np.asarray(t.counts)[:, 0]
    assert not np.asarray(t.counts)[:, 1:].any()
    got = tuple((int(((part == p) & (c == 3)).sum()), int(((part == p) & (c == 2)).sum()), int(((part == p) & (c == 1)).sum()))
                for p in range(8))
    assert got == hi.L512_PARTS
    for p in range(8):                                 # a sized bucket holds every partition: no retry round
        assert int(c[part == p].sum()) <= ri.bucket_cap(t.n, hi.L512_LG)
    # pilot: two-click keys only, so any threshold guess it leaves is a two-click key (it leaves one when at least 32 of the 64
    # group bests of P2 are valid, which depends on how its 510 keys fall on the waves: not proved here)
    assert got[0][1] == 510 and got[0][0] == got[0][2] == 0
    for k in hi.KS:
        three = [g[0] for g in got[1:]]
        assert k <= three[0] <= ri.EXCAP and three[1] < k and three[2] > ri.EXCAP
        assert all(k <= v <= ri.EXCAP for v in three[3:])
    assert all(g[1] == 0 for g in got[1:])             # nothing ties with the threshold outside the pilot


def test_gather_and_bucket_items_alternate():
    case = hi.CASE_BY_NAME['handover-l512-gather-bucket']
    ev, where = ri.case_stream(case)
    a, b, d = (where[t.name][0] for t in case.targets)
    assert a < b < d
    # whole aid (gather) -> pilot bucket -> whole aid (gather) -> guess buckets
    assert hi.work_order(ev, 'L13x512', 2, hi.GB_LCAP) == [(a, 0, 0), (b, 0, 2), (d, 0, 0), (b, 1, 2), (b, 2, 2), (b, 3, 2)]
    assert sorted(o.get('guess', 1) for o in case.option_sets) == [0, 1]


def test_pref_kernels_alternate_gather_and_bucket_items_and_end_on_the_largest():
    case = hi.CASE_BY_NAME['handover-pref']
    ev, where = ri.case_stream(case)
    assert all(o['l_cap'] == hi.PREF_LCAP and o['packed_heavy'] == 1 for o in case.option_sets)
    assert sorted(o.get('guess', 1) for o in case.option_sets) == [0, 1]
    t = {u.name: u for u in case.targets}
    assert hi.work_order(ev, 'L13x512', 1, hi.PREF_LCAP) == []
    for kernel, pre in (('L14', 'p14'), ('Lwide', 'pw')):
        ta, tb, td = t[f'{pre}-a-whole'], t[f'{pre}-b-four-partitions'], t[f'{pre}-d-whole']
        a, (b, pids), d = where[ta.name][0], where[tb.name], where[td.name][0]
        assert a < b < d
        # whole aid (gather) -> pilot bucket -> whole aid (gather) -> sibling buckets (guess path when guess = 1)
        order = hi.work_order(ev, kernel, 1, hi.PREF_LCAP)
        assert order == [(a, 0, 0), (b, 0, 2), (d, 0, 0), (b, 1, 2), (b, 2, 2), (b, 3, 2)]
        part = hi.partition_of(pids, hi.PREF_LOG2T[kernel], hi.PREF_LG)
        per_key = np.asarray(tb.counts).sum(axis=1)
        recs = {(b, p): int(per_key[part == p].sum()) for p in range(4)}
        assert [recs[(b, p)] for p in range(4)] == [3 * h + c for h, c in hi.PREF_PARTS[kernel]]
        assert max(recs.values()) <= ri.bucket_cap(tb.n, hi.PREF_LG)           # sized buckets hold them: no retry round
        recs[(a, 0)], recs[(d, 0)] = ta.n, td.n
        size = [recs[(x, p)] for x, p, _ in order]
        assert size[-1] == max(size) and size.count(size[-1]) == 1, 'the largest item is not the last'
        if kernel == 'Lwide':
            assert min(ta.runs, tb.runs, td.runs) >= ri.PACKED_MAX_RUNS
        else:
            assert max(ta.runs, tb.runs, td.runs) < ri.PACKED_MAX_RUNS


def test_overflowing_item_is_followed_by_a_small_one():
    case = hi.CASE_BY_NAME['handover-ovf']
    ev, where = ri.case_stream(case)
    big, small = (where[t.name][0] for t in case.targets)
    assert hi.work_order(ev, 'Lwide', 2, hi.OVF_LCAP) == [(big, 0, 0), (small, 0, 0)]
    assert case.targets[0].d > 1 << ri.KERNELS['Lwide']['log2t'] and case.targets[1].d < ri.KERNELS['Lwide']['ocap']
    assert case.min_retries == {0: 1}
