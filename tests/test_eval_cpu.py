"""SPEC-EVAL without a GPU: the NumPy restatement (tests/eval_restatement.py) against the labels the reference's own
``validation.get_labels`` gave (tests/golden/eval_golden.npz), the hand-worked file, ``otto_amd.metrics.recall_at_20`` and
the committed metric cases; the cutoff rule; the split as a partition of every session."""
import json
import math
import os

import numpy as np
import pytest

import eval_inputs as ei
import eval_restatement as er
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'eval_golden.npz'))


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'eval_hand.json')) as f:
        return json.load(f)


def test_restatement_reproduces_reference_labels_at_every_index(golden):
    aid, typ, off = golden['aid'], golden['typ'], golden['sess_off']
    assert len(off) - 1 >= 200
    for s in range(len(off) - 1):
        b, e = int(off[s]), int(off[s + 1])
        for i in range(e - b):
            click, carts, orders = er.labels_after(aid[b:e], typ[b:e], i)
            p = b + i
            assert click == ([int(golden['click'][p])] if golden['click'][p] >= 0 else []), (s, i)
            assert carts == golden['cart_aid'][golden['cart_off'][p]:golden['cart_off'][p + 1]].tolist(), (s, i)
            assert orders == golden['order_aid'][golden['order_off'][p]:golden['order_off'][p + 1]].tolist(), (s, i)


def test_restatement_reproduces_hand_file(hand):
    for case in hand['split']:
        for at in case['at']:
            got = er.labels_after(case['aids'], case['types'], at['cutoff'])
            assert got == (at['clicks'], at['carts'], at['orders']), (case, at)
    for case in hand['last_click']:
        t = np.asarray(case['types'], dtype=np.uint8)
        assert er.last_click(t, np.array([0, len(t)])).tolist() == [case['last_click']]
    for case in hand['hits']:
        h, d = er.hits([case['labels']], [case['pred']], cap=case['cap'])
        assert (int(h[0]), int(d[0])) == (case['hits'], case['denom']), case


def test_split_of_all_sessions_equals_per_session_labels(hand):
    sessions = [(c['aids'], c['types'], at['cutoff']) for c in hand['split'] for at in c['at']]
    aid, ts, typ, off, cutoff = ei.pack(sessions)
    kept, labels = er.split(aid, ts, typ, off, cutoff)
    want = [at for c in hand['split'] for at in c['at']]
    for name in ('clicks', 'carts', 'orders'):
        assert er.lists_csr(*labels[name]) == [at[name] for at in want]
    assert np.diff(kept['sess_off']).tolist() == [at['cutoff'] + 1 for at in want]


def test_restated_hits_equal_host_metric():
    from otto_amd import metrics
    with open(os.path.join(GOLDEN, 'metrics_golden.json')) as f:
        cases = json.load(f)
    labels, rows = [c['gt'] for c in cases], [c['pred'] for c in cases]
    h, d = er.hits(labels, rows, cap=20)
    assert h.sum() / d.sum() == metrics.recall_at_20(rows, labels)
    for c, hj in zip(cases, h):
        if not c['gt']:
            assert c['cart_order'] is None and c['click'] is None      # NaN in the reference, no denominator here
            continue
        distinct = len(set(c['gt']))
        assert hj / min(distinct, 20) == pytest.approx(c['cart_order'], rel=0, abs=1e-15)
        assert int(c['gt'][0] in c['pred'][:20]) == c['click']
    for S, k in ((65, 20), (257, 64)):
        lab, pred, n = ei.padded_case(S, k)
        rows = er.rows_padded(pred, n)
        h, d = er.hits(lab, rows, cap=20)
        want = metrics.recall_at_20([[v for v in r if v >= 0] for r in (row[:20] for row in rows)], lab)
        assert h.sum() / d.sum() == want
    lab, rows = ei.csr_case(40)
    h, d = er.hits(lab, rows, cap=20)
    assert h.sum() / d.sum() == metrics.recall_at_20([[v for v in r[:20] if v >= 0] for r in rows], lab)
    assert math.isnan(metrics.recall_at_20([[1]], [[]])) and er.hits([[]], [[1]])[1].sum() == 0


def test_hits_session_alignment_rules():
    lab = [[1], [2, 2], [3]]
    ids = np.array([10, 20, 30], dtype=np.int32)
    h, d = er.hits(lab, [[2], [3, 1]], label_session=ids, pred_session=[20, 30])
    assert h.tolist() == [0, 1, 1] and d.tolist() == [1, 2, 1]          # a session without a row keeps its denominator
    with pytest.raises(er.Refused):
        er.hits(lab, [[2]], label_session=ids, pred_session=[25])
    t = er.totals(h, d, mask=[1, 0, 1])
    assert t == {'hits': 2, 'denom': 4, 'mask_hits': 1, 'mask_denom': 2}


def test_cutoff_rule():
    rng = np.random.default_rng(3)
    sessions = [ei.random_session(rng, int(n)) for n in rng.integers(0, 30, 4000)]
    _, _, typ, off, _ = ei.pack(sessions)
    last = er.last_click(typ, off)
    for seed in (0, 1, 2 ** 63 + 5):
        cut, without = er.cutoffs(typ, off, seed)
        n = np.diff(off)
        assert np.all(cut[n == 2] == 0) and np.all(cut[last <= 0] == 0)
        free = (n != 2) & (last > 0)
        assert np.all((cut[free] >= 0) & (cut[free] < last[free]))
        assert without == int(np.sum((last < 0) & (n != 2)))
        assert np.all(cut < np.maximum(n, 1))
    assert not np.array_equal(er.cutoffs(typ, off, 1)[0], er.cutoffs(typ, off, 2)[0])
    # roughly uniform: 200,000 sessions whose last click is at index 10; each of the 10 values expects 20,000 draws with
    # a standard deviation of sqrt(200000 * 0.1 * 0.9) = 134; six of those is a bound a fair hash stays inside
    S = 200_000
    typ = np.tile(np.array([1] * 10 + [0], dtype=np.uint8), S)
    off = np.arange(S + 1, dtype=np.int64) * 11
    cut, without = er.cutoffs(typ, off, 12345)
    assert without == 0
    counts = np.bincount(cut, minlength=10)
    assert len(counts) == 10 and np.all(np.abs(counts - S / 10) < 6 * 134), counts


@pytest.mark.parametrize('name', ('S_65', 'lengths', 'edges'))
def test_kept_events_and_tail_partition_every_session(name):
    aid, ts, typ, off, cutoff = ei.pack(ei.split_cases()[name])
    kept, labels = er.split(aid, ts, typ, off, cutoff)
    for s in range(len(off) - 1):
        b, e = int(off[s]), int(off[s + 1])
        kb, ke = int(kept['sess_off'][s]), int(kept['sess_off'][s + 1])
        assert np.array_equal(kept['aid'][kb:ke], aid[b:b + (ke - kb)]) and np.array_equal(kept['typ'][kb:ke], typ[b:b + (ke - kb)])
        assert np.array_equal(kept['ts'][kb:ke], ts[b:b + (ke - kb)])
        tail_a, tail_t = aid[b + (ke - kb):e], typ[b + (ke - kb):e]
        assert (ke - kb) + len(tail_a) == e - b and (ke - kb == cutoff[s] + 1 or e == b)
        for t, lname in ((1, 'carts'), (2, 'orders')):
            o, a = labels[lname]
            assert a[o[s]:o[s + 1]].tolist() == sorted(set(tail_a[tail_t == t].tolist()))
        o, a = labels['clicks']
        clicks = tail_a[tail_t == 0]
        assert a[o[s]:o[s + 1]].tolist() == clicks[:1].tolist()


def test_refusals_of_the_restatement():
    aid, ts, typ, off, cutoff = ei.pack([([1, 2, 3], [0, 1, 2], 0), ([], [], 0)])
    for bad in ([3, 0], [-1, 0], [0, 1]):
        with pytest.raises(er.Refused):
            er.split(aid, ts, typ, off, np.asarray(bad, dtype=np.int32))
    typ[1] = 3
    with pytest.raises(er.Refused):
        er.split(aid, ts, typ, off, cutoff)
    with pytest.raises(er.Refused):
        er.last_click(typ, off)


def test_capacity_cases_cross_the_lds_buffer():
    """the input builder does what the GPU test relies on: label events one below, at and one above EVAL_LDS_KEYS, and a
    tail with more distinct aids than the buffer holds"""
    sizes = []
    for aids, types, cut in ei.capacity_cases():
        t = np.asarray(types)[cut + 1:]
        sizes.append((int(np.sum((t == 1) | (t == 2))), len(set(np.asarray(aids)[cut + 1:][t == 1].tolist()))))
    m = [s[0] for s in sizes]
    assert {ei.EVAL_LDS_KEYS - 1, ei.EVAL_LDS_KEYS, ei.EVAL_LDS_KEYS + 1} <= set(m)
    assert max(s[1] for s in sizes) > ei.EVAL_LDS_KEYS and max(m) > 2 * ei.EVAL_LDS_KEYS


def test_split_cases_take_every_named_session_and_tail_length():
    """what the GPU split tests claim: every length of LENGTHS occurs as a session length AND as a tail length, and the
    workgroup path (sessions past EVAL_WAVE) sorts exactly 65, 128 and 129 cart / order keys somewhere"""
    sessions = [s for name, case in ei.split_cases().items() for s in case]
    lengths = {len(a) for a, _, _ in sessions}
    tails = {len(a) - c - 1 for a, _, c in sessions if len(a)}
    assert set(ei.LENGTHS) <= lengths and set(ei.LENGTHS) <= tails | {0}, (sorted(lengths), sorted(tails))
    assert 0 in tails
    keys = set()
    for a, t, c in sessions:
        if len(a) > ei.EVAL_WAVE:
            tt = np.asarray(t)[c + 1:]
            keys.add(int(np.sum((tt == 1) | (tt == 2))))
    assert {65, 128, 129} <= keys, sorted(keys)
    on_wave = {len(a) - c - 1 for a, _, c in sessions if ei.EVAL_SHORT < len(a) <= ei.EVAL_WAVE}
    assert {1, 2, 7, 8, 9, 63} <= on_wave
