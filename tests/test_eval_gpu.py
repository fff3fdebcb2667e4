"""SPEC-EVAL on the device: last click, cutoffs, the split with its three label lists and the hit counts, each against the
NumPy restatement (tests/eval_restatement.py), the hand-worked file or the labels the reference's ``get_labels`` gave
(tests/golden/eval_golden.npz) -- never against the code under test. Everything is integer work: comparisons are exact.

The shapes sit on each side of what csrc/otto_eval.hip stages by: sessions of up to EVAL_SHORT = 8 events run on an
8-lane group, up to EVAL_WAVE = 64 on a wave, longer ones on a workgroup that sorts up to EVAL_LDS_KEYS = 2048 cart /
order events of the tail in LDS and any more in global memory (tests/eval_inputs.py names the three). That the inputs
take every named session length, tail length and key count is itself checked in tests/test_eval_cpu.py."""
import json
import os

import numpy as np
import pytest

import eval_inputs as ei
import eval_restatement as er
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ev(gpu_device):
    import __graft_entry__ as g
    g.build()
    from otto_amd.ranker import evaluate as mod
    return mod


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'eval_hand.json')) as f:
        return json.load(f)


def dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)


def device_events(aid, ts, typ, off, gpu_device):
    from otto_amd.events import DeviceEvents
    return DeviceEvents(dev(aid, gpu_device), dev(ts, gpu_device), dev(typ, gpu_device), dev(off, gpu_device), None, None,
                        int(aid.max()) + 1 if len(aid) else 1)


def check_split(ev, gpu_device, sessions, tag):
    aid, ts, typ, off, cutoff = ei.pack(sessions)
    kept_w, labels_w = er.split(aid, ts, typ, off, cutoff)
    events = device_events(aid, ts, typ, off, gpu_device)
    d_cut = dev(cutoff, gpu_device)
    kept, labels = ev.split(events, d_cut)
    assert np.array_equal(kept.sess_off.cpu().numpy(), kept_w['sess_off']), tag
    assert np.array_equal(kept.aid.cpu().numpy(), kept_w['aid']), tag
    assert np.array_equal(kept.ts.cpu().numpy(), kept_w['ts']), tag
    assert np.array_equal(kept.type.cpu().numpy(), kept_w['typ']), tag
    for name in ev.TYPES:
        o, a = labels[name]
        assert np.array_equal(o.cpu().numpy(), labels_w[name][0]), (tag, name)
        assert np.array_equal(a.cpu().numpy(), labels_w[name][1]), (tag, name)
    for got, want in ((events.aid, aid), (events.ts, ts), (events.type, typ), (events.sess_off, off), (d_cut, cutoff)):
        assert np.array_equal(got.cpu().numpy(), want), f'{tag}: an input was written'
    assert np.array_equal(ev.last_click(events).cpu().numpy(), er.last_click(typ, off)), tag
    return labels_w


@pytest.mark.parametrize('name', sorted(ei.split_cases()))
def test_split_matches_restatement(ev, gpu_device, name):
    check_split(ev, gpu_device, ei.split_cases()[name], name)


def test_split_hand_fixture(ev, gpu_device, hand):
    sessions = [(c['aids'], c['types'], at['cutoff']) for c in hand['split'] for at in c['at']]
    want = [at for c in hand['split'] for at in c['at']]
    aid, ts, typ, off, cutoff = ei.pack(sessions)
    kept, labels = ev.split(device_events(aid, ts, typ, off, gpu_device), dev(cutoff, gpu_device))
    for name in ev.TYPES:
        o, a = labels[name]
        assert er.lists_csr(o.cpu().numpy(), a.cpu().numpy()) == [at[name] for at in want], name
    assert np.diff(kept.sess_off.cpu().numpy()).tolist() == [at['cutoff'] + 1 for at in want]
    types = [c['types'] for c in hand['last_click']]
    _, _, typ, off, _ = ei.pack([(t, t, 0) for t in types])
    got = ev.last_click(device_events(typ.astype(np.int32), typ.astype(np.int32), typ, off, gpu_device))
    assert got.tolist() == [c['last_click'] for c in hand['last_click']]


def test_split_reproduces_reference_labels_at_every_index(ev, gpu_device):
    """every session of the golden file once per index: the device labels are what get_labels gave there"""
    g = np.load(os.path.join(GOLDEN, 'eval_golden.npz'))
    aid, typ, off = g['aid'], g['typ'], g['sess_off']
    sessions, where = [], []
    for s in range(len(off) - 1):
        b, e = int(off[s]), int(off[s + 1])
        for i in range(e - b):
            sessions.append((aid[b:e], typ[b:e], i))
            where.append(b + i)
    a2, ts2, t2, o2, cut = ei.pack(sessions)
    _, labels = ev.split(device_events(a2, ts2, t2, o2, gpu_device), dev(cut, gpu_device))
    where = np.asarray(where)
    o, a = (x.cpu().numpy() for x in labels['clicks'])
    click = np.full(len(where), -1, dtype=np.int64)
    click[np.diff(o) == 1] = a
    assert np.array_equal(click, g['click'][where])
    for name, key in (('carts', 'cart'), ('orders', 'order')):
        o, a = (x.cpu().numpy() for x in labels[name])
        assert np.array_equal(np.diff(o), np.diff(g[f'{key}_off'])[where]), name
        want = np.concatenate([g[f'{key}_aid'][g[f'{key}_off'][p]:g[f'{key}_off'][p + 1]] for p in where])
        assert np.array_equal(a, want), name


@pytest.mark.parametrize('S', ei.S_SIZES)
def test_cutoffs_match_restatement(ev, gpu_device, S):
    aid, ts, typ, off, _ = ei.pack(ei.sized_case(S, seed=3) + ei.edge_cases()[:S])
    events = device_events(aid, ts, typ, off, gpu_device)
    for seed in (0, 7, 2 ** 63 + 5):
        want, without = er.cutoffs(typ, off, seed)
        got, n_without = ev.cutoffs(events, seed)
        assert np.array_equal(got.cpu().numpy(), want) and n_without == without, (S, seed)
    assert np.array_equal(events.type.cpu().numpy(), typ)
    if S:
        kept, labels = ev.split(events, got)                          # a cutoff the library made is one it accepts
        assert np.array_equal(kept.sess_off.cpu().numpy(), er.split(aid, ts, typ, off, want)[0]['sess_off'])


def test_out_of_range_type_and_cutoff_are_refused(ev, gpu_device):
    from otto_amd._lib import OttoError
    sessions = ei.sized_case(65, seed=9)
    aid, ts, typ, off, cutoff = ei.pack(sessions)
    n = np.diff(off)
    for where, value in ((int(np.flatnonzero(n > 0)[0]), None), (int(np.flatnonzero(n > 70)[0]), None), (int(np.flatnonzero(n > 0)[-1]), -1),
                         (int(np.flatnonzero(n == 0)[0]), 1)):
        bad = cutoff.copy()
        bad[where] = n[where] if value is None else value
        with pytest.raises(er.Refused):
            er.split(aid, ts, typ, off, bad)
        events, d_bad = device_events(aid, ts, typ, off, gpu_device), dev(bad, gpu_device)
        with pytest.raises(OttoError, match=r'code -22.*cutoff'):
            ev.split(events, d_bad)
        assert np.array_equal(d_bad.cpu().numpy(), bad) and np.array_equal(events.aid.cpu().numpy(), aid)
    for where in (0, int(off[int(np.flatnonzero(n > 70)[0])]) + 69, len(typ) - 1):
        bad_t = typ.copy()
        bad_t[where] = 3
        events = device_events(aid, ts, bad_t, off, gpu_device)
        with pytest.raises(OttoError, match=r'code -22.*typ'):
            ev.split(events, dev(cutoff, gpu_device))
        with pytest.raises(OttoError, match=r'code -22.*typ'):
            ev.last_click(events)
        with pytest.raises(OttoError, match=r'code -22.*typ'):
            ev.cutoffs(events, 1)
        assert np.array_equal(events.type.cpu().numpy(), bad_t) and np.array_equal(events.aid.cpu().numpy(), aid)
    check_split(ev, gpu_device, sessions, 'after refusals')            # the library is still usable afterwards


def check_hits(ev, gpu_device, lab, rows, preds, tag, cap=20, label_session=None, pred_session=None, mask=None):
    want_h, want_d = er.hits(lab, rows, label_session, pred_session, cap)
    d = lambda x: None if x is None else dev(np.asarray(x), gpu_device)
    l_off, l_aid = ei.to_csr(lab)
    h, dn, tot = ev.hits((dev(l_off, gpu_device), dev(l_aid, gpu_device)), preds, d(label_session), d(pred_session), cap=cap, mask=d(mask))
    assert np.array_equal(h.cpu().numpy(), want_h), tag
    assert np.array_equal(dn.cpu().numpy(), want_d), tag
    assert tot == er.totals(want_h, want_d, mask), tag
    return want_h, want_d


@pytest.mark.parametrize('k', (1, 20, 64))
@pytest.mark.parametrize('S', ei.S_SIZES)
def test_hits_padded_rows(ev, gpu_device, S, k):
    lab, pred, n = ei.padded_case(S, k)
    d_pred, d_n = dev(pred.reshape(S, k), gpu_device), dev(n, gpu_device)
    mask = (np.arange(S) % 3 == 0).astype(np.uint8)
    for cap in (20, 0, 5):
        check_hits(ev, gpu_device, lab, er.rows_padded(pred, n), (d_pred, d_n), (S, k, cap, 'n'), cap=cap, mask=mask)
        check_hits(ev, gpu_device, lab, er.rows_padded(pred), d_pred, (S, k, cap, 'padded only'), cap=cap)


@pytest.mark.parametrize('S', ei.S_SIZES)
def test_hits_csr_rows(ev, gpu_device, S):
    lab, rows = ei.csr_case(S)
    off, flat = ei.to_csr(rows)
    preds = (dev(off, gpu_device), dev(flat, gpu_device))
    for cap in (20, 0):
        check_hits(ev, gpu_device, lab, rows, preds, (S, cap), cap=cap, mask=np.ones(S, dtype=np.uint8))


def test_hits_hand_fixture(ev, gpu_device, hand):
    for case in hand['hits']:
        lab = [case['labels']]
        k = max(len(case['pred']), 1)
        pred = np.full((1, k), -1, dtype=np.int32)
        pred[0, :len(case['pred'])] = case['pred']
        h, d, _ = ev.hits(tuple(dev(x, gpu_device) for x in ei.to_csr(lab)), dev(pred, gpu_device), cap=case['cap'])
        assert (h.tolist(), d.tolist()) == ([case['hits']], [case['denom']]), case
        off, flat = ei.to_csr([case['pred']])
        h, d, _ = ev.hits(tuple(dev(x, gpu_device) for x in ei.to_csr(lab)), (dev(off, gpu_device), dev(flat, gpu_device)), cap=case['cap'])
        assert (h.tolist(), d.tolist()) == ([case['hits']], [case['denom']]), case


@pytest.mark.parametrize('form', ('padded', 'csr'))
def test_hits_session_alignment_and_masks(ev, gpu_device, form):
    from otto_amd._lib import OttoError
    S = 257
    if form == 'padded':
        lab, pred, n = ei.padded_case(S, 20, seed=1)
        rows = er.rows_padded(pred, n)
        make = lambda take: (dev(pred[take], gpu_device), dev(n[take], gpu_device))
    else:
        lab, rows = ei.csr_case(S, seed=1)
        make = lambda take: tuple(dev(x, gpu_device) for x in ei.to_csr([rows[p] for p in take]))
    ids, take = ei.subset_ids(S)
    assert 0 < len(take) < S
    masks = (np.zeros(S, np.uint8), np.ones(S, np.uint8), (np.arange(S) % 2).astype(np.uint8))
    everyone = np.arange(S)
    for mask in masks:
        # a strict subset of the label sessions, all of them, and position-aligned rows
        check_hits(ev, gpu_device, lab, [rows[p] for p in take], make(take), (form, 'subset'), label_session=ids, pred_session=ids[take], mask=mask)
        a = check_hits(ev, gpu_device, lab, rows, make(everyone), (form, 'equal'), label_session=ids, pred_session=ids, mask=mask)
        b = check_hits(ev, gpu_device, lab, rows, make(everyone), (form, 'aligned'), mask=mask)
        assert np.array_equal(a[0], b[0])
    # ids that are positions, without label_session
    check_hits(ev, gpu_device, lab, [rows[p] for p in take], make(take), (form, 'positions'), pred_session=take.astype(np.int32))
    # one foreign session
    foreign = ids[take].copy()
    gap = int(np.flatnonzero(np.diff(ids) > 1)[0])
    foreign[np.searchsorted(foreign, ids[gap] + 1):][:1] = ids[gap] + 1
    assert not np.isin(foreign, ids).all() and np.all(np.diff(foreign) > 0)
    l_off, l_aid = (dev(x, gpu_device) for x in ei.to_csr(lab))
    with pytest.raises(er.Refused):
        er.hits(lab, [rows[p] for p in take], ids, foreign)
    with pytest.raises(OttoError, match=r'code -22.*not among the label sessions'):
        ev.hits((l_off, l_aid), make(take), dev(ids, gpu_device), dev(foreign, gpu_device))
    with pytest.raises(OttoError, match=r'code -22.*ascending'):
        ev.hits((l_off, l_aid), make(take), dev(ids, gpu_device), dev(ids[take][::-1].copy(), gpu_device))
    check_hits(ev, gpu_device, lab, rows, make(everyone), (form, 'after refusals'))


def test_recall_and_evaluate_equal_host_metric(ev, gpu_device):
    from otto_amd import metrics
    S = 257
    tops, labels, want = {}, {}, {}
    for i, name in enumerate(ev.TYPES):
        lab, pred, n = ei.padded_case(S, 20, seed=10 + i)
        tops[name] = dev(pred, gpu_device)
        labels[name] = tuple(dev(x, gpu_device) for x in ei.to_csr(lab))
        rows = [[v for v in r if v >= 0] for r in er.rows_padded(pred)]
        want[name] = (metrics.recall_at_20(rows, lab), rows, lab)
        assert ev.recall_at_20(labels[name], tops[name]) == want[name][0]
    hold = (np.arange(S) % 4 == 1)
    out = ev.evaluate(tops, labels, holdout=dev(hold.astype(np.uint8), gpu_device))
    for name in ev.TYPES:
        assert out[name] == want[name][0]
        rows, lab = want[name][1:]
        assert out['holdout'][name] == metrics.recall_at_20([rows[s] for s in np.flatnonzero(hold)], [lab[s] for s in np.flatnonzero(hold)])
    assert out['weighted'] == metrics.weighted_recall(*(want[n][0] for n in ev.TYPES))


def test_non_device_tensors_are_refused(ev, gpu_device):
    import torch
    from otto_amd._lib import OttoError
    from otto_amd.events import DeviceEvents
    aid, ts, typ, off, cutoff = ei.pack(ei.sized_case(5))
    host = DeviceEvents(*(torch.from_numpy(x) for x in (aid, ts, typ, off)), None, None, 10)
    for call in (lambda: ev.last_click(host), lambda: ev.cutoffs(host, 1), lambda: ev.split(host, torch.from_numpy(cutoff))):
        with pytest.raises(OttoError, match='no CPU fallback'):
            call()
    with pytest.raises(OttoError, match='no CPU fallback'):
        ev.hits((torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)), torch.zeros((1, 20), dtype=torch.int32))
