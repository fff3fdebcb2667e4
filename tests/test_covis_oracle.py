"""CPU tests of the covisitation oracle: hand-computed micro-sessions, the two
restatements against each other, the committed golden fixture, top-k tie-breaking."""
import os

import numpy as np
import pytest

import covis_oracle as co
from conftest import GOLDEN
from otto_amd.synth import generate_sessions

T = 1_660_000_000
Q = co.Q16


def _micro():
    # session 1: aids 10,20,10,30 (click, click, cart, order); session 2: one pair more than a day
    # apart (no contribution); session 3: aids 20,30,20 (cart, cart, click)
    aid = np.array([10, 20, 10, 30, 20, 30, 20, 30, 20], dtype=np.uint32)
    ts = np.array([0, 5, 9, 12, 1000, 1000 + 86401, 2000, 2010, 2020], dtype=np.int32) + T
    typ = np.array([0, 0, 1, 2, 0, 0, 1, 1, 0], dtype=np.uint8)
    off = np.array([0, 4, 6, 9], dtype=np.int64)
    return aid, ts, typ, off


# hand-derived (see DESIGN.md "Worked example"): unit weights, multiply by 65536
HAND = {
    'click_weighted': {(10, 20): 1, (10, 30): 3, (20, 10): 1, (20, 30): 3 + 6, (30, 10): 1, (30, 20): 1 + 6},
    'cart_weighted': {(10, 20): 1, (10, 30): 6, (20, 10): 1, (20, 30): 6 + 9, (30, 10): 1, (30, 20): 1 + 9},
    'order_weighted': {(10, 20): 1, (10, 30): 6, (20, 10): 1, (20, 30): 6 + 3, (30, 10): 1, (30, 20): 1 + 3},
    'click_cart': {(20, 10): 1, (20, 30): 1},
    'click_order': {(10, 30): 1, (20, 30): 1},
    'cart_order': {(10, 30): 1, (30, 10): 1, (20, 30): 1, (30, 20): 1},
    'click_click': {(10, 20): 1, (20, 10): 1},
}
# time_weighted: t0 = T, t1 = T + 87401; extra(ts) = (196608 * (ts - t0)) // 87401
HAND_TIME = {(10, 20): Q, (10, 30): Q, (20, 10): Q + 11, (20, 30): (Q + 11) + (Q + 4498),
             (30, 10): Q + 26, (30, 20): (Q + 26) + (Q + 4521)}


def test_hand_computed_micro_sessions():
    aid, ts, typ, off = _micro()
    for fn in (co.covis_pairs_python, lambda *a: {k: dict(zip(zip(v[0].tolist(), v[1].tolist()), v[2].tolist()))
                                                  for k, v in co.covis_pairs_numpy(*a).items()}):
        got = fn(aid, ts, typ, off, co.CovisSpec())
        for kind, want in HAND.items():
            assert got[kind] == {p: w * Q for p, w in want.items()}, kind
        assert got['time_weighted'] == HAND_TIME


@pytest.mark.parametrize('seed,n_aids', [(1, 200), (2, 30), (3, 5000)])
def test_python_and_numpy_restatements_agree(seed, n_aids):
    ev = generate_sessions(250, n_aids=n_aids, seed=seed)
    for window, gap in ((30, 86400), (4, 300)):
        sp = co.CovisSpec(window=window, max_gap=gap)
        st = {}
        a = co.covis_pairs_python(ev.aid, ev.ts, ev.type, ev.sess_off, sp)
        b = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, sp, stats=st)
        for k in co.ALL_KINDS:
            pa = co.pairs_dict_to_arrays(a[k])
            assert all(np.array_equal(p, q) for p, q in zip(pa, b[k])), k
        n_all = sum(len(co.expand_window_python(ev.aid, ev.ts, ev.type, int(ev.sess_off[s]), int(ev.sess_off[s + 1]), sp))
                    for s in range(ev.n_sessions))
        assert st['P'] == n_all


def test_expand_window_order_and_attributes():
    aid, ts, typ, off = _micro()
    rows = co.expand_window_python(aid, ts, typ, 0, 4, co.CovisSpec(), ('click_cart', 'click_order', 'cart_order', 'click_click'), T, T + 87401)
    # rows by first position of x (10, 20, 30), columns by first position of y
    assert [(r[0], r[1]) for r in rows] == [(10, 20), (10, 30), (20, 10), (20, 30), (30, 10), (30, 20)]
    assert [r[2] for r in rows] == [0, 2, 0, 2, 0, 0]                       # type_y of the first valid pair
    assert [r[3] for r in rows] == [0b1000, 0b0110, 0b1001, 0b0010, 0b0100, 0]   # filter bits
    assert [r[4] for r in rows] == [0, 0, 11, 11, 26, 26]                   # time extra of the first pair's x


def test_golden_fixture_is_reproduced():
    g = np.load(os.path.join(GOLDEN, 'covis_golden.npz'))
    got = co.covis_topk_numpy(g['aid'], g['ts'], g['type'], g['sess_off'], co.CovisSpec(), k=20)
    for k in co.ALL_KINDS:
        for name, arr in zip('xyw', got[k]):
            assert np.array_equal(arr, g[f'{k}_{name}']), (k, name)


def test_topk_tie_break_and_truncation():
    x = np.array([1, 1, 1, 1, 2], dtype=np.uint32)
    y = np.array([9, 3, 5, 7, 1], dtype=np.uint32)
    W = np.array([5, 7, 7, 5, 1], dtype=np.uint64)
    rx, ry, rw = co.topk_rows(x, y, W, k=3)
    assert ry.tolist() == [3, 5, 7, 1] and rw.tolist() == [7, 7, 5, 1] and rx.tolist() == [1, 1, 1, 2]
    assert co.wgt_float32(np.array([65536 * 3 + 32768], dtype=np.uint64)).tolist() == [3.5]


def test_window_is_the_session_tail():
    aid = np.arange(40, dtype=np.uint32)
    ts = (T + np.arange(40)).astype(np.int32)
    typ = np.zeros(40, dtype=np.uint8)
    off = np.array([0, 40], dtype=np.int64)
    got = co.covis_pairs_numpy(aid, ts, typ, off, co.CovisSpec(window=30, kinds=('click_click',)))['click_click']
    assert got[0].min() == 10 and len(got[0]) == 30 * 29


def test_c_restatement_matches_numpy_and_hand_values():
    """oracle/covis_oracle.c (the timed cpu_baseline) against the NumPy oracle and the hand-derived micro-sessions."""
    import __graft_entry__ as g
    g._run(['make', 'all'], os.path.join(g.ROOT, 'oracle'))
    import covis_oracle_c as coc
    assert coc.available()
    ev = generate_sessions(1500, n_aids=300, seed=9)
    want = co.covis_topk_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(), k=20)
    st = {}
    co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(kinds=('click_click',)), stats=st)
    got = coc.covis_topk_c(ev.aid, ev.ts, ev.type, ev.sess_off, ev.n_aids, co.ALL_KINDS, k=20, threads=4)
    assert got['P'] == st['P']
    for kind in co.ALL_KINDS:
        for a_, b_ in zip(got[kind], want[kind]):
            assert np.array_equal(a_, b_), kind
    aid, ts, typ, off = _micro()
    got = coc.covis_topk_c(aid, ts, typ, off, 31, ('cart_weighted', 'time_weighted', 'cart_order'), k=20, threads=1)
    d = dict(zip(zip(got['cart_weighted'][0].tolist(), got['cart_weighted'][1].tolist()), got['cart_weighted'][2].tolist()))
    assert d == {p: w * Q for p, w in HAND['cart_weighted'].items()}
    d = dict(zip(zip(got['time_weighted'][0].tolist(), got['time_weighted'][1].tolist()), got['time_weighted'][2].tolist()))
    assert d == HAND_TIME


def test_time_extra_is_clamped_to_the_given_ts_range():
    """SPEC-COVIS 6: ts_min / ts_max come from the caller; an event outside [t0, t1] counts as t0 or t1, so every time
    extra lies in [0, 3 * 65536]. The three restatements (Python loops, NumPy, C) and expand_window_python agree, by hand
    on one pair and on generated sessions with events on both sides of the range."""
    import __graft_entry__ as g
    g._run(['make', 'all'], os.path.join(g.ROOT, 'oracle'))
    import covis_oracle_c as coc
    aid = np.array([1, 2, 3, 4], dtype=np.uint32)
    ts = np.array([0, 1, 300, 301], dtype=np.int32) + T
    off = np.array([0, 2, 4], dtype=np.int64)
    sp = co.CovisSpec(kinds=('time_weighted',), ts_min=T + 100, ts_max=T + 200)
    # (1, 2) at ts T < t0: no extra; (3, 4) at T + 300 > t1: the full 3 * 65536
    want = {(1, 2): Q, (2, 1): Q, (3, 4): 4 * Q, (4, 3): 4 * Q}
    assert co.covis_pairs_python(aid, ts, np.zeros(4, np.uint8), off, sp)['time_weighted'] == want
    x, y, w = co.covis_pairs_numpy(aid, ts, np.zeros(4, np.uint8), off, sp)['time_weighted']
    assert dict(zip(zip(x.tolist(), y.tolist()), w.tolist())) == want
    assert [r[4] for r in co.expand_window_python(aid, ts, np.zeros(4, np.uint8), 2, 4, sp, (), T + 100, T + 200)] == [3 * Q] * 2
    ev = generate_sessions(600, n_aids=200, seed=19)
    q1, q3 = (int(v) for v in np.quantile(ev.ts, [0.25, 0.75]))
    for t0, t1 in ((q1, q3), (q1, q1)):
        sp = co.CovisSpec(ts_min=t0, ts_max=t1)
        want = co.covis_topk_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, sp, k=20)
        py = co.covis_pairs_python(ev.aid, ev.ts, ev.type, ev.sess_off, sp)['time_weighted']
        x, y, w = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, sp)['time_weighted']
        assert dict(zip(zip(x.tolist(), y.tolist()), w.tolist())) == py
        got = coc.covis_topk_c(ev.aid, ev.ts, ev.type, ev.sess_off, ev.n_aids, co.ALL_KINDS, k=20, threads=2, ts_min=t0, ts_max=t1)
        for kind in co.ALL_KINDS:
            for a_, b_ in zip(got[kind], want[kind]):
                assert np.array_equal(a_, b_), kind
        if t0 == t1:
            assert (w % Q == 0).all()                    # no extra without a time span


def test_c_restatement_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """SURVEY.md section 5 (CPU-side sanitizers; never on the GPU box): `make -C oracle asan` builds covis_oracle.c with
    -fsanitize=address,undefined behind a file-driven main; it runs the hand-derived micro-sessions, random sessions with
    window 32 (the table bound of the expansion), an empty stream and length-1 sessions, with 1 and 4 threads. A sanitizer
    report or a difference between the two runs fails the process; its rows must equal the NumPy restatement's."""
    import subprocess
    oracle_dir = os.path.join(os.path.dirname(os.path.abspath(co.__file__)))
    r = subprocess.run(['make', '-C', oracle_dir, 'asan'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    exe = os.path.join(oracle_dir, '_build', 'covis_oracle_asan')
    from covis_oracle_c import covis_topk_c  # noqa: F401  (same kind encoding as the ctypes wrapper)
    kinds = co.ALL_KINDS
    group, param = [], []
    for kd in kinds:
        if kd == 'time_weighted':
            group.append(0); param += [0, 0, 0]
        elif kd in co.TYPE_WEIGHTS:
            group.append(1); param += list(co.TYPE_WEIGHTS[kd])
        else:
            m = co.FILTER_MASKS[kd]
            group.append(2); param += [sum(1 << (tx * 3 + ty) for tx in range(3) for ty in range(3) if m[tx][ty]), 0, 0]
    ev = generate_sessions(300, n_aids=40, seed=9, max_len=70)
    lone = (np.array([3, 4, 5], dtype=np.uint32), np.array([T, T + 1, T + 2], dtype=np.int32), np.zeros(3, dtype=np.uint8),
            np.array([0, 1, 2, 3], dtype=np.int64))                       # three sessions of one event: no pair
    empty = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    cases = [(_micro(), 31, 30, 86400, 20), ((ev.aid, ev.ts, ev.type, ev.sess_off), 40, 32, 86400, 20),
             ((ev.aid, ev.ts, ev.type, ev.sess_off), 40, 5, 600, 3), (lone, 8, 30, 86400, 20), (empty, 8, 30, 86400, 20)]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    for ci, ((aid, ts, typ, off), n_aids, window, gap, k) in enumerate(cases):
        t0, t1 = (int(ts.min()), int(ts.max())) if len(ts) else (0, 0)
        src, dst = tmp_path / f'case{ci}.bin', tmp_path / f'out{ci}.bin'
        with open(src, 'wb') as f:
            f.write(np.array([len(off) - 1, len(aid), n_aids, window, gap, t0, t1, len(kinds), k], dtype=np.int64).tobytes())
            f.write(np.array(group, dtype=np.int32).tobytes())
            f.write(np.array(param, dtype=np.int32).tobytes())
            for a in (off.astype(np.int64), aid.astype(np.uint32), ts.astype(np.int32), typ.astype(np.uint8)):
                f.write(a.tobytes())
        r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
        assert r.returncode == 0 and 'runtime error' not in r.stdout and 'AddressSanitizer' not in r.stdout, f'case {ci}:\n{r.stdout}'
        raw = open(dst, 'rb').read()
        nk = len(kinds)
        P = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
        o = 8
        oy = np.frombuffer(raw, dtype=np.uint32, count=nk * n_aids * k, offset=o).reshape(nk, n_aids, k); o += oy.nbytes
        ow = np.frombuffer(raw, dtype=np.uint64, count=nk * n_aids * k, offset=o).reshape(nk, n_aids, k); o += ow.nbytes
        on = np.frombuffer(raw, dtype=np.int32, count=nk * n_aids, offset=o).reshape(nk, n_aids)
        st = {}
        want = co.covis_topk_numpy(aid, ts, typ, off, co.CovisSpec(window=window, max_gap=gap), k=k, stats=st) if len(aid) else None
        assert P == (st['P'] if want is not None else 0)
        for j, kd in enumerate(kinds):
            valid = np.arange(k)[None, :] < on[j][:, None]
            x = np.broadcast_to(np.arange(n_aids, dtype=np.uint32)[:, None], (n_aids, k))[valid]
            if want is None:
                assert x.size == 0
                continue
            assert np.array_equal(x, want[kd][0]) and np.array_equal(oy[j][valid], want[kd][1]) and np.array_equal(ow[j][valid], want[kd][2]), (ci, kd)
