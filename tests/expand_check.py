"""Per-window decoder and comparer of the raw pair-expand output (``CovisBuilder.copy_records()``), shared by
tests/test_covis_gpu.py and tests/test_covis_expand_edges_gpu.py.

Slot layout restated from ``otto_covis_feed`` (csrc/otto_covis.hip): every fed chunk appends, to the record slots, n (n - 1)
pair slots per window and -- from the component-list kernel only -- n list slots per window behind ALL the chunk's pair
slots; to the run slots, one slot per window event. A run descriptor is ``len | slot << 8 | sp << 48``; sp != 63: the run
reads a shared component list that holds the run's own aid at position sp (not a pair; its slot of the time channel carries
the run's time extra); sp == 63: a private row, every record a pair with its own time extra.
"""
from dataclasses import dataclass

import numpy as np

import covis_oracle as co

SP_NONE = 63
RUN_X_EMPTY = 0xFFFFFFFF


def chunk_bounds(n_sessions, chunks):
    """Session bounds of the chunks as test_covis_gpu._build feeds them."""
    return np.linspace(0, n_sessions, chunks + 1).astype(np.int64)


@dataclass
class Layout:
    nwin: np.ndarray        # [S] window events (0: no window)
    run0: np.ndarray        # [S] first run slot of the window
    pair0: np.ndarray       # [S] first pair slot of the window
    list0: np.ndarray       # [S] first list slot of the window (lists only)
    pair_slots: int         # record slots in all
    tail_events: int


def layout(sess_off, window, lists, chunks=1):
    L = np.diff(np.asarray(sess_off, dtype=np.int64))
    n = np.minimum(L, window)
    nwin = np.where(n >= 2, n, 0)
    S = len(nwin)
    run0, pair0, list0 = (np.zeros(S, np.int64) for _ in range(3))
    rec_used = run_used = 0
    b = chunk_bounds(S, chunks)
    for c in range(chunks):
        lo, hi = int(b[c]), int(b[c + 1])
        w = nwin[lo:hi]
        pairs, evs = int((w * (w - 1)).sum()), int(w.sum())
        pair0[lo:hi] = rec_used + np.r_[0, np.cumsum(w * (w - 1))][:-1]
        list0[lo:hi] = rec_used + pairs + np.r_[0, np.cumsum(w)][:-1]
        run0[lo:hi] = run_used + np.r_[0, np.cumsum(w)][:-1]
        rec_used += pairs + (evs if lists else 0)
        run_used += evs
    return Layout(nwin, run0, pair0, list0, rec_used, run_used)


@dataclass
class WindowReport:
    pairs: int
    shared_runs: int        # runs with sp != 63
    row_records: int        # sum of the lengths of the runs with sp == 63


_oracle_cache = {}


def oracle_window(ev, s, spec, filter_kinds, t0, t1):
    """expand_window_python of session s; equal windows (the library repeats them inside a stream) are expanded once."""
    lo, hi = int(ev.sess_off[s]), int(ev.sess_off[s + 1])
    lo = max(lo, hi - spec.window)
    key = (ev.aid[lo:hi].tobytes(), ev.ts[lo:hi].tobytes(), ev.type[lo:hi].tobytes(), spec.max_gap, tuple(filter_kinds), t0, t1)
    if key not in _oracle_cache:
        _oracle_cache[key] = co.expand_window_python(ev.aid, ev.ts, ev.type, lo, hi, spec, filter_kinds, t0, t1)
    return _oracle_cache[key]


def check_window(s, lay, lists, rec, tw, run_x, run_desc, want):
    """Decode the runs of window s, check their geometry and compare the records, as a set of (x, y, type_y, filter bits,
    time extra), with `want` (the oracle's tuples): each ordered pair at most once, whatever runs it is spread over."""
    n = int(lay.nwin[s])
    r0, p0, l0 = int(lay.run0[s]), int(lay.pair0[s]), int(lay.list0[s])
    got = []
    used = set()
    shared_runs = row_records = 0
    for r in range(r0, r0 + n):
        d = int(run_desc[r])
        ln, off, spos = d & 0x3F, (d >> 8) & ((1 << 40) - 1), (d >> 48) & 63
        if not ln:
            assert d == 0 and run_x[r] == RUN_X_EMPTY, f'session {s}: an empty run has desc == 0 and run_x == 0xFFFFFFFF'
            continue
        x = int(run_x[r])
        if spos != SP_NONE:
            assert lists and l0 <= off and off + ln <= l0 + n, f'session {s}: a shared list outside the window\'s list slots'
            assert spos < ln and int(rec[off + spos]) & 0x3FFFFFF == x, f'session {s}: sp does not point at the run\'s own entry'
            shared_runs += 1
        else:
            assert p0 <= off and off + ln <= p0 + n * (n - 1), f'session {s}: a private row outside the window\'s pair slots'
            row_records += ln
        for t in range(ln):
            if t == spos:
                continue
            rc = int(rec[off + t])
            if spos == SP_NONE:
                assert off + t not in used, f'session {s}: a private slot is used twice'
                used.add(off + t)
            e = 0 if tw is None else int(tw[off + (spos if spos != SP_NONE else t)])
            got.append((x, rc & 0x3FFFFFF, (rc >> 26) & 3, rc >> 28, e))
    if tw is None:
        want = [w[:4] + (0,) for w in want]
    assert len(set(g[:2] for g in got)) == len(got), f'session {s}: a pair occurs twice'
    assert sorted(got) == sorted(want), f'session {s}'
    return WindowReport(len(want), shared_runs, row_records)


def check_records(ev, builder, spec, t0, t1, chunks=1):
    """Every window of the stream against the oracle. Returns (lists, [WindowReport per session]); `lists` says that the
    records carry list slots (the component-list kernel wrote them)."""
    rec, tw, run_x, run_desc = builder.copy_records()
    plain = layout(ev.sess_off, spec.window, False, chunks)
    lists = len(rec) == plain.pair_slots + plain.tail_events
    lay = layout(ev.sess_off, spec.window, lists, chunks)
    st = builder.stats()
    assert st['tail_events'] == lay.tail_events == len(run_x) == len(run_desc) and st['pair_slots'] == lay.pair_slots == len(rec)
    fk = builder.filter_kinds
    reports = []
    for s in range(ev.n_sessions):
        want = oracle_window(ev, s, spec, fk, t0, t1) if lay.nwin[s] else []
        reports.append(check_window(s, lay, lists, rec, tw, run_x, run_desc, want))
    return lists, reports
