"""The covisitation pair-expand at every window shape and lane-group size: the streams of tests/expand_inputs.py (every
window's kind proved by tests/test_expand_inputs_cpu.py) run through the component-list kernel and the class kernels, with
and without the time channel and the filter bits, and every window's records are compared with the oracle's per-window
expansion (tests/expand_check.py). Integer work: every comparison is exact.

What says which branch a window took: from a component-list build, the window's runs with sp != 63 and the records of its
runs with sp == 63 equal `classify`'s shared runs and row records (DESIGN.md section 2 restated from its text), and their
sums equal the library's `shared_runs` / `row_records` statistics. A class-kernel build has no shared run.

Unsorted windows: SPEC-COVIS 1 makes sorted stamps a precondition, but both kernels define the result (include/otto_covis.h,
`otto_covis_feed`): the pairs with |ts_i - ts_j| <= max_gap, which is what the oracle computes. The library's `descending-*`,
`reversed-*`, `extremes-descending-*`, `gap0-descending-*` and `gapmax-descending-*` windows pin it."""
import numpy as np
import pytest

import covis_oracle as co
import expand_check
import expand_inputs as ei
from otto_amd.covisitation import spec as cs
from test_covis_gpu import NOFILT, _assert_rows_equal, _build

pytestmark = pytest.mark.gpu

TYPE3 = ('click_weighted', 'cart_weighted', 'order_weighted')
# name: (kinds, options, component-list kernel)
CONFIGS = {
    'lists': (TYPE3, None, True),
    'lists-time': (NOFILT, None, True),
    'class': (TYPE3, {'lists': 0}, False),
    'class-time': (NOFILT, {'lists': 0}, False),
    'class-filters': (cs.ALL_KINDS, None, False),
}
# t0 / t1 of the time weight, set explicitly per max_gap: the stamps 0 and 2^31 - 1 of the `extremes` windows lie outside
# the first range and are clamped to it
TS_RANGE = {ei.GAP: (ei.T0 - 1000, ei.T0 + 4 * ei.GAP), 0: (0, 16), ei.TS_MAX: (0, ei.TS_MAX)}
STREAMS = {w: ei.streams(w) for w in (32, 30)}
_events, _pairs, _classes = {}, {}, {}


def _stream(name, window):
    if (name, window) not in _events:
        _events[(name, window)] = ei.stream(STREAMS[window][name][0], window)
    return _events[(name, window)], STREAMS[window][name][1]


def _want_rows(name, window, kinds, k, ts_range):
    """covis_pairs_python + topk_rows; the pairs of a (stream, window, kind, range) are expanded once."""
    ev, g = _stream(name, window)
    rows = {}
    for kind in kinds:
        key = (name, window, kind, ts_range if kind == 'time_weighted' else None)
        if key not in _pairs:
            sp = co.CovisSpec(window=window, max_gap=g, kinds=(kind,), ts_min=ts_range[0], ts_max=ts_range[1])
            _pairs[key] = co.pairs_dict_to_arrays(co.covis_pairs_python(ev.aid, ev.ts, ev.type, ev.sess_off, sp)[kind])
        rows[kind] = co.topk_rows(*_pairs[key], k=k)
    return rows


def _classify(ev, s, window, g):
    lo, hi = int(ev.sess_off[s]), int(ev.sess_off[s + 1])
    lo = max(lo, hi - window)
    key = (ev.aid[lo:hi].tobytes(), ev.ts[lo:hi].tobytes(), g)
    if key not in _classes:
        _classes[key] = ei.classify(ev.aid[lo:hi], ev.ts[lo:hi], g)
    return _classes[key]


def _check_build(b, ev, window, g, ts_range, lists_kernel, chunks=1):
    """Records of every window vs the oracle, the branch every window took vs `classify`, the sums vs the statistics."""
    names = b.kernel_names()['expand']
    assert ('k_expand_lists' in names) == lists_kernel and ('k_expand<' in names) == (not lists_kernel), names
    sp = co.CovisSpec(window=window, max_gap=g)
    lists, reports = expand_check.check_records(ev, b, sp, ts_range[0], ts_range[1], chunks)
    assert lists == lists_kernel
    for s, r in enumerate(reports):
        if ev.sess_off[s + 1] - ev.sess_off[s] < 2:
            assert (r.pairs, r.shared_runs, r.row_records) == (0, 0, 0)
        elif lists_kernel:
            kind, shared, rows, _ = _classify(ev, s, window, g)
            assert (r.shared_runs, r.row_records) == (shared, rows), f'session {s} ({kind}): shared runs, row records'
        else:
            assert r.shared_runs == 0 and r.row_records == r.pairs, f'session {s}'
    st = b.stats()
    assert st['shared_runs'] == sum(r.shared_runs for r in reports)
    assert st['row_records'] == sum(r.row_records for r in reports)
    assert st['pairs'] == sum(r.pairs for r in reports)
    return reports


def _cases():
    for window, chunks in ((32, 1), (30, 1), (32, 3)):
        for name in STREAMS[window]:
            for cfg in CONFIGS:
                yield pytest.param(name, window, chunks, cfg, id=f'{name}-w{window}-chunks{chunks}-{cfg}')


@pytest.mark.parametrize('name,window,chunks,cfg', list(_cases()))
def test_every_window_matches_oracle_and_takes_its_branch(gpu_device, name, window, chunks, cfg):
    """K1 alone, window by window, then the full pipeline (k = 20) on the same build."""
    kinds, options, lists_kernel = CONFIGS[cfg]
    ev, g = _stream(name, window)
    tr = TS_RANGE[g]
    b, got = _build(ev, gpu_device, kinds=kinds, k=20, window=window, max_gap=g, chunks=chunks, options=options, ts_range=tr)
    _check_build(b, ev, window, g, tr, lists_kernel, chunks)
    _assert_rows_equal(got, _want_rows(name, window, kinds, 20, tr), kinds)


@pytest.mark.parametrize('k', [1, 32])
@pytest.mark.parametrize('cfg', ['lists-time', 'class-time', 'class-filters'])
@pytest.mark.parametrize('name', ['library-g86400', 'library-g0', 'library-gmax'])
def test_rows_of_the_library_at_k(gpu_device, name, cfg, k):
    """finalize rows for k = 1 and 32 (k = 20: above). The gather skips a shared list's `sp` entry and reads the run's time
    extra at tw[slot + sp]: `list-len32-sp31` holds a 32-entry list, sp = 0 .. 31."""
    kinds, options, _ = CONFIGS[cfg]
    ev, g = _stream(name, 32)
    tr = TS_RANGE[g]
    b, got = _build(ev, gpu_device, kinds=kinds, k=k, window=32, max_gap=g, options=options, ts_range=tr)
    _assert_rows_equal(got, _want_rows(name, 32, kinds, k, tr), kinds)


@pytest.mark.parametrize('cfg', ['lists-time', 'class-time'])
def test_time_channel_with_an_empty_ts_range(gpu_device, cfg):
    """ts_min == ts_max: every time extra is 0 (SPEC-COVIS 6), in the lists' sp slots and in every row record."""
    kinds, options, lists_kernel = CONFIGS[cfg]
    ev, g = _stream('library-g86400', 32)
    tr = (ei.T0, ei.T0)
    b, got = _build(ev, gpu_device, kinds=kinds, window=32, max_gap=g, options=options, ts_range=tr)
    _check_build(b, ev, 32, g, tr, lists_kernel)
    _assert_rows_equal(got, _want_rows('library-g86400', 32, kinds, 20, tr), kinds)
    w = got['time_weighted'][2]
    assert len(w) and not (w % co.Q16).any()


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_unsorted_windows_follow_the_gap_rule(gpu_device, cfg):
    """Windows with a descending stamp only: the component-list kernel takes the general loop for each (no shared run) and
    both kernels give the pairs with |ts_i - ts_j| <= max_gap, first valid (i, j) in window order."""
    kinds, options, lists_kernel = CONFIGS[cfg]
    sess = [c.name for c in ei.LIBRARY.values() if c.max_gap == ei.GAP and (np.diff(c.ts.astype(np.int64)) < 0).any()]
    assert len(sess) >= 18 and {ei.LIBRARY[nm].G for nm in sess} == {8, 16, 32}
    ev = ei.stream(sess, 32)
    tr = TS_RANGE[ei.GAP]
    b, _ = _build(ev, gpu_device, kinds=kinds, window=32, max_gap=ei.GAP, options=options, ts_range=tr)
    reports = _check_build(b, ev, 32, ei.GAP, tr, lists_kernel)
    assert all(r.shared_runs == 0 and r.row_records == r.pairs for r in reports) and sum(r.pairs for r in reports) > 0
