"""The stable LSD radix sort + CSR of csrc/otto_events.hip through its C-ABI (include/otto_events.h), at the sizes and key
patterns where its tiles, waves, counters and pass skipping change behaviour. Reference: ``numpy.lexsort((seconds,
session))`` in int64 (``edge_inputs.sort_reference``); everything is compared with ``array_equal``.
``tests/test_edge_cases_cpu.py`` checks that every pattern holds the keys its name claims."""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as ei

pytestmark = pytest.mark.gpu


def _sort(dev, sess, ts, div, with_order=True, ws_short=0, n=None):
    """otto_events_sort on the device; host arrays (order, aid, seconds, type, n_sessions, sess_off, sess_id as uint32)."""
    import torch
    from otto_amd import _lib
    n = len(sess) if n is None else n
    rng = np.random.default_rng(n)
    aid = rng.integers(0, 1_855_603, len(sess)).astype(np.int32)
    typ = rng.integers(0, 3, len(sess)).astype(np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_sess, d_ts, d_aid, d_typ = t(sess.view(np.int32)), t(ts), t(aid), t(typ)
    lib = _lib.lib()
    ws_b = int(lib.otto_events_sort_workspace(n))
    ws = torch.empty(max(ws_b, 8), dtype=torch.uint8, device=dev)
    m = max(n, 1)
    o_aid = torch.full((m,), -7, dtype=torch.int32, device=dev)
    o_ts = torch.full((m,), -7, dtype=torch.int32, device=dev)
    o_type = torch.full((m,), 77, dtype=torch.uint8, device=dev)
    o_order = torch.full((m,), -7, dtype=torch.int32, device=dev)
    o_off = torch.full((m + 1,), -7, dtype=torch.int64, device=dev)
    o_id = torch.full((m,), -7, dtype=torch.int32, device=dev)
    ns = C.c_int64(-1)
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(lib.otto_events_sort(p(d_sess), p(d_ts), p(d_aid), p(d_typ), n, int(div), p(o_aid), p(o_ts), p(o_type),
                                        p(o_order) if with_order else C.c_void_p(0), p(o_off), p(o_id), C.byref(ns), p(ws),
                                        ws_b - ws_short, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'otto_events_sort')
        torch.cuda.synchronize(dev)
    h = lambda x: x.cpu().numpy()
    return dict(order=h(o_order).view(np.uint32), aid=h(o_aid), ts=h(o_ts), type=h(o_type), n_sessions=int(ns.value),
                off=h(o_off), sid=h(o_id).view(np.uint32), in_aid=aid, in_type=typ)


def _check(dev, pattern, n):
    sess, ts, div = ei.sort_case(pattern, n)
    order, sec, ids, off = ei.sort_reference(sess, ts, div)
    got = _sort(dev, sess, ts, div)
    S = got['n_sessions']
    assert S == len(ids), (pattern, n, S, len(ids))
    assert np.array_equal(got['order'][:n].astype(np.int64), order), (pattern, n)
    assert np.array_equal(got['aid'][:n], got['in_aid'][order]) and np.array_equal(got['type'][:n], got['in_type'][order])
    assert np.array_equal(got['ts'][:n].astype(np.int64), sec)
    assert np.array_equal(got['off'][:S + 1], off) and np.array_equal(got['sid'][:S].astype(np.int64), ids)
    if pattern in ei.TIE_PATTERNS:            # stability, stated directly: inside one key the input rows keep their order
        key = sess.astype(np.int64)[order] * (1 << 32) + sec
        o = got['order'][:n].astype(np.int64)
        same = key[1:] == key[:-1]
        assert same.any() or n < 8
        assert (o[1:][same] > o[:-1][same]).all(), (pattern, n)
    # the same call without the permutation output
    blind = _sort(dev, sess, ts, div, with_order=False)
    for name in ('aid', 'ts', 'type', 'n_sessions'):
        assert np.array_equal(blind[name], got[name]), name
    assert np.array_equal(blind['off'][:S + 1], off) and np.array_equal(blind['sid'][:S], got['sid'][:S])
    assert (blind['order'].view(np.int32) == -7).all()
    return got


@pytest.mark.parametrize('pattern', ['generic', 'ties3'])
@pytest.mark.parametrize('n', ei.SORT_SIZES)
def test_sort_sizes_next_to_wave_block_tile_and_span(gpu_device, n, pattern):
    _check(gpu_device, pattern, n)


@pytest.mark.parametrize('n', ei.SORT_PATTERN_SIZES)
@pytest.mark.parametrize('pattern', ei.SORT_PATTERNS)
def test_sort_key_patterns(gpu_device, pattern, n):
    got = _check(gpu_device, pattern, n)
    if pattern == 'all_equal':                 # no pass runs: the output is the input
        assert np.array_equal(got['order'][:n], np.arange(n, dtype=np.uint32)) and got['n_sessions'] == 1
    if pattern == 'high_sessions':
        assert got['sid'][:got['n_sessions']].max() == 2 ** 32 - 1
    if pattern == 'ts_extremes':
        assert got['ts'][:n].min() == 0 and got['ts'][:n].max() == 2 ** 31 - 1


def test_sort_argument_and_range_errors(gpu_device):
    """One negative stamp and one of 2^31 seconds are counted by ``k_make_keys`` and refused before any sort pass; a workspace
    one byte short and ``ts_div = 0`` are refused on the host; ``n = 0`` is valid. The negative stamp is -1 ms at
    ``ts_div = 1000``: ``ts // ts_div`` is -1, but the kernel's truncating division made it second 0 and let it through until
    the check was put on the stamp itself."""
    from otto_amd import _lib
    sess, ts, div = ei.sort_case('generic', 5000)
    bad = ts.copy()
    bad[1234] = -1                              # // 1000 floors to -1 second
    with pytest.raises(_lib.OttoError, match='1 timestamps are negative or beyond'):
        _sort(gpu_device, sess, bad, div)
    bad = ts.copy()
    bad[4999] = (2 ** 31) * 1000
    with pytest.raises(_lib.OttoError, match='1 timestamps are negative or beyond'):
        _sort(gpu_device, sess, bad, div)
    with pytest.raises(_lib.OttoError, match='workspace too small'):
        _sort(gpu_device, sess, ts, div, ws_short=1)
    with pytest.raises(_lib.OttoError, match='ts_div must be >= 1'):
        _sort(gpu_device, sess, ts, 0)
    got = _sort(gpu_device, sess[:0], ts[:0], 1000)
    assert got['n_sessions'] == 0 and got['off'][0] == 0
