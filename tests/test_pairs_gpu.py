"""The aid-pair builders of csrc/otto_pairs.hip (include/otto_pairs.h) against the pandas restatement
``oracle/pairs_oracle.py``, on event streams built directly as ``DeviceEvents`` so that the CSR holds what the frame
ingest never produces: empty sessions, dt on every side of the time predicate, a per-pair mean of exactly 0.5, the
smallest and largest aid in the packed key. Rows are compared as int64 with ``array_equal`` after sorting by (x1, x2).
``tests/test_edge_cases_cpu.py`` checks that the streams hold what they claim."""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as ei
import pairs_oracle as po

pytestmark = pytest.mark.gpu


def _device_events(dev, aid, ts, off, n_aids=ei.MAX_AID + 1):
    import torch
    from otto_amd.events import DeviceEvents
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return DeviceEvents(t(aid), t(ts), t(np.zeros(len(aid), dtype=np.uint8)), t(off), t(np.arange(len(off) - 1)), None, n_aids)


def _got(cols):
    return ei.pair_rows([c.cpu().numpy() for c in cols])


def _want(frame):
    return ei.pair_rows([frame['x1'].to_numpy(), frame['x2'].to_numpy(), frame['target'].to_numpy()])


@pytest.mark.parametrize('agg', ['mean', 'max'])
@pytest.mark.parametrize('hours', [1, 24, 0.5])
def test_time_pairs_with_empty_sessions_and_dt_edges(gpu_device, hours, agg):
    """Sessions of 0 (start, middle, two in a row, end), 1, 2, 3, 64, 65 and 300 events; dt = max_dt, max_dt + 1, 0, -1, one day
    and 25 h, for one shared pair of aids and for one pair each; label means of exactly 0.5 (-> 1) and of 2 / 6 (-> 0); aid 0 and
    aid 1,855,602 on either side of the key."""
    from otto_amd.matrix_factorization.data import build_aid_pairs_device
    max_dt = int(round(hours * 3600))
    aid, ts, off, fr = ei.stream_to_frame(ei.time_edge_sessions(max_dt))
    assert (np.diff(off) == 0).sum() == 5
    want = _want(po.pairs_time(fr, hour_difference=hours, target_aggregation=agg))
    got = _got(build_aid_pairs_device(_device_events(gpu_device, aid, ts, off), 'time', hour_difference=hours, target_aggregation=agg,
                                      sample_frac=1.0))
    assert got.shape == want.shape and np.array_equal(got, want)
    lab = {(int(a), int(b)): int(c) for a, b, c in got}
    assert lab[(ei.AID_DT_EACH, ei.AID_DT_EACH + 1)] == 1 and lab[(ei.AID_DT_EACH + 2, ei.AID_DT_EACH + 3)] == 0      # dt = max_dt, max_dt + 1
    assert lab[(0, ei.MAX_AID)] == 1 and lab[(ei.MAX_AID, 0)] == 0
    if agg == 'mean':
        assert lab[ei.AID_HALF] == 1 and lab[ei.AID_BELOW_HALF] == 0


def test_time_pairs_at_a_size_of_many_sort_workgroups(gpu_device):
    """40,000 sessions of up to 60 events: 4,831,576 raw slots = 295 sort workgroups, slot bases above 2^22; slots of equal
    aids carry PAIR_NONE keys (all ones), so all eight radix passes of the value sort run. Full sample, mean and max. The
    oracle takes about 3 s per aggregation for this size."""
    from otto_amd.matrix_factorization.data import build_aid_pairs_device
    aid, ts, off, fr = ei.stream_to_frame(ei.random_sessions(**ei.TIME_BIG))
    assert ei.raw_time_slots(off) > 2 ** 22
    ev = _device_events(gpu_device, aid, ts, off, n_aids=ei.TIME_BIG['n_aids'])
    for agg in ('mean', 'max'):
        want = _want(po.pairs_time(fr, hour_difference=0.5, target_aggregation=agg))
        got = _got(build_aid_pairs_device(ev, 'time', hour_difference=0.5, target_aggregation=agg, sample_frac=1.0))
        assert got.shape == want.shape and np.array_equal(got, want), agg
        assert 0 < got[:, 2].mean() < 1


@pytest.mark.parametrize('frac,seed', [(0.15, 42), (0.5, 7)])
def test_sampled_time_pairs_equal_the_oracle_on_the_same_draw(gpu_device, frac, seed):
    """The sampled path (its CSR holds empty sessions on every real call) against the oracle: the documented draw --
    a device generator seeded with ``seed``, ``torch.rand(E) < sample_frac`` -- is reproduced here and handed to the
    oracle as ``row_mask``."""
    import torch
    from otto_amd.matrix_factorization.data import build_aid_pairs_device
    aid, ts, off, fr = ei.stream_to_frame(ei.random_sessions(3000, 400, 40, 0.15, seed=5))
    gen = torch.Generator(device=gpu_device)
    gen.manual_seed(seed)
    keep = (torch.rand(len(aid), device=gpu_device, generator=gen) < frac).cpu().numpy()
    kept_per_session = np.add.reduceat(np.r_[keep, False].astype(np.int64), off[:-1])
    assert (kept_per_session == 0).any() and 0.8 * frac < keep.mean() < 1.2 * frac
    ev = _device_events(gpu_device, aid, ts, off, n_aids=400)
    for agg in ('mean', 'max'):
        want = _want(po.pairs_time(fr, hour_difference=0.5, target_aggregation=agg, row_mask=keep))
        got = _got(build_aid_pairs_device(ev, 'time', hour_difference=0.5, target_aggregation=agg, sample_frac=frac, seed=seed))
        assert len(want) > 100 and got.shape == want.shape and np.array_equal(got, want), agg


def test_diff_pairs_hand_built_stream(gpu_device):
    """Sessions of 1, 2 and 3 events, one repeated aid, rows with x2 == x3 and x1 == x3, shuffle keys 0 and 2^31 - 1, the pair
    (10, 11) positive in one session and negative in another (positive wins); then all keys equal: the permutation is the
    identity, x3 == x1 on every row, and no pair survives."""
    from otto_amd.matrix_factorization.data import build_aid_pairs_device
    sessions, keys = ei.diff_edge_stream()
    aid, ts, off, fr = ei.stream_to_frame(sessions)
    ev = _device_events(gpu_device, aid, ts, off, n_aids=100)
    want = _want(po.pairs_diff(fr, shuffle_keys=keys))
    got = _got(build_aid_pairs_device(ev, 'diff', shuffle_keys=keys))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert [10, 11, 1] in got.tolist() and [10, 11, 0] not in got.tolist()
    got = _got(build_aid_pairs_device(ev, 'diff', shuffle_keys=np.full(len(aid), 9, dtype=np.uint64)))
    assert got.shape == (0, 3) and len(po.pairs_diff(fr, shuffle_keys=np.full(len(aid), 9))) == 0


def test_diff_pairs_with_extreme_keys_and_aids(gpu_device):
    """Random short sessions whose shuffle keys are drawn from {0, 1, 2^31 - 2, 2^31 - 1} (ties everywhere: the stable order
    decides) and whose aids include 0 and 1,855,602."""
    from otto_amd.matrix_factorization.data import build_aid_pairs_device
    rng = np.random.default_rng(8)
    sessions = ei.random_sessions(5000, 60, 12, 0.3, seed=9)
    sessions = [(np.where(a == 59, ei.MAX_AID, a), t) for a, t in sessions]
    aid, ts, off, fr = ei.stream_to_frame(sessions)
    keys = np.array([0, 1, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.uint64)[rng.integers(0, 4, len(aid))]
    want = _want(po.pairs_diff(fr, shuffle_keys=keys))
    got = _got(build_aid_pairs_device(_device_events(gpu_device, aid, ts, off), 'diff', shuffle_keys=keys))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert (got[:, 0] == 0).any() and (got[:, 1] == ei.MAX_AID).any() and 0 < got[:, 2].mean() < 1


def test_pair_builder_argument_errors(gpu_device):
    import torch
    from otto_amd import _lib
    lib = _lib.lib()
    aid, ts, off, _ = ei.stream_to_frame(ei.random_sessions(50, 30, 8, 0.3, seed=2))
    E, S = len(aid), len(off) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    d_aid, d_ts, d_off = t(aid), t(ts), t(off)
    raw = ei.raw_time_slots(off)
    cap = max(raw, 2 * E) + 2
    ws_b = int(lib.otto_pairs_workspace(cap))
    ws = torch.empty(ws_b, dtype=torch.uint8, device=gpu_device)
    x1, x2, tg = (torch.empty(cap, dtype=torch.int64, device=gpu_device) for _ in range(3))
    rows = C.c_int64()
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    with torch.cuda.device(gpu_device):
        with pytest.raises(_lib.OttoError, match='raw must be 2 \\* events'):
            _lib.check(lib.otto_pairs_diff(p(d_aid), p(d_aid), p(d_off), S, 2 * E - 1, p(x1), p(x2), p(tg), C.byref(rows), p(ws), ws_b, stream), 'diff')
        with pytest.raises(_lib.OttoError, match='workspace too small'):
            _lib.check(lib.otto_pairs_diff(p(d_aid), p(d_aid), p(d_off), S, 2 * E, p(x1), p(x2), p(tg), C.byref(rows), p(ws),
                                           int(lib.otto_pairs_workspace(2 * E)) - 1, stream), 'diff')
        with pytest.raises(_lib.OttoError, match='workspace too small'):
            _lib.check(lib.otto_pairs_time(p(d_aid), p(d_ts), p(d_off), S, raw, 3600, 0, p(x1), p(x2), p(tg), C.byref(rows), p(ws),
                                           int(lib.otto_pairs_workspace(raw)) - 1, stream), 'time')
        with pytest.raises(_lib.OttoError, match='Invalid target aggregation'):
            _lib.check(lib.otto_pairs_time(p(d_aid), p(d_ts), p(d_off), S, raw, 3600, 2, p(x1), p(x2), p(tg), C.byref(rows), p(ws), ws_b, stream), 'time')
