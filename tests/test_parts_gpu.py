"""Part files back to resident top-k arrays on the device (SPEC-ROWS, include/otto_rows.h; otto_amd/covisitation/parts.py):
``rows_to_topk`` against the NumPy restatement (tests/parts_restatement.py) on every run shape around the 64-row waves, its
refusals, canaries around the three outputs and the calling contract; the round trip build -> part files (pyarrow-written
and device-written, delta-coded) -> ``load_matrix`` -> ``candidate_lookup`` against the resident matrices."""
import ctypes as C

import numpy as np
import pytest
import torch

import parts_restatement as P

pytestmark = pytest.mark.gpu
CANARY = 0x5A


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want):
    for g, w, name in zip(got, want, 'ywn'):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, g.dtype)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name


def _run(dev, rows, n_aids, k, work=None):
    from otto_amd.covisitation import parts
    return parts.rows_to_topk(*[_dev(a, dev) for a in rows], n_aids, k, work=work)


def _case(k, seed=0):
    lengths = P.edge_lengths(k)
    n_aids = 2 * len(lengths) + 7
    rng = np.random.default_rng(seed)
    aids = np.sort(rng.choice(np.arange(1, n_aids - 1), size=len(lengths), replace=False))      # aid 0 and n_aids - 1 have no rows
    return P.rows(lengths, n_aids, seed, aids), n_aids


@pytest.mark.parametrize('k', [1, 15, 20, 64])
def test_rows_to_topk_equals_the_restatement(gpu_device, k):
    rows, n_aids = _case(k)
    x = rows[0]
    heads = np.flatnonzero(np.r_[True, x[1:] != x[:-1]])
    lens = np.diff(np.r_[heads, len(x)])
    assert lens.max() == k and len(x) > 128
    assert any(h % 64 == 0 and h for h in heads)                               # a run starts exactly on a 64-row boundary
    if k > 1:
        assert any(h // 64 != (h + n - 1) // 64 for h, n in zip(heads, lens))       # a run crosses one
        assert any((h + k - 1) % 64 == 0 and n == k for h, n in zip(heads, lens))   # a look-back of k - 1
    want = P.rows_to_topk(*rows, n_aids, k)
    assert want[2][0] == 0 and want[2][-1] == 0 and (want[2] == 0).sum() > 2
    _same(_run(gpu_device, rows, n_aids, k), want)


def test_empty_and_single_row(gpu_device):
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    for n_aids in (0, 5):
        _same(_run(gpu_device, empty, n_aids, 15), P.rows_to_topk(*empty, n_aids, 15))
    one = (np.array([3], np.int32), np.array([4], np.int32), np.array([0.5], np.float32))
    _same(_run(gpu_device, one, 5, 15), P.rows_to_topk(*one, 5, 15))
    got = _run(gpu_device, one, 5, 15)
    assert got[0][3].tolist() == [4] + [-1] * 14 and got[2].tolist() == [0, 0, 0, 1, 0]


def _refused(dev, rows, n_aids, k):
    from otto_amd import _lib
    with pytest.raises(P.Refused) as want:
        P.rows_to_topk(*rows, n_aids, k)
    with pytest.raises(_lib.OttoError) as e:
        _run(dev, rows, n_aids, k)
    assert f'row {want.value.row}: {P.REASONS[want.value.code]}' in str(e.value), (str(e.value), str(want.value))
    return want.value


@pytest.mark.parametrize('k', [1, 15, 64])
def test_a_run_of_k_plus_1_is_refused_naming_its_row(gpu_device, k):
    for start in (0, 64 - k, 64, 70, 130):                                      # inside one wave, ending on a boundary, starting on one, across
        lengths = [1] * start + [k + 1] + [1] * 40 + [k + 2]
        rows = P.rows(lengths, len(lengths) + 3, seed=start)
        bad = _refused(gpu_device, rows, len(lengths) + 3, k)
        assert (bad.row, bad.code) == (start + k, P.RUN)
    rows = P.rows([200], 9, seed=1)                                             # one run far longer than k, over several waves
    assert _refused(gpu_device, rows, 9, k).row == k


def test_order_and_range_refusals(gpu_device):
    k, n_aids = 15, 500
    rows = P.rows([3] * 100, n_aids, seed=2)
    for col, row, value, code in ((0, 130, -1, P.AID_X), (0, 299, n_aids, P.AID_X), (1, 64, n_aids, P.AID_Y), (1, 5, -1, P.AID_Y),
                                  (1, 63, 2 ** 31 - 1, P.AID_Y)):
        bad = [a.copy() for a in rows]
        bad[col][row] = value
        got = _refused(gpu_device, bad, n_aids, k)
        assert (got.row, got.code) == (row, code)
    bad = [a.copy() for a in rows]
    bad[0][192:195] = rows[0][100]                                               # a run that steps down, on a wave's first row
    got = _refused(gpu_device, bad, n_aids, k)
    assert (got.row, got.code) == (192, P.ORDER)
    bad = [a.copy() for a in rows]                                               # several violations: the smallest row wins, then its first reason
    bad[1][250], bad[0][200], bad[1][200] = -5, n_aids + 1, -5
    got = _refused(gpu_device, bad, n_aids, k)
    assert (got.row, got.code) == (200, P.AID_X)
    _same(_run(gpu_device, rows, n_aids, k), P.rows_to_topk(*rows, n_aids, k))            # the clean rows still pass


def _raw_call(dev, d_rows, n_aids, k, outs, work):
    """otto_rows_topk on caller-owned outputs (views between canaries)"""
    from otto_amd import _lib
    job = _lib.RowsJob(_lib.ptr(d_rows[0]), _lib.ptr(d_rows[1]), _lib.ptr(d_rows[2]), int(d_rows[0].numel()), _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                       _lib.ptr(outs[2]), n_aids, k, 0, _lib.ptr(work), int(work.numel()), _lib.stream(dev))
    err = np.full(2, -1, dtype=np.int64)
    with torch.cuda.device(dev):
        rc = _lib.lib().otto_rows_topk(C.byref(job), err.ctypes.data_as(C.c_void_p))
    return rc, err


def test_canaries_around_the_outputs(gpu_device):
    """the three outputs lie inside larger buffers; nothing outside them is written, with clean rows and with refused ones"""
    dev, k = gpu_device, 15
    rows, n_aids = _case(k, seed=3)
    want = P.rows_to_topk(*rows, n_aids, k)
    bad = [a.copy() for a in rows]
    bad[0][70] = n_aids + 5                                                     # a store at this aid would land behind y and w
    bad[1][10] = -1
    pad = 4096
    work = torch.empty(256, dtype=torch.uint8, device=dev)
    for r, clean in ((rows, True), (bad, False)):
        bufs = [torch.full((pad + n * 4 + pad,), CANARY, dtype=torch.uint8, device=dev) for n in (n_aids * k, n_aids * k, n_aids)]
        outs = [b[pad:len(b) - pad].view(dt) for b, dt in zip(bufs, (torch.int32, torch.float32, torch.int32))]
        rc, err = _raw_call(dev, [_dev(a, dev) for a in r], n_aids, k, outs, work)
        torch.cuda.synchronize(dev)
        for b in bufs:
            h = b.cpu().numpy()
            assert (h[:pad] == CANARY).all() and (h[-pad:] == CANARY).all()
        if clean:
            assert rc == 0 and err.tolist() == [-1, 0]
            _same([outs[0].view(n_aids, k), outs[1].view(n_aids, k), outs[2]], want)
        else:
            assert rc == -22 and err.tolist() == [10, P.AID_Y]


def _contract_rows(seed, scale=1):
    rng = np.random.default_rng(seed)
    n_aids = 3000 * scale
    lengths = rng.permutation(np.arange(n_aids) % 16)                            # one multiset of run lengths: the seed moves them
    return P.rows(lengths[lengths > 0], n_aids, seed, np.flatnonzero(lengths > 0)), n_aids


def test_reused_scratch_and_repetition(gpu_device):
    (real, n_aids), (decoy, _), (decoy2, n2) = _contract_rows(1), _contract_rows(2), _contract_rows(2, 2)
    want = P.rows_to_topk(*real, n_aids, 15)
    work = torch.empty(4096, dtype=torch.uint8, device=gpu_device)
    _same(_run(gpu_device, real, n_aids, 15, work), want)
    _same(_run(gpu_device, real, n_aids, 15, work), want)                       # twice in a row
    _same(_run(gpu_device, decoy, n_aids, 15, work), P.rows_to_topk(*decoy, n_aids, 15))
    _same(_run(gpu_device, real, n_aids, 15, work), want)                       # after a decoy of the same size
    _same(_run(gpu_device, decoy2, n2, 15, work), P.rows_to_topk(*decoy2, n2, 15))
    _same(_run(gpu_device, real, n_aids, 15, work), want)                       # after one of twice the size


def test_side_stream_with_late_inputs(gpu_device):
    """The inputs hold a decoy; on a side stream a delay is followed by the copies of the real rows and by the call. An
    entry point that launched on another stream than the job's would read the decoy."""
    from otto_amd.covisitation import parts
    dev = gpu_device
    (real, n_aids), (decoy, _) = _contract_rows(1), _contract_rows(2)
    assert len(real[0]) == len(decoy[0])
    k = 15
    want = P.rows_to_topk(*real, n_aids, k)
    assert not np.array_equal(want[0], P.rows_to_topk(*decoy, n_aids, k)[0])
    torch.cuda._sleep(1_000_000)                             # the first launch of the delay kernel is not the measured one
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                               # about 30 ms
    d_in = [_dev(a, dev) for a in decoy]
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in real]
    work = torch.empty(4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        for t, p in zip(d_in, pinned):
            t.copy_(p, non_blocking=True)
        got = parts.rows_to_topk(*d_in, n_aids, k, work=work)
    side.synchronize()
    print(f'rows: the delay in front of the late inputs took {e0.elapsed_time(e1):.1f} ms')
    assert e0.elapsed_time(e1) >= 10.0
    _same(got, want)


def test_host_refusals(gpu_device):
    from otto_amd import _lib
    from otto_amd.covisitation import parts
    x = torch.zeros(4, dtype=torch.int32, device=gpu_device)
    w = torch.zeros(4, dtype=torch.float32, device=gpu_device)
    for k in (0, 65):
        with pytest.raises(ValueError, match='k must be'):
            parts.rows_to_topk(x, x, w, 10, k)
    with pytest.raises(ValueError, match='aid_y'):
        parts.rows_to_topk(x, x[:3], w, 10, 15)
    with pytest.raises(ValueError, match='wgt'):
        parts.rows_to_topk(x, x, x, 10, 15)
    with pytest.raises(_lib.OttoError, match='ROCm'):
        parts.rows_to_topk(x.cpu(), x.cpu(), w.cpu(), 10, 15)


# ---- the round trip: build -> part files -> load_matrix -> candidate_lookup ---------------------------------------------------
@pytest.fixture(scope='module')
def built(gpu_device, tmp_path_factory):
    """a small synthetic build (3,000 sessions), its resident matrices, and its part files from both writers"""
    from otto_amd.covisitation import builder
    from otto_amd.covisitation.engine import CovisBuilder, topk_to_rows, topk_to_device_rows
    from otto_amd.covisitation.spec import REFERENCE_KINDS
    from otto_amd.synth import generate_sessions
    dev = gpu_device
    ev = generate_sessions(3000, n_aids=1500, seed=7)
    feed = [_dev(ev.aid.astype(np.int32), dev), _dev(ev.ts, dev), _dev(ev.type, dev), _dev(ev.sess_off, dev)]
    b = CovisBuilder(ev.n_aids, kinds=REFERENCE_KINDS, ts_min=int(ev.ts.min()), ts_max=int(ev.ts.max()), device=dev)
    b.feed(*feed)
    mats = b.finalize(k=20)
    dirs = {w: tmp_path_factory.mktemp(w) for w in ('pyarrow', 'device')}
    res = {w: {k: {} for k in (15, 20)} for w in dirs}
    for k in (15, 20):
        for kind in REFERENCE_KINDS:
            y, w, n = mats[kind]
            cut = (y[:, :k].contiguous(), w[:, :k].contiguous(), torch.clamp(n, max=k))
            res['pyarrow'][k][kind] = topk_to_rows(*cut)
            res['device'][k][kind] = topk_to_device_rows(*cut)
    for prefix, kind, rows, n_parts in builder.part_sets('validation', res['pyarrow']):
        builder.write_parts(dirs['pyarrow'], prefix, kind, rows, n_parts, ev.n_aids)
    for prefix, kind, rows, n_parts in builder.part_sets('validation', res['device']):
        builder.write_device_parts(dirs['device'], prefix, kind, rows, n_parts, ev.n_aids)
    return ev, feed, mats, dirs


@pytest.mark.parametrize('writer', ['pyarrow', 'device'])
def test_load_matrix_equals_the_resident_arrays(gpu_device, built, writer):
    from otto_amd import parquet
    from otto_amd.covisitation import builder, parts
    from otto_amd.covisitation.spec import REFERENCE_KINDS, Q16
    ev, _, mats, dirs = built
    if writer == 'device':
        _, pages = parquet.page_table(str(dirs[writer] / 'top_15_click_weighted_0.pqt'), ['aid_x', 'aid_y'])
        assert {p.encoding for v in pages.values() for p in v} == {5}
    rows = 0
    for prefix, k in (('top_15', 15), ('top', 20)):
        for kind in REFERENCE_KINDS:
            co = kind == 'cart_order'
            n_parts = ((builder.TOP15_CART_ORDER_PARTS if co else builder.TOP15_PARTS)['validation'] if k == 15
                       else builder.TOP_CART_ORDER_PARTS if co else builder.TOP_PARTS)
            y, w, n = parts.load_matrix(dirs[writer], prefix, kind, n_parts, ev.n_aids, k, gpu_device)
            ry, rw, rn = mats[kind]
            want_n = torch.clamp(rn, max=k)
            valid = torch.arange(k, device=gpu_device)[None, :] < want_n[:, None]
            want_y = torch.where(valid, ry[:, :k].to(torch.int32), torch.full_like(y, -1))
            want_w = torch.where(valid, (rw[:, :k].double() / Q16).float(), torch.zeros_like(w))
            assert torch.equal(n, want_n) and torch.equal(y, want_y), (prefix, kind)
            assert torch.equal(w.view(torch.int32), want_w.view(torch.int32)), (prefix, kind)
            rows += int(n.sum())
    assert rows > 10000


@pytest.mark.parametrize('writer', ['pyarrow', 'device'])
def test_candidate_lookup_over_loaded_matrices(gpu_device, built, writer):
    from otto_amd.covisitation import parts
    from otto_amd.covisitation.candidates import candidate_lookup, CLICK_RECIPE, CART_RECIPE
    ev, feed, mats, dirs = built
    loaded = parts.load_matrices(dirs[writer], 'validation', 'top_15', ev.n_aids, gpu_device)
    guessed = parts.load_matrices(dirs[writer], 'validation', 'top_15', None, gpu_device)
    assert set(loaded) == set(mats) and guessed['click_weighted'][0].shape[0] <= ev.n_aids
    resident = {kind: (y[:, :15].contiguous(), w[:, :15].contiguous(), torch.clamp(n, max=15)) for kind, (y, w, n) in mats.items()}
    off = feed[3][:501].contiguous()
    e = int(off[-1])
    for recipe in (CLICK_RECIPE, CART_RECIPE):
        want = candidate_lookup(feed[0][:e].contiguous(), feed[2][:e].contiguous(), off, resident, recipe)
        got = candidate_lookup(feed[0][:e].contiguous(), feed[2][:e].contiguous(), off, loaded, recipe)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert int(got[2].sum()) > 1000
    top = parts.load_matrices(dirs[writer], 'validation', 'top', ev.n_aids, gpu_device)
    assert top['cart_order'][0].shape == (ev.n_aids, 20)
