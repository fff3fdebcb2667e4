"""The Snappy encoder kernels of csrc/otto_snappy.hip through ``otto_amd.snappy`` and ``otto_amd.parquet_write`` against the
restatement of SPEC-SNAPPY (tests/snappy_restatement.py): the device bytes are the restatement's bytes, pyarrow and the
project's own decoders read them, nothing outside a stream's extent is written, and the entry points keep the contract of
tests/contract_cases.py (side stream, late inputs, reused scratch, repetition)."""
import importlib
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_write_restatement as R
import snappy_inputs
import snappy_restatement as S

pytestmark = pytest.mark.gpu
INPUTS = snappy_inputs.inputs()
CANARY = 0xA5
_WANT = {}


def want(name):
    """The restatement's stream of a named input, computed once for all tests."""
    if name not in _WANT:
        _WANT[name] = S.compress(INPUTS[name])
    return _WANT[name]


@pytest.fixture(scope='module')
def sn():
    import __graft_entry__ as g
    g.build()
    from otto_amd import snappy
    return snappy


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bytes(b, dev):
    return _dev(np.frombuffer(b, dtype=np.uint8).copy(), dev)


@pytest.mark.parametrize('name', list(INPUTS))
def test_device_stream_equals_the_restatement(sn, gpu_device, name):
    out = sn.compress(_bytes(INPUTS[name], gpu_device))
    assert out.cpu().numpy().tobytes() == want(name)


def _packed(names, rng, lead):
    """The named inputs in one buffer at odd offsets with gaps of junk between them."""
    parts, off, at = [bytes(rng.integers(0, 256, lead, dtype=np.uint8))], [], lead
    for n in names:
        off.append(at)
        gap = int(rng.choice([0, 1, 3, 17]))
        parts += [INPUTS[n], bytes(rng.integers(0, 256, gap, dtype=np.uint8))]
        at += len(INPUTS[n]) + gap
    return b''.join(parts), np.array(off, dtype=np.int64), np.array([len(INPUTS[n]) for n in names], dtype=np.int64)


def test_many_streams_at_odd_offsets_with_guards(sn, gpu_device):
    import torch
    from otto_amd import parquet
    rng = np.random.default_rng(4)
    names = [n for n in INPUTS if len(INPUTS[n]) <= 70000]
    names = [names[i] for i in rng.permutation(len(names))]
    buf, src_off, src_len = _packed(names, rng, lead=3)
    assert any(o % 2 for o in src_off.tolist()) and any(o % 4 == 2 for o in src_off.tolist())
    d_in = _bytes(buf, gpu_device)
    out0, sizes = sn.compress_extents(d_in, src_off, src_len)               # back to back, a fresh tensor
    assert sizes.tolist() == [len(want(n)) for n in names]
    assert out0.cpu().numpy().tobytes() == b''.join(want(n) for n in names)
    gaps = rng.choice([1, 2, 5, 13], size=len(names))
    dst = np.cumsum(np.r_[7, sizes[:-1] + gaps[:-1]])
    out = torch.full((int(dst[-1] + sizes[-1]) + 9,), CANARY, dtype=torch.uint8, device=gpu_device)
    got, sizes2 = sn.compress_extents(d_in, src_off, src_len, out=out, dst_off=dst)
    assert got is out and sizes2.tolist() == sizes.tolist() and any(d % 2 for d in dst.tolist())
    h = out.cpu().numpy()
    guard = np.ones(len(h), dtype=bool)
    for n, d in zip(names, dst.tolist()):
        assert h[d:d + len(want(n))].tobytes() == want(n), n
        guard[d:d + len(want(n))] = False
    assert guard.sum() == 7 + 9 + int(gaps[:-1].sum()) and (h[guard] == CANARY).all()
    # the device decoder reads every stream back, at odd destinations as well
    back, status = parquet.snappy_decompress(out, dst, sizes, src_len, dst_off=src_off,
                                             out=torch.full((len(buf),), CANARY, dtype=torch.uint8, device=gpu_device))
    assert (status == 0).all()
    b = back.cpu().numpy()
    for n, o in zip(names, src_off.tolist()):
        assert b[o:o + len(INPUTS[n])].tobytes() == INPUTS[n], n


@pytest.mark.parametrize('name', ['column_session', 'column_aid', 'column_ts', 'column_type', 'column_wgt', 'text_like', 'random_131073',
                                  'zeros_65537', 'repeat_straddles_cut', 'random_0'])
def test_round_trip_through_the_device_decoder(sn, gpu_device, name):
    from otto_amd import parquet
    x = INPUTS[name]
    z = sn.compress(_bytes(x, gpu_device))
    assert z.numel() <= sn.compressed_bound(len(x))
    assert pa.Codec('snappy').decompress(z.cpu().numpy().tobytes(), decompressed_size=len(x), asbytes=True) == x if x else z.cpu().tolist() == [0]
    assert parquet._snappy_host(z.cpu().numpy().tobytes(), len(x)) == x
    back, status = parquet.snappy_decompress(z, [0], [z.numel()], [len(x)])
    assert status.tolist() == [0] and back.cpu().numpy().tobytes() == x


def test_refusals_write_nothing(sn, gpu_device):
    import torch
    from otto_amd import _lib
    x, y = INPUTS['column_type'][:70000], INPUTS['column_wgt'][:70000]
    d_x, d_y = _bytes(x, gpu_device), _bytes(y, gpu_device)
    off, ln = [1, 30000, 69000], [29000, 39000, 1000]
    work = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu_device)
    job = sn.DeviceJob(d_x, off, ln, work)
    nb = job.plan().tolist()
    assert nb == [len(S.compress(x[o:o + k])) for o, k in zip(off, ln)]
    out = torch.full((sum(nb) + 64,), CANARY, dtype=torch.uint8, device=gpu_device)
    untouched = lambda: bool((out.cpu().numpy() == CANARY).all())
    good = [0, nb[0], nb[0] + nb[1]]
    with pytest.raises(_lib.OttoError, match='overlap'):
        job.emit([0, nb[0] - 1, nb[0] + nb[1]], out)
    with pytest.raises(_lib.OttoError, match='overlap'):
        job.emit([5, 5 + nb[0], 5], out)
    with pytest.raises(_lib.OttoError, match='leave out_bytes'):
        job.emit([0, nb[0], out.numel() - nb[2] + 1], out)
    with pytest.raises(_lib.OttoError, match='leave out_bytes'):
        job.emit([-1, nb[0], nb[0] + nb[1]], out)
    with pytest.raises(_lib.OttoError, match='leave out_bytes'):             # too small an out
        job.emit(good, out[:sum(nb) - 1])
    assert untouched()
    other = sn.DeviceJob(d_y, off, ln, work)                  # same extents, same scratch, another buffer: another job
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):
        other.emit(good, out)
    moved = sn.DeviceJob(d_x, [1, 30000, 68000], ln, work)
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):
        moved.emit(good, out)
    fewer = sn.DeviceJob(d_x, off[:2], ln[:2], work)
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):
        fewer.emit(good[:2], out)
    assert untouched()
    for bad_off, bad_len in (([1, 30000, 69001], ln), ([-1, 30000, 69000], ln), (off, [29000, 39000, -1]), ([70001, 0, 0], [0, 1, 1])):
        with pytest.raises(_lib.OttoError, match='leave the input|src_len'):      # a source extent outside the buffer
            sn.DeviceJob(d_x, bad_off, bad_len, work)
        with pytest.raises(_lib.OttoError, match='leave the input|src_len'):
            sn.compress_extents(d_x, bad_off, bad_len, out=out, dst_off=good)
    with pytest.raises(ValueError, match='work'):
        sn.DeviceJob(d_x, off, ln, work[:256])
    with pytest.raises(ValueError, match='one entry per stream'):
        sn.compress_extents(d_x, off, ln[:2])
    with pytest.raises(ValueError, match='uint8'):
        sn.compress_extents(d_x.to(torch.int32), off, ln)
    with pytest.raises(_lib.OttoError, match='no CPU fallback'):
        sn.compress_extents(d_x.cpu(), off, ln)
    assert untouched()
    job.emit(good, out)                                       # the plan is still there
    h = out.cpu().numpy()
    assert h[:sum(nb)].tobytes() == b''.join(S.compress(x[o:o + k]) for o, k in zip(off, ln)) and (h[sum(nb):] == CANARY).all()


# ---- Parquet files ----------------------------------------------------------------------------------------------------------
EDGE = dict(page_rows=256, row_group_rows=512)


@pytest.mark.parametrize('compression', ['snappy', {'wgt': 'snappy'}, {'aid_x': 'snappy', 'ts': 'snappy', 'wgt': None}])
def test_encode_tables_with_compression(gpu_device, tmp_path, compression):
    from otto_amd import parquet, parquet_write as pw
    rng = np.random.default_rng(3)
    n = 3000
    cols = {'aid_x': np.repeat(np.sort(rng.choice(R.N_AIDS, size=n // 15, replace=False)), 15).astype(np.int32),
            'aid_y': rng.integers(0, R.N_AIDS, size=n).astype(np.int32),
            'ts': (1_661_724_000_000 + np.cumsum(rng.integers(1, 5000, n))).astype(np.int64),
            'wgt': (rng.integers(1, 2 ** 12, size=n) / 16).astype(np.float32)}
    enc = {'aid_x': 'delta', 'aid_y': 'delta'}
    cuts = [0, 0, 1, 1300, 2990, 3000, 3000]                 # empty files first and last: every chunk is one page of 0 values
    d_cols = {k: _dev(v, gpu_device) for k, v in cols.items()}
    images = pw.encode_tables(d_cols, cuts, enc, compression=compression, **EDGE)
    host = pw.encode_tables_host(cols, cuts, enc, body=R.page_body, compression=compression, compress=S.compress, **EDGE)
    plain = pw.encode_tables(d_cols, cuts, enc, **EDGE)
    assert [bytes(p) for p in plain] == [bytes(p) for p in pw.encode_tables_host(cols, cuts, enc, body=R.page_body, **EDGE)]
    assert sum(map(len, images)) < sum(map(len, plain))
    paths = []
    for i, (image, h, lo, hi) in enumerate(zip(images, host, cuts, cuts[1:])):
        assert bytes(image) == bytes(h), i
        t = pq.read_table(pa.BufferReader(bytes(image)))
        for name, a in cols.items():
            got = t.column(name).to_numpy()
            assert got.dtype == a.dtype and np.array_equal(got, a[lo:hi]), (i, name)
        paths.append(str(tmp_path / f'part_{i}.pqt'))
        with open(paths[-1], 'wb') as f:
            f.write(image)
    back = parquet.read_columns(paths, list(cols), gpu_device, floats=True)
    for (name, a), t in zip(cols.items(), back):
        got = t.cpu().numpy()
        assert got.dtype == a.dtype and got.tobytes() == a[:3000].tobytes(), name
    sizes = pw.write_tables([tmp_path / f'w_{i}.pqt' for i in range(6)], d_cols, cuts, enc, compression=compression, **EDGE)
    assert sizes == [len(i) for i in images] and open(tmp_path / 'w_3.pqt', 'rb').read() == bytes(images[3])


def test_builder_device_write_with_snappy_gives_the_same_matrices(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setenv('OTTO_ROOT', str(tmp_path))
    import otto_amd.settings as settings
    importlib.reload(settings)
    import torch
    from otto_amd.covisitation import builder, parts
    from otto_amd.synth import generate_sessions
    monkeypatch.setattr(builder, 'settings', settings)
    fr = generate_sessions(1200, n_aids=400, seed=8).to_frame()
    splits = tmp_path / 'data' / 'splits'
    splits.mkdir(parents=True)
    cut = int(np.searchsorted(fr['session'].to_numpy(), fr['session'].iloc[len(fr) // 2]))
    fr.iloc[:cut].to_parquet(splits / 'train.parquet')
    fr.iloc[cut:].to_parquet(splits / 'val.parquet')
    out = tmp_path / 'data' / 'covisitation' / 'validation'
    with pytest.raises(ValueError, match='--device-write'):
        builder.main(['validation', '--compression', 'snappy'])
    builder.main(['validation', '--device-write'])
    names = sorted(os.listdir(out))
    load = lambda: {w: parts.load_matrices(out, 'validation', w, 400, gpu_device) for w in ('top_15', 'top')}
    first, first_frames, first_bytes = load(), {n: pd.read_parquet(out / n) for n in names}, sum(os.path.getsize(out / n) for n in names)
    for n in names:
        os.remove(out / n)
    builder.main(['validation', '--device-write', '--compression', 'snappy'])
    assert sorted(os.listdir(out)) == names and len(names) > 60
    assert sum(os.path.getsize(out / n) for n in names) < first_bytes
    for n in names:
        md = pq.ParquetFile(out / n).metadata
        assert [md.row_group(0).column(j).compression for j in range(3)] == ['UNCOMPRESSED', 'UNCOMPRESSED', 'SNAPPY'], n
        pd.testing.assert_frame_equal(pd.read_parquet(out / n), first_frames[n])
    second = load()
    for w in first:
        assert list(second[w]) == list(first[w])
        for kind in first[w]:
            for a, b in zip(first[w][kind], second[w][kind]):
                assert a.dtype == b.dtype and bool(torch.equal(a, b)), (w, kind)


def test_chunk_writer_with_snappy(gpu_device, tmp_path):
    import torch
    from otto_amd import events
    from otto_amd.utilities import split_dataset_writer_parquet as sw
    rng = np.random.default_rng(5)
    sess = np.sort(rng.choice(np.r_[0:30, 36:42, 60:70], size=30, replace=False)).astype(np.int32)
    session = np.repeat(sess, rng.integers(1, 9, size=len(sess)))
    n = len(session)
    frame = pd.DataFrame({'session': session, 'aid': rng.integers(0, R.N_AIDS, size=n).astype(np.int32),
                          'ts': (1659304800000 + rng.permutation(n)).astype(np.int64), 'type': rng.integers(0, 3, size=n).astype(np.uint8)})
    frame = frame.iloc[rng.permutation(n)].reset_index(drop=True)
    splits = [tmp_path / 'train.parquet', tmp_path / 'val.parquet']
    frame.iloc[:n // 2].to_parquet(splits[0])
    frame.iloc[n // 2:].to_parquet(splits[1])
    for encoding in ('plain', 'delta'):
        plain = sw.write_chunks(splits, tmp_path / f'{encoding}_none', gpu_device, encoding, chunk=13)
        packed = sw.write_chunks(splits, tmp_path / f'{encoding}_snappy', gpu_device, encoding, chunk=13, compression='snappy')
        assert [p.name for p in packed] == [p.name for p in plain] and len(packed) == 3
        for a, b in zip(plain, packed):
            md = pq.ParquetFile(b).metadata
            assert {md.row_group(0).column(j).compression for j in range(4)} == {'SNAPPY'}
            got, ref = pd.read_parquet(b), pd.read_parquet(a)
            assert list(got.dtypes) == list(ref.dtypes)
            pd.testing.assert_frame_equal(got, ref)
        x, y = events.parquet_to_events_device(packed, gpu_device), events.parquet_to_events_device(plain, gpu_device)
        for k in ('aid', 'ts', 'type', 'sess_off', 'session_ids', 'order'):
            assert getattr(x, k).dtype == getattr(y, k).dtype and bool(torch.equal(getattr(x, k), getattr(y, k))), k
        assert x.n_aids == y.n_aids and x.n_events > 0


# ---- stream and scratch: the contract of tests/contract_cases.py for the job record -------------------------------------------
def _contract_inputs(seed, scale=1):
    rng = np.random.default_rng(seed)
    n = 45000 * scale
    typ = rng.choice(3, n, p=[0.9, 0.07, 0.03]).astype(np.int32).tobytes()
    wgt = rng.geometric(0.35, n).astype(np.float32).tobytes()
    buf = typ + wgt
    cutp = [0, 70001, 4 * n + 3, len(buf)]                     # three streams, the second of several fragments
    return buf, np.array(cutp[:-1], dtype=np.int64), np.diff(cutp).astype(np.int64)


def _contract_want(inputs):
    buf, off, ln = inputs
    return [S.compress(buf[o:o + k]) for o, k in zip(off.tolist(), ln.tolist())]


def _job_bytes(sn, dev, d_in, inputs, work):
    import torch
    job = sn.DeviceJob(d_in, inputs[1], inputs[2], work)
    nb = job.plan()
    dst = np.r_[0, np.cumsum(nb)[:-1]] + 3
    out = torch.full((int(nb.sum()) + 8,), CANARY, dtype=torch.uint8, device=dev)
    job.emit(dst, out)
    return nb.tolist(), out


def _same(nb, out, want):
    buf = out.cpu().numpy()
    at = 3
    assert nb == [len(w) for w in want]
    for w in want:
        assert buf[at:at + len(w)].tobytes() == w
        at += len(w)
    assert (buf[:3] == CANARY).all() and (buf[at:] == CANARY).all()


def test_reused_scratch_and_repetition(sn, gpu_device):
    import torch
    real, decoy, decoy2 = _contract_inputs(1), _contract_inputs(2), _contract_inputs(2, 2)
    want = _contract_want(real)
    work = torch.empty(4 << 20, dtype=torch.uint8, device=gpu_device)
    d = lambda inputs: _bytes(inputs[0], gpu_device)
    _same(*_job_bytes(sn, gpu_device, d(real), real, work), want)
    _same(*_job_bytes(sn, gpu_device, d(real), real, work), want)                                 # twice in a row
    _same(*_job_bytes(sn, gpu_device, d(decoy), decoy, work), _contract_want(decoy))
    _same(*_job_bytes(sn, gpu_device, d(real), real, work), want)                                 # after a decoy of the same size
    _same(*_job_bytes(sn, gpu_device, d(decoy2), decoy2, work), _contract_want(decoy2))
    _same(*_job_bytes(sn, gpu_device, d(real), real, work), want)                                 # after one of twice the size


def test_side_stream_with_late_inputs(sn, gpu_device):
    """The input holds a decoy; on a side stream a delay is followed by the copy of the real bytes and by plan + emit. An entry
    point that launched on another stream than the job's would read the decoy."""
    import torch
    real, decoy = _contract_inputs(1), _contract_inputs(2)
    want = _contract_want(real)
    assert all(a != b for a, b in zip(want, _contract_want(decoy)))
    torch.cuda._sleep(1_000_000)                             # the first launch of the delay kernel is not the measured one
    torch.cuda.synchronize(gpu_device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                               # about 30 ms
    d_in = _bytes(decoy[0], gpu_device)
    pinned = torch.from_numpy(np.frombuffer(real[0], dtype=np.uint8).copy()).pin_memory()
    work = torch.empty(4 << 20, dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        d_in.copy_(pinned, non_blocking=True)
        nb, out = _job_bytes(sn, gpu_device, d_in, real, work)
    side.synchronize()
    print(f'snappy: the delay in front of the late inputs took {e0.elapsed_time(e1):.1f} ms')
    assert e0.elapsed_time(e1) >= 10.0
    _same(nb, out, want)
