"""The device-side Parquet encoder (include/otto_pqwrite.h, otto_amd/parquet_write.py) on the GPU: the page bodies must equal
the restatement (tests/parquet_write_restatement.py) byte for byte, the assembled files must read back through pyarrow and
pandas, the builder's ``--device-write`` and the chunk writer must give the frames of the host paths, and the calling contract
tests/contract_cases.py states for the streamed entry points (side stream with late inputs, reused scratch, repetition) must
hold for these two, whose stream rides in the job record. Everything is exact."""
import importlib
import os

import numpy as np
import pandas as pd
import pyarrow.parquet as pq
import pytest

import parquet_write_restatement as R

pytestmark = pytest.mark.gpu

EDGE = dict(page_rows=256, row_group_rows=512)
CANARY = 0xA5


@pytest.fixture(scope='module')
def pw():
    import __graft_entry__ as g
    g.build()
    from otto_amd import parquet_write
    return parquet_write


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bodies(pw, dev, arrays, encodings, page_rows=256, gaps=(0,), lead=0, work=None):
    """Every column cut into pages of ``page_rows``; plan + emit with the bodies ``gaps`` bytes apart (cycled) from byte
    ``lead`` of a canary-filled buffer. Returns (pages, page_bytes, page_dst, the buffer on the host)."""
    import torch
    pages = [(r, min(page_rows, len(a) - r), j) for j, a in enumerate(arrays) for r in range(0, max(len(a), 1), page_rows)]
    job = pw.DeviceJob([_dev(a, dev) for a in arrays], encodings, np.array(pages, dtype=pw.PAGE_DTYPE), work)
    page_bytes = job.plan()
    dst, at = [], lead
    for i, b in enumerate(page_bytes.tolist()):
        dst.append(at)
        at += b + gaps[i % len(gaps)]
    out = torch.full((at + 7,), CANARY, dtype=torch.uint8, device=dev)
    job.emit(dst, out)
    return pages, page_bytes.tolist(), dst, out.cpu().numpy()


def _check_bodies(arrays, encodings, pages, page_bytes, dst, buf):
    covered = np.zeros(len(buf), dtype=bool)
    for (r, k, j), nb, at in zip(pages, page_bytes, dst):
        want = R.page_body(arrays[j][r:r + k], encodings[j])
        assert nb == len(want), (j, r, k, nb, len(want))
        got = buf[at:at + nb].tobytes()
        assert got == want, (j, r, k, next(i for i in range(nb) if got[i] != want[i]))
        covered[at:at + nb] = True
    assert (buf[~covered] == CANARY).all(), 'a byte outside every page extent was written'


def _read_back(path, columns):
    t = pq.read_table(path)
    df = pd.read_parquet(path)
    assert t.column_names == list(columns)
    for name, a in columns.items():
        got = t.column(name).to_numpy()
        assert got.dtype == a.dtype and df[name].dtype == a.dtype, (name, got.dtype)
        assert np.array_equal(got.view(np.uint8), a.view(np.uint8)), name
        assert np.array_equal(df[name].to_numpy().view(np.uint8), a.view(np.uint8)), name


# ---- delta -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.EDGE_ROWS)
def test_delta_edge_sizes(pw, gpu_device, tmp_path, n):
    arrays = [R.pattern('runs_of_20', n), R.pattern('random_aids', n, seed=n), R.pattern('alt_int64', n)]
    enc = [R.DELTA] * 3
    _check_bodies(arrays, enc, *_bodies(pw, gpu_device, arrays, enc))
    cols = dict(zip(('aid_x', 'aid_y', 'big'), arrays))
    path = tmp_path / 'edge.parquet'
    pw.write_table(path, {k: _dev(v, gpu_device) for k, v in cols.items()}, {k: 'delta' for k in cols}, **EDGE)
    _read_back(path, cols)
    assert len(pq.ParquetFile(path).metadata.to_dict()['row_groups']) == max(1, -(-n // 512))
    want, = pw.encode_tables_host(cols, [0, n], {k: 'delta' for k in cols}, body=R.page_body, **EDGE)
    assert path.read_bytes() == bytes(want)                  # the whole image, headers and footer included


@pytest.mark.parametrize('name', R.PATTERNS)
def test_delta_value_patterns(pw, gpu_device, tmp_path, name):
    for n in R.PATTERN_ROWS:
        a = R.pattern(name, n)
        _check_bodies([a], [R.DELTA], *_bodies(pw, gpu_device, [a], [R.DELTA]))
        pw.write_table(tmp_path / 'p.parquet', {'v': _dev(a, gpu_device)}, {'v': 'delta'}, **EDGE)
        _read_back(tmp_path / 'p.parquet', {'v': a})


def test_delta_a_block_per_width(pw, gpu_device, tmp_path):
    """Every w in 0..32 as INT32 and 33..63 as INT64; one job holds them all, a column per width."""
    cases = R.width_cases()
    arrays = [v for _, v in cases]
    enc = [R.DELTA] * len(arrays)
    pages, page_bytes, dst, buf = _bodies(pw, gpu_device, arrays, enc)
    _check_bodies(arrays, enc, pages, page_bytes, dst, buf)
    for (w, v), at in zip(cases, dst):
        hdr = len(R.uleb(128) + R.uleb(4) + R.uleb(len(v)) + R.uleb(0))
        m = v[2] - v[1]                                      # the -b step
        z = len(R.uleb(R.zigzag(int(m))))
        assert buf[at + hdr + z:at + hdr + z + 4].tolist() == [w] * 4, w
    for w in (0, 1, 31, 32, 33, 62, 63):
        v = arrays[w]
        pw.write_table(tmp_path / 'w.parquet', {'v': _dev(v, gpu_device)}, {'v': 'delta'}, **EDGE)
        _read_back(tmp_path / 'w.parquet', {'v': v})


def test_delta_of_narrow_and_unsigned_columns(pw, gpu_device, tmp_path):
    cols = {'a': np.arange(300, dtype=np.uint8), 'b': (np.arange(300) * 100).astype(np.uint16), 'c': np.arange(300, dtype=np.int8) & 0x7F,
            'd': np.arange(300, dtype=np.uint32) * 7000000, 'e': np.arange(300, dtype=np.uint64) << 53, 'f': np.arange(300, dtype=np.int16)}
    arrays = list(cols.values())
    _check_bodies(arrays, [R.DELTA] * 6, *_bodies(pw, gpu_device, arrays, [R.DELTA] * 6))
    pw.write_table(tmp_path / 'n.parquet', {k: _dev(v, gpu_device) for k, v in cols.items()}, {k: 'delta' for k in cols}, **EDGE)
    _read_back(tmp_path / 'n.parquet', cols)


# ---- PLAIN -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.PLAIN_DTYPES)
def test_plain_every_element_type(pw, gpu_device, tmp_path, dtype):
    for n in R.PLAIN_ROWS:
        a = R.plain_column(dtype, n)
        _check_bodies([a], [R.PLAIN], *_bodies(pw, gpu_device, [a], [R.PLAIN], page_rows=4096, gaps=(3,), lead=1))
        pw.write_table(tmp_path / 'plain.parquet', {'v': _dev(a, gpu_device)}, **EDGE)
        _read_back(tmp_path / 'plain.parquet', {'v': a})


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_a_value_outside_the_delta_domain_is_refused(pw, gpu_device):
    import torch
    from otto_amd import _lib
    a = R.pattern('random_aids', 700)
    neg = a.copy()
    neg[[300, 555]] = -5
    cols = {'aid_x': _dev(a, gpu_device), 'aid_y': _dev(neg, gpu_device)}
    with pytest.raises(_lib.OttoError, match=r"column 'aid_y', row 300\b"):
        pw.encode_tables(cols, [0, 700], {'aid_x': 'delta', 'aid_y': 'delta'}, **EDGE)
    image, = pw.encode_tables(cols, [0, 700], {'aid_x': 'delta'}, **EDGE)          # the same column under PLAIN is accepted
    pages = np.array([(0, 256, 0), (256, 256, 0), (512, 188, 0)], dtype=pw.PAGE_DTYPE)
    job = pw.DeviceJob([cols['aid_y']], [R.DELTA], pages)
    with pytest.raises(_lib.OttoError, match=r'code -22\): otto_pqw_plan: column 0, row 300: .*DELTA_BINARY_PACKED'):
        job.plan()
    out = torch.full((4096,), CANARY, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):                 # a refused plan leaves no plan behind
        job.emit([0, 1000, 2000], out)
    assert (out.cpu().numpy() == CANARY).all()
    big = a.astype(np.uint32)
    big[[0, 699]] = 2 ** 31                                   # the first value of a page, which no block checks, and the last
    with pytest.raises(_lib.OttoError, match=r"column 'v', row 0\b"):
        pw.encode_tables({'v': _dev(big, gpu_device)}, [0, 700], {'v': 'delta'}, **EDGE)
    big[0] = 5
    with pytest.raises(_lib.OttoError, match=r"column 'v', row 699\b.*2\^31"):
        pw.encode_tables({'v': _dev(big, gpu_device)}, [0, 700], {'v': 'delta'}, **EDGE)
    one = np.array([2 ** 62], dtype=np.int64)                 # a page of one value has no block at all
    with pytest.raises(_lib.OttoError, match=r"column 'v', row 0\b.*2\^62"):
        pw.encode_tables({'v': _dev(one, gpu_device)}, [0, 1], {'v': 'delta'}, **EDGE)
    _read_back_image(image, {'aid_x': a, 'aid_y': neg})


def _read_back_image(image, columns):
    import pyarrow as pa
    t = pq.read_table(pa.BufferReader(bytes(image)))
    for name, a in columns.items():
        got = t.column(name).to_numpy()
        assert got.dtype == a.dtype and np.array_equal(got, a), name


def test_emit_refuses_bad_extents_and_foreign_workspaces(pw, gpu_device):
    import torch
    from otto_amd import _lib
    a, b = R.pattern('random_aids', 600), R.pattern('random_aids', 600, seed=9)
    pages = np.array([(0, 256, 0), (256, 256, 0), (512, 88, 0)], dtype=pw.PAGE_DTYPE)
    work = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu_device)
    da, db = _dev(a, gpu_device), _dev(b, gpu_device)
    job = pw.DeviceJob([da], [R.DELTA], pages, work)
    nb = job.plan().tolist()
    out = torch.full((sum(nb) + 64,), CANARY, dtype=torch.uint8, device=gpu_device)
    untouched = lambda: bool((out.cpu().numpy() == CANARY).all())
    with pytest.raises(_lib.OttoError, match='overlap'):
        job.emit([0, nb[0] - 1, nb[0] + nb[1]], out)
    with pytest.raises(_lib.OttoError, match='overlap'):
        job.emit([5, 5 + nb[0], 5], out)
    assert untouched()
    with pytest.raises(_lib.OttoError, match='leave out_bytes'):
        job.emit([0, nb[0], out.numel() - nb[2] + 1], out)
    with pytest.raises(_lib.OttoError, match='leave out_bytes'):
        job.emit([-1, nb[0], nb[0] + nb[1]], out)
    assert untouched()
    other = pw.DeviceJob([db], [R.DELTA], pages, work)        # same shapes, same scratch, another column: another job
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):
        other.emit([0, nb[0], nb[0] + nb[1]], out)
    fewer = pw.DeviceJob([da], [R.DELTA], pages[:2], work)
    with pytest.raises(_lib.OttoError, match='does not hold the plan'):
        fewer.emit([0, nb[0]], out)
    assert untouched()
    job.emit([0, nb[0], nb[0] + nb[1]], out)                  # the plan is still there
    _check_bodies([a], [R.DELTA], pages.tolist(), nb, [0, nb[0], nb[0] + nb[1]], out.cpu().numpy())
    with pytest.raises(ValueError, match='work'):
        pw.DeviceJob([da], [R.DELTA], pages, work[:256])
    with pytest.raises(_lib.OttoError, match='rows'):
        pw.DeviceJob([da], [R.DELTA], np.array([(500, 256, 0)], dtype=pw.PAGE_DTYPE))
    with pytest.raises(_lib.OttoError, match='encoding'):
        pw.DeviceJob([_dev(a.astype(np.float32), gpu_device)], [R.DELTA], pages)


# ---- extents -----------------------------------------------------------------------------------------------------------
def test_extents_at_odd_offsets_with_gaps(pw, gpu_device):
    n = 1025
    arrays = [R.pattern('runs_of_20', n), R.pattern('random_aids', n), R.pattern('alt_int64', n), R.plain_column('float32', n),
              R.plain_column('int8', n), R.pattern('alt_int32', n), R.plain_column('uint64', n)]
    enc = [R.DELTA, R.DELTA, R.DELTA, R.PLAIN, R.PLAIN, R.DELTA, R.PLAIN]
    for lead in (1, 3):
        pages, nb, dst, buf = _bodies(pw, gpu_device, arrays, enc, gaps=(1, 3, 17), lead=lead)
        assert any(d % 2 for d in dst) and {(b - a - k) for a, b, k in zip(dst, dst[1:], nb)} == {1, 3, 17}
        _check_bodies(arrays, enc, pages, nb, dst, buf)
        assert (buf[:lead] == CANARY).all() and (buf[dst[-1] + nb[-1]:] == CANARY).all()


# ---- files ----------------------------------------------------------------------------------------------------------------
def test_encode_tables_with_cuts(pw, gpu_device, tmp_path):
    from otto_amd.covisitation import builder
    rng = np.random.default_rng(3)
    n = 3000
    aid_x = np.repeat(np.sort(rng.choice(R.N_AIDS, size=n // 15, replace=False)), 15).astype(np.int32)
    aid_y = rng.integers(0, R.N_AIDS, size=n).astype(np.int32)
    W = rng.integers(1, 2 ** 40, size=n).astype(np.uint64)
    wgt = (W.astype(np.float64) / 65536).astype(np.float32)
    cuts = [0, 0, 1, 1300, 2990, 3000, 3000]
    cols = {'aid_x': _dev(aid_x, gpu_device), 'aid_y': _dev(aid_y, gpu_device), 'wgt': _dev(wgt, gpu_device)}
    paths = [tmp_path / f'dev_{i}.pqt' for i in range(6)]
    sizes = pw.write_tables(paths, cols, cuts, {'aid_x': 'delta', 'aid_y': 'delta'}, **EDGE)
    to_dict = lambda df: df.groupby('aid_x')['aid_y'].apply(list).to_dict()           # covisitation_df_to_dict
    for i, (p, lo, hi) in enumerate(zip(paths, cuts, cuts[1:])):
        assert os.path.getsize(p) == sizes[i]
        _read_back(p, {'aid_x': aid_x[lo:hi], 'aid_y': aid_y[lo:hi], 'wgt': wgt[lo:hi]})
        host = str(tmp_path / f'host_{i}.pqt')
        builder.write_part((host, aid_x[lo:hi].view(np.uint32), aid_y[lo:hi].view(np.uint32), W[lo:hi]))
        want, got = pd.read_parquet(host), pd.read_parquet(p)
        assert to_dict(got) == to_dict(want)
        pd.testing.assert_frame_equal(got, want)
    from otto_amd import parquet
    assert [parquet.read_metadata(p).num_rows for p in paths] == [0, 1, 1299, 1690, 10, 0]


def test_builder_device_write_gives_the_same_parts(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setenv('OTTO_ROOT', str(tmp_path))
    import otto_amd.settings as settings
    importlib.reload(settings)
    from otto_amd.covisitation import builder
    from otto_amd.synth import generate_sessions
    monkeypatch.setattr(builder, 'settings', settings)
    fr = generate_sessions(1200, n_aids=400, seed=8).to_frame()
    splits = tmp_path / 'data' / 'splits'
    splits.mkdir(parents=True)
    cut = int(np.searchsorted(fr['session'].to_numpy(), fr['session'].iloc[len(fr) // 2]))
    fr.iloc[:cut].to_parquet(splits / 'train.parquet')
    fr.iloc[cut:].to_parquet(splits / 'val.parquet')
    out = tmp_path / 'data' / 'covisitation' / 'validation'
    builder.main(['validation'])
    first = {n: pd.read_parquet(out / n) for n in sorted(os.listdir(out))}
    for n in first:
        os.remove(out / n)
    builder.main(['validation', '--device-write'])
    assert sorted(os.listdir(out)) == list(first) and len(first) > 60
    rows = 0
    for n, want in first.items():
        got = pd.read_parquet(out / n)
        assert list(got.columns) == ['aid_x', 'aid_y', 'wgt'] and list(got.dtypes) == list(want.dtypes) == [np.int32, np.int32, np.float32]
        pd.testing.assert_frame_equal(got, want)
        rows += len(got)
    assert rows > 10000


def _split_files(tmp_path, frame, tag):
    paths = [tmp_path / f'{tag}_train.parquet', tmp_path / f'{tag}_val.parquet']
    frame.iloc[:len(frame) // 2].to_parquet(paths[0])
    frame.iloc[len(frame) // 2:].to_parquet(paths[1])
    return paths


def _reference_chunks(frame, chunk):
    """The loop of the reference's split_dataset_writer_parquet.py."""
    df = frame.sort_values(by=['session', 'ts'], ascending=[True, True])
    return [df.loc[(df['session'] >= i * chunk) & (df['session'] < (i + 1) * chunk)].reset_index(drop=True)
            for i in range(df['session'].nunique() // chunk + 1)]


def _check_chunks(tmp_path, paths, want, plain, dev):
    from otto_amd import parquet
    assert [p.name for p in paths] == [f'train_truncated_{i}.parquet' for i in range(len(want))]
    for p, w in zip(paths, want):
        w.to_parquet(tmp_path / 'ref.parquet')
        ref, got = pd.read_parquet(tmp_path / 'ref.parquet'), pd.read_parquet(p)
        assert list(got.dtypes) == list(ref.dtypes) and isinstance(got.index, pd.RangeIndex)
        pd.testing.assert_frame_equal(got, ref)
    if plain:                                                 # the project's own decoder reads the PLAIN chunks on the device
        back = parquet.read_columns([str(p) for p in paths], list(want[0].columns), dev)
        whole = pd.concat(want, ignore_index=True)
        for name, t in zip(whole.columns, back):
            assert t.cpu().numpy().dtype == whole[name].dtype and np.array_equal(t.cpu().numpy(), whole[name].to_numpy()), name


def test_chunk_writer(pw, gpu_device, tmp_path):
    from otto_amd.utilities import split_dataset_writer_parquet as sw
    rng = np.random.default_rng(5)
    # 200,000 sessions, 0 .. 199,999, 5,000 of them with a second event: two chunks on either side of session 100,000 and,
    # because nunique // 100,000 + 1 is 3, the empty third chunk the reference writes
    session = np.r_[np.arange(200_000), rng.choice(200_000, size=5_000, replace=False)].astype(np.int32)
    n = len(session)
    frame = pd.DataFrame({'session': session, 'aid': rng.integers(0, R.N_AIDS, size=n).astype(np.int32),
                          'ts': (1659304800000 + rng.permutation(n)).astype(np.int64), 'type': rng.integers(0, 3, size=n).astype(np.uint8)})
    frame = frame.iloc[rng.permutation(n)].reset_index(drop=True)
    want = _reference_chunks(frame, 100_000)
    assert [len(w) > 0 for w in want] == [True, True, False]
    splits = _split_files(tmp_path, frame, 'big')
    for encoding in ('plain', 'delta'):
        paths = sw.write_chunks(splits, tmp_path / encoding, gpu_device, encoding)
        assert sorted(os.listdir(tmp_path / encoding)) == sorted(p.name for p in paths)
        _check_chunks(tmp_path, paths, want, encoding == 'plain', gpu_device)
    # the cut is at session values, not at counts: 40 sessions scattered around the multiples of 13, sessions past the last
    # chunk dropped as the reference's loop drops them
    sess = np.sort(rng.choice(np.r_[0:30, 36:42, 60:70], size=30, replace=False)).astype(np.int32)
    session = np.repeat(sess, rng.integers(1, 9, size=len(sess)))
    n = len(session)
    small = pd.DataFrame({'session': session, 'aid': rng.integers(0, R.N_AIDS, size=n).astype(np.int32),
                          'ts': (1659304800000 + rng.permutation(n)).astype(np.int64), 'type': rng.integers(0, 3, size=n).astype(np.uint8)})
    small = small.iloc[rng.permutation(n)].reset_index(drop=True)
    want = _reference_chunks(small, 13)
    assert len(want) == 3 and sum(len(w) for w in want) < n
    _check_chunks(tmp_path, sw.write_chunks(_split_files(tmp_path, small, 'small'), tmp_path / 'small', gpu_device, chunk=13), want, True,
                  gpu_device)


# ---- stream and scratch ------------------------------------------------------------------------------------------------
def _job_bytes(pw, dev, d_arrays, enc, pages, work):
    import torch
    job = pw.DeviceJob(d_arrays, enc, pages, work)
    nb = job.plan()
    dst = np.r_[0, np.cumsum(nb)[:-1]] + 3
    out = torch.full((int(nb.sum()) + 8,), CANARY, dtype=torch.uint8, device=dev)
    job.emit(dst, out)
    return nb.tolist(), out


def _contract_inputs(seed, scale=1):
    n = 3000 * scale
    rng = np.random.default_rng(seed)
    return [np.sort(rng.integers(0, R.N_AIDS, size=n)).astype(np.int32), rng.integers(0, R.N_AIDS, size=n).astype(np.int32),
            rng.integers(0, 2 ** 62, size=n, dtype=np.int64), rng.random(n).astype(np.float32)]


CONTRACT_ENC = [R.DELTA, R.DELTA, R.DELTA, R.PLAIN]


def _contract_pages(pw, n):
    return np.array([(r, min(512, n - r), j) for j in range(4) for r in range(0, n, 512)], dtype=pw.PAGE_DTYPE)


def _contract_want(arrays, pages):
    return [R.page_body(arrays[j][r:r + k], CONTRACT_ENC[j]) for r, k, j in pages.tolist()]


def _same(nb, out, want):
    buf = out.cpu().numpy()
    at = 3
    assert nb == [len(w) for w in want]
    for w in want:
        assert buf[at:at + len(w)].tobytes() == w
        at += len(w)
    assert (buf[:3] == CANARY).all() and (buf[at:] == CANARY).all()


def test_reused_scratch_and_repetition(pw, gpu_device):
    import torch
    real, decoy, decoy2 = _contract_inputs(1), _contract_inputs(2), _contract_inputs(2, 2)
    pages, pages2 = _contract_pages(pw, 3000), _contract_pages(pw, 6000)
    want = _contract_want(real, pages)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    d = lambda arrays: [_dev(a, gpu_device) for a in arrays]
    first = _job_bytes(pw, gpu_device, d(real), CONTRACT_ENC, pages, work)
    _same(*first, want)
    _same(*_job_bytes(pw, gpu_device, d(real), CONTRACT_ENC, pages, work), want)                  # twice in a row
    _same(*_job_bytes(pw, gpu_device, d(decoy), CONTRACT_ENC, pages, work), _contract_want(decoy, pages))
    _same(*_job_bytes(pw, gpu_device, d(real), CONTRACT_ENC, pages, work), want)                  # after a decoy of the same size
    _same(*_job_bytes(pw, gpu_device, d(decoy2), CONTRACT_ENC, pages2, work), _contract_want(decoy2, pages2))
    _same(*_job_bytes(pw, gpu_device, d(real), CONTRACT_ENC, pages, work), want)                  # after one of twice the size


def test_side_stream_with_late_inputs(pw, gpu_device):
    """The inputs hold a decoy; on a side stream a delay is followed by the copies of the real values and by plan + emit. An
    entry point that launched on another stream than the job's would read the decoy."""
    import torch
    real, decoy = _contract_inputs(1), _contract_inputs(2)
    pages = _contract_pages(pw, 3000)
    want = _contract_want(real, pages)
    assert all(a != b for a, b in zip(want, _contract_want(decoy, pages)))
    torch.cuda._sleep(1_000_000)                             # the first launch of the delay kernel is not the measured one
    torch.cuda.synchronize(gpu_device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                               # about 30 ms
    d_in = [_dev(a, gpu_device) for a in decoy]
    pinned = [torch.from_numpy(a).pin_memory() for a in real]
    work = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        for t, p in zip(d_in, pinned):
            t.copy_(p, non_blocking=True)
        nb, out = _job_bytes(pw, gpu_device, d_in, CONTRACT_ENC, pages, work)
    side.synchronize()
    print(f'pqwrite: the delay in front of the late inputs took {e0.elapsed_time(e1):.1f} ms')
    assert e0.elapsed_time(e1) >= 10.0
    _same(nb, out, want)
