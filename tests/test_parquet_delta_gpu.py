"""DELTA_BINARY_PACKED pages and float columns on the device (SPEC-PARQUET, include/otto_parquet.h; k_pq_delta_* of
csrc/otto_parquet.hip): every decoded column bit-exact against pyarrow's decode of the same file -- files pyarrow wrote
(V1 / V2 pages, REQUIRED / OPTIONAL columns, with and without Snappy, several pages, row groups and files) and files
assembled from the restatement's encoder (tests/parquet_delta_restatement.py) at every block shape, value count and width;
every refusal names file, column, row group and page and hands out nothing; the calling contract. The bodies are the ones
``test_parquet_delta_cpu.py`` runs through the sanitizer build of the same helpers first."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import parquet_delta_restatement as D
import test_parquet_delta_cpu as H

pytestmark = pytest.mark.gpu


def _bits(t):
    a = t.cpu().numpy()
    return a.view(f'u{a.dtype.itemsize}')


def _check(paths, columns, dev, **kw):
    """read_columns against pyarrow's read of the same files, bit for bit"""
    from otto_amd import parquet
    paths = [paths] if isinstance(paths, str) else list(paths)
    got = parquet.read_columns(paths, columns, dev, **kw)
    tables = [pq.read_table(p, columns=columns) for p in paths]
    for g, c in zip(got, columns):
        w = np.concatenate([t.column(c).to_numpy() for t in tables])
        w = w.view(np.int64) if w.dtype.kind == 'M' else w
        assert g.device == dev and g.shape == w.shape and g.cpu().numpy().dtype.itemsize == w.dtype.itemsize, (paths[0], c)
        assert np.array_equal(_bits(g), w.view(f'u{w.dtype.itemsize}')), (paths[0], c)
    return got


# ---- the restatement's encoder: block shapes, value counts, widths, wrap-around, garbage width bytes -------------------------
@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('shape', D.SHAPES, ids=lambda s: f'{s[0]}_{s[1]}')
def test_block_shapes_counts_and_widths(gpu_device, tmp_path, shape, bits):
    """one call over the files of every value count (the last miniblock partly filled, 0 and 1 value included), then the
    column that has every width 0..bits with its largest delta, cut into pages of 256 values and row groups of 512; the width
    bytes of the miniblocks without a value hold 0xFF"""
    B, M = shape
    paths, want = [], {'w': [], 'r': []}
    for n in D.counts(B):
        cols = {'w': D.wrap_around(bits, n), 'r': D.random_column(bits, n, n)}
        paths.append(H.own_file(tmp_path / f'c{n}.parquet', cols, B, M, garbage=0xFF))
        for c in cols:
            want[c].append(cols[c])
    got = _check(paths, ['w', 'r'], gpu_device)
    for g, c in zip(got, ('w', 'r')):
        assert g.dtype == (torch.int32 if bits == 32 else torch.int64) and np.array_equal(g.cpu().numpy(), np.concatenate(want[c]))
    ew = D.every_width(bits, B, M)
    assert D.widths_seen(D.encode(D.stored(ew)[0], bits, B, M), len(ew)) == set(range(bits + 1))
    one = H.own_file(tmp_path / 'ew_one.parquet', {'v': ew}, B, M, garbage=0xFF, page_rows=len(ew) // 128 * 128 + 128)
    cut = H.own_file(tmp_path / 'ew_cut.parquet', {'v': ew}, B, M, garbage=0xFF, page_rows=256, row_group_rows=512)
    got, = _check([one, cut], ['v'], gpu_device)
    assert np.array_equal(got.cpu().numpy(), np.r_[ew, ew])


def test_largest_block_and_long_pages(gpu_device, tmp_path):
    """65536 / 1 (one miniblock of a whole block), and pages of more than 64 blocks (the per-page scan loops)"""
    a = D.random_column(64, 70000, 1)
    p0 = H.own_file(tmp_path / 'big.parquet', {'v': a}, 65536, 1, page_rows=1 << 17)
    b = D.random_column(32, 128 * 150 + 7, 2, 'any')
    p1 = H.own_file(tmp_path / 'long.parquet', {'v': b}, 128, 4, page_rows=1 << 15)
    _check(p0, ['v'], gpu_device)
    _check(p1, ['v'], gpu_device)


# ---- files pyarrow wrote ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compression', ['none', 'snappy'])
@pytest.mark.parametrize('required', [False, True], ids=['optional', 'required'])
@pytest.mark.parametrize('version', ['1.0', '2.0'])
def test_pyarrow_written_files(gpu_device, tmp_path, version, required, compression):
    paths = []
    for n in (1, 129, 130, 300, 777, 1000, 5000):
        paths.append(H.write_arrow(tmp_path / f'a{n}.parquet', H.arrow_columns(n, seed=n), required, data_page_version=version,
                                   compression=compression, data_page_size=300, row_group_size=2048))
    assert pq.ParquetFile(paths[-1]).num_row_groups == 3
    cols = list(H.arrow_columns(1))
    got = _check(paths, cols, gpu_device)
    assert [g.dtype for g in got] == [torch.int32] * 3 + [torch.int64] * 3
    _check(paths, ['r64', 'a32'], gpu_device, batch_bytes=1)                     # a subset, one row group per batch
    _check(paths[-1], cols, gpu_device)


def test_delta_dictionary_and_plain_columns_in_one_call(gpu_device, tmp_path):
    from otto_amd import _lib, parquet
    rng = np.random.default_rng(4)
    n = 3000
    cols = {'delta32': D.random_column(32, n, 1, 'sorted'), 'dict': rng.integers(0, 50, n).astype(np.int32), 'plain': rng.integers(-9, 9, n).astype(np.int64),
            'delta64': D.wrap_around(64, n), 'f': rng.random(n).astype(np.float32), 'd': rng.standard_normal(n)}
    paths = []
    for k, kw in enumerate((dict(compression='snappy'), dict(compression='none', data_page_version='2.0'))):
        paths.append(str(tmp_path / f'mixed{k}.parquet'))
        pq.write_table(pa.table(cols), paths[-1], use_dictionary=['dict', 'd'], data_page_size=300, write_batch_size=64,
                       column_encoding={'delta32': 'DELTA_BINARY_PACKED', 'delta64': 'DELTA_BINARY_PACKED', 'plain': 'PLAIN', 'f': 'PLAIN'}, **kw)
    meta, pages = parquet.page_table(paths[0], list(cols), floats=True)
    kinds = {c: {p.encoding for p in pages[0, c] if p.page_type != parquet.DICTIONARY_PAGE} for c in cols}
    assert kinds == {'delta32': {5}, 'dict': {8}, 'plain': {0}, 'delta64': {5}, 'f': {0}, 'd': {8}}
    got = _check(paths, list(cols), gpu_device, floats=True)
    assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.int64, torch.int64, torch.float32, torch.float64]
    with pytest.raises(_lib.OttoError, match='physical type FLOAT is not supported'):
        parquet.read_columns(paths, ['f'], gpu_device)
    for bad in (torch.float64, torch.int32):
        with pytest.raises(ValueError, match='dtypes'):
            parquet.read_columns(paths, ['f'], gpu_device, floats=True, dtypes={'f': bad})
    with pytest.raises(ValueError, match='dtypes'):
        parquet.read_columns(paths, ['plain'], gpu_device, floats=True, dtypes={'plain': torch.float64})


def test_every_output_cast_on_delta_pages(gpu_device, tmp_path):
    """the columns and casts of test_parquet_gpu.py::test_dtypes_default_and_explicit, delta-coded"""
    from otto_amd import parquet
    rng = np.random.default_rng(3)
    n = 5000
    cols = {'u8': rng.integers(0, 256, n).astype(np.uint8), 'i8': rng.integers(-128, 128, n).astype(np.int8),
            'i16': rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16), 'u16': rng.integers(0, 2 ** 16, n).astype(np.uint16),
            'u32': rng.integers(0, 2 ** 32, n).astype(np.uint32), 'i32': rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
            'i64': rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64), 'u64': rng.integers(0, 2 ** 63, n).astype(np.uint64) * 2 + 1,
            'ms': rng.integers(0, 2 ** 40, n).astype('datetime64[ms]')}
    for k, kw in enumerate(({}, {'data_page_version': '2.0', 'compression': 'snappy'})):
        path = H.write_arrow(tmp_path / f'dtypes{k}.parquet', cols, **kw)
        _, pages = parquet.page_table(path, list(cols))
        assert all(p.encoding == 5 for c in cols for p in pages[0, c])
        got = _check(path, list(cols), gpu_device)
        assert [g.dtype for g in got] == [torch.uint8, torch.int8, torch.int16, torch.int16, torch.int32, torch.int32, torch.int64,
                                          torch.int64, torch.int64]
        casts = {'u8': torch.int64, 'i8': torch.int32, 'i16': torch.int64, 'u16': torch.int32, 'u32': torch.int64, 'i32': torch.int64,
                 'i64': torch.int16, 'u64': torch.uint8, 'ms': torch.int32}
        got = parquet.read_columns(path, list(cols), gpu_device, dtypes=casts)
        for g, (c, dt) in zip(got, casts.items()):
            nd = torch.empty(0, dtype=dt).numpy().dtype
            src = cols[c].view(np.int64) if cols[c].dtype.kind == 'M' else cols[c]
            assert g.dtype == dt and np.array_equal(g.cpu().numpy(), src.astype(nd)), (c, dt)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _bad_file(tmp_path, name, body):
    """898 INT32 rows as row groups of 512 and pages of 256: the bad body is page 1 of row group 1 (130 values) of column 'v';
    column 'u' in front of it is clean"""
    v = D.random_column(32, 898, 5)
    assert 898 - 768 == 130
    return H.own_file(tmp_path / f'{name}.parquet', {'u': v, 'v': v}, page_rows=256, row_group_rows=512, bodies={(1, 768): body})


@pytest.mark.parametrize('name', list(H.refusal_bodies()))
def test_refusals_name_the_page_and_hand_out_nothing(gpu_device, tmp_path, name):
    from otto_amd import _lib, parquet
    body, n, code = H.refusal_bodies()[name]
    assert n == 130
    path = _bad_file(tmp_path, name, body)
    out = tuple(torch.full((898,), -7, dtype=torch.int32, device=gpu_device) for _ in range(2))
    with pytest.raises(_lib.OttoError) as e:
        parquet.read_columns(path, ['u', 'v'], gpu_device, out=out)
    msg = str(e.value)
    assert os.path.basename(path) in msg and "column 'v', row group 1, page 1: " in msg and D.REASONS[code] in msg, msg
    assert (out[0] == -7).all() and (out[1] == -7).all()
    good = _bad_file(tmp_path, 'good', None)                                  # a clean file in front of the bad one: still nothing
    out = tuple(torch.full((2 * 898,), -7, dtype=torch.int32, device=gpu_device) for _ in range(2))
    with pytest.raises(_lib.OttoError, match=f'{name}.parquet'):
        parquet.read_columns([good, path], ['u', 'v'], gpu_device, out=out, batch_bytes=1)
    assert (out[0] == -7).all() and (out[1] == -7).all()
    got = parquet.read_columns(good, ['u', 'v'], gpu_device)
    assert np.array_equal(got[1].cpu().numpy(), D.random_column(32, 898, 5))


# ---- the calling contract -----------------------------------------------------------------------------------------------------
def _contract_file(tmp_path, seed, scale=1):
    n = 3000 * scale
    rng = np.random.default_rng(seed)
    cols = {'x': np.sort(rng.integers(0, 1 << 21, size=n)).astype(np.int32), 'y': rng.integers(0, 1 << 21, size=n).astype(np.int32),
            'b': D.random_column(64, n, seed, 'any'), 'w': rng.random(n).astype(np.float32)}
    path = H.own_file(tmp_path / f'contract{seed}_{scale}.parquet', cols, 256, 8, page_rows=512, row_group_rows=1024)
    return path, cols


def _job(path, dev):
    """one otto_parquet_decode call over the image of a whole file: (image bytes, page table, page infos, rows)"""
    from otto_amd import parquet
    names = ['x', 'y', 'b', 'w']
    meta, pages = parquet.page_table(path, names, floats=True)
    image = np.fromfile(path, dtype=np.uint8)
    table, infos, row = [], [], 0
    for g, rg in enumerate(meta.row_groups):
        for j, c in enumerate(names):
            r = row
            for k, p in enumerate(pages[g, c]):
                table.append((rg.chunks[c].start + p.src_off, p.comp_size, p.uncomp_size, p.page_type, p.encoding, p.def_len, p.rep_len,
                              p.num_values, p.is_compressed, r, j, -1))
                infos.append((f'{path}: column {c!r}, row group {g}', k))
                r += p.num_values
        row += rg.num_rows
    return image, table, infos, meta.num_rows


def _decode(dev, d_bytes, table, infos, n, work, canary=64):
    """one decode into fresh outputs between canaries -> the four columns as NumPy"""
    from otto_amd import parquet
    dts = [torch.int32, torch.int32, torch.int64, torch.float32]
    bufs = [torch.full(((n + 2 * canary) * torch.empty(0, dtype=dt).element_size(),), 0x5A, dtype=torch.uint8, device=dev) for dt in dts]
    cols = []
    for b, dt in zip(bufs, dts):
        size = torch.empty(0, dtype=dt).element_size()
        cols.append((b.data_ptr() + canary * size, size, n, size, 0))
    parquet._decode(dev, d_bytes, int(d_bytes.numel()), table, cols, infos, work=work)
    res = []
    for b, dt in zip(bufs, dts):
        size = torch.empty(0, dtype=dt).element_size()
        h = b.cpu().numpy()
        assert (h[:canary * size] == 0x5A).all() and (h[(canary + n) * size:] == 0x5A).all(), 'a byte outside the column was written'
        res.append(h[canary * size:(canary + n) * size].view(torch.empty(0, dtype=dt).numpy().dtype))
    return res


def _same(got, cols):
    for g, (c, a) in zip(got, cols.items()):
        assert np.array_equal(g.view(f'u{g.dtype.itemsize}'), a.view(f'u{a.dtype.itemsize}')), c


def test_reused_scratch_and_repetition(gpu_device, tmp_path):
    dev = gpu_device
    (real, rc), (decoy, dc), (decoy2, d2c) = _contract_file(tmp_path, 1), _contract_file(tmp_path, 2), _contract_file(tmp_path, 2, 2)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)

    def run(path, cols):
        image, table, infos, n = _job(path, dev)
        _same(_decode(dev, torch.from_numpy(image).to(dev), table, infos, n, work), cols)
    run(real, rc)
    run(real, rc)                                            # twice in a row
    run(decoy, dc)
    run(real, rc)                                            # after a decoy of the same size
    run(decoy2, d2c)
    run(real, rc)                                            # after one of twice the size


def test_side_stream_with_late_inputs(gpu_device, tmp_path):
    """The device bytes hold a decoy file; on a side stream a delay is followed by the copy of the real file and by the
    decode. A kernel launched on another stream than the caller's would read the decoy."""
    dev = gpu_device
    (real, rc), (decoy, _) = _contract_file(tmp_path, 1), _contract_file(tmp_path, 2)
    image, table, infos, n = _job(real, dev)
    other = np.fromfile(decoy, dtype=np.uint8)
    size = max(len(image), len(other))
    d_bytes = torch.zeros(size, dtype=torch.uint8, device=dev)
    d_bytes[:len(other)] = torch.from_numpy(other).to(dev)
    pinned = torch.from_numpy(image).pin_memory()
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    torch.cuda._sleep(1_000_000)                             # the first launch of the delay kernel is not the measured one
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                               # about 30 ms
    side = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        d_bytes[:len(image)].copy_(pinned, non_blocking=True)
        got = _decode(dev, d_bytes, table, infos, n, work)
    side.synchronize()
    print(f'parquet delta: the delay in front of the late inputs took {e0.elapsed_time(e1):.1f} ms')
    assert e0.elapsed_time(e1) >= 10.0
    _same(got, rc)


def test_chunk_files_written_delta_read_back_as_events(gpu_device, tmp_path):
    """a chunk file of the split writer with delta encodings reads through events.parquet_to_events_device equal to the PLAIN one"""
    import pandas as pd
    from otto_amd import events
    from otto_amd.utilities import split_dataset_writer_parquet as sw
    rng = np.random.default_rng(5)
    session = np.r_[np.arange(3000), rng.choice(3000, size=4000)].astype(np.int32)
    n = len(session)
    frame = pd.DataFrame({'session': session, 'aid': rng.integers(0, 50000, size=n).astype(np.int32),
                          'ts': (1659304800000 + rng.permutation(n)).astype(np.int64), 'type': rng.integers(0, 3, size=n).astype(np.uint8)})
    frame = frame.iloc[rng.permutation(n)].reset_index(drop=True)
    splits = [tmp_path / 'train.parquet', tmp_path / 'val.parquet']
    frame.iloc[:n // 2].to_parquet(splits[0])
    frame.iloc[n // 2:].to_parquet(splits[1])
    got = {}
    for encoding in ('plain', 'delta'):
        paths = sw.write_chunks(splits, tmp_path / encoding, gpu_device, encoding, chunk=1000)
        assert len(paths) == 4
        got[encoding] = events.parquet_to_events_device([str(p) for p in paths], device=gpu_device)
    from otto_amd import parquet
    _, pages = parquet.page_table(str(tmp_path / 'delta' / 'train_truncated_0.parquet'), ['aid'])
    assert {p.encoding for p in pages[0, 'aid']} == {5}
    a, b = got['plain'], got['delta']
    assert a.n_events == b.n_events == n
    for k in ('aid', 'ts', 'type', 'sess_off', 'session_ids', 'order'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
