"""List columns and dictionary-coded strings on the device (SPEC-PQLIST, include/otto_pqlist.h; otto_amd/parquet.py):
``read_lists`` against pyarrow's own read on every page shape, value encoding, level depth and naming of
tests/pqlist_inputs.py, on the hand-cut file whose pages open inside a row, over several files and batches; every device
refusal with its file, column, row group, page and reason; ``read_string_codes`` against pyarrow; the calling contract of
``otto_pqlist_levels`` (side stream with late inputs, reused scratch after a larger job, canaries around the outputs)."""
import numpy as np
import pytest
import torch

import pqlist_inputs as I
import pqlist_restatement as R

pytestmark = pytest.mark.gpu
CASES = I.cases()
CANARY = 0x5A


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """every pyarrow-written input once, with pyarrow's own read of it"""
    import pyarrow.parquet as pq
    d = tmp_path_factory.mktemp('pqlist')
    out = {}
    for name, (rws, kw) in CASES.items():
        path = I.write(d / f'{name}.parquet', rws, **kw)
        out[name] = (path, I.from_pylist(pq.read_table(path)[I.COLUMN].to_pylist()))
    return out


def _same(got, want, dtype=torch.int64):
    off, values, null = got
    assert off.dtype == torch.int64 and null.dtype == torch.uint8 and values.dtype == dtype
    assert np.array_equal(off.cpu().numpy(), want[0]), 'off'
    assert np.array_equal(values.cpu().numpy().astype(np.int64), want[1]), 'values'
    assert np.array_equal(null.cpu().numpy(), want[2]), 'null'


@pytest.mark.parametrize('name', sorted(CASES))
def test_read_lists_equals_pyarrow(gpu_device, files, name):
    from otto_amd import parquet
    path, want = files[name]
    int32 = CASES[name][1].get('elem') == 'int32'
    dtype = torch.int64 if name == 'int32_to_int64' else None
    _same(parquet.read_lists(path, I.COLUMN, gpu_device, dtype=dtype), want, torch.int32 if int32 and dtype is None else torch.int64)


def test_several_files_and_batches(gpu_device, files):
    from otto_amd import parquet
    names = ['v1_page1k', 'zero_rows', 'none_v2', 'rowgroups', 'delta', 'only_nulls', 'd2_outer']
    paths = [files[n][0] for n in names]
    off = np.concatenate([[0]] + [files[n][1][0][1:] + sum(len(files[m][1][1]) for m in names[:i]) for i, n in enumerate(names)])
    want = (off.astype(np.int64), np.concatenate([files[n][1][1] for n in names]), np.concatenate([files[n][1][2] for n in names]))
    _same(parquet.read_lists(paths, I.COLUMN, gpu_device), want)
    _same(parquet.read_lists(paths, I.COLUMN, gpu_device, batch_bytes=1), want)              # every row group its own batch
    _same(parquet.read_lists(paths, I.COLUMN, gpu_device, batch_bytes=40000), want)
    out = (torch.zeros(len(want[0]), dtype=torch.int64, device=gpu_device), torch.zeros(len(want[1]), dtype=torch.int64, device=gpu_device),
           torch.zeros(len(want[2]), dtype=torch.uint8, device=gpu_device))
    got = parquet.read_lists(paths, I.COLUMN, gpu_device, out=out)
    assert all(g is o for g, o in zip(got, out))
    _same(out, want)
    for dt in (torch.int32, torch.int16, torch.uint8):                                        # the cast of SPEC-PARQUET's store
        v = parquet.read_lists(files['v1_page1k'][0], I.COLUMN, gpu_device, dtype=dt)[1]
        assert v.dtype == dt and np.array_equal(v.cpu().numpy(), files['v1_page1k'][1][1].astype(v.cpu().numpy().dtype))


def test_pages_cut_inside_a_row(gpu_device, tmp_path):
    from otto_amd import parquet
    rws, rep, dfn, vals, cuts = I.hand_case()
    path = I.hand_file(tmp_path / 'hand.parquet', rep, dfn, vals, cuts)
    _same(parquet.read_lists(path, I.COLUMN, gpu_device), I.expected(rws))
    for outer, elem in ((False, False), (True, False), (False, True)):
        r2, d2, v2 = I.levels_of(rws, outer, elem)
        p2 = I.hand_file(tmp_path / f'hand{outer}{elem}.parquet', r2, d2, v2, cuts, outer, elem)
        _same(parquet.read_lists(p2, I.COLUMN, gpu_device), I.expected(rws, outer))
    one = list(range(5000))                                                                   # one row over five tiles and four pages
    r1, d1, v1 = I.levels_of([one, None, [], one[:3]])
    p1 = I.hand_file(tmp_path / 'one.parquet', r1, d1, v1, [0, 1024, 1025, 3000, len(r1)])
    _same(parquet.read_lists(p1, I.COLUMN, gpu_device), I.expected([one, None, [], one[:3]]))


def test_device_refusals_name_file_column_row_group_page_and_reason(gpu_device, tmp_path, files):
    from otto_amd import _lib, parquet
    for name, (path, page, code) in I.damaged(tmp_path).items():
        with pytest.raises(_lib.OttoError) as e:
            parquet.read_lists(path, I.COLUMN, gpu_device)
        reason = R.REASONS[code] if code else 'the value stream does not hold the 571 values its definition levels announce'
        assert f"{path}: column '{I.COLUMN}', row group 0, page {page}: {reason}" in str(e.value), (name, str(e.value))
    path, want = files['v1_page1k']
    out = (torch.full((len(want[0]),), -3, dtype=torch.int64, device=gpu_device), torch.full((len(want[1]),), -3, dtype=torch.int64, device=gpu_device),
           torch.full((len(want[2]),), 3, dtype=torch.uint8, device=gpu_device))
    raw = bytearray(open(path, 'rb').read())
    meta, table = parquet.list_page_table(path, I.COLUMN)
    chunk = meta.row_groups[0][1]
    page = next(p for p in table[0] if p.page_type == 0)
    raw[chunk.start + page.src_off + 1] ^= 0xFF                                               # inside a Snappy body
    bad = str(tmp_path / 'snappy.parquet')
    open(bad, 'wb').write(bytes(raw))
    with pytest.raises(_lib.OttoError, match='snappy'):
        parquet.read_lists(bad, I.COLUMN, gpu_device, out=out)
    assert all(bool((o == (-3 if o.dtype == torch.int64 else 3)).all()) for o in out)         # a refused call leaves out unwritten
    _same(parquet.read_lists(path, I.COLUMN, gpu_device, out=out), want)


def test_read_string_codes_equals_pyarrow(gpu_device, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_amd import _lib, parquet
    rng = np.random.default_rng(0)
    names = np.array(['clicks', 'carts', 'orders'])
    codes = rng.choice(3, size=70001, p=[0.8, 0.15, 0.05])
    codes[1000:9000] = 2                                                                      # long RLE runs next to mixed ones
    paths = []
    for k, kw in enumerate(({}, dict(compression='none'), dict(data_page_version='2.0', data_page_size=4096), dict(row_group_size=20000),
                            dict(nullable=False))):
        nullable = kw.pop('nullable', True)
        p = str(tmp_path / f's{k}.parquet')
        tab = pa.table([pa.array(names[codes])], schema=pa.schema([pa.field('type', pa.string(), nullable=nullable)]))
        pq.write_table(tab, p, **kw)
        got = parquet.read_string_codes(p, 'type', I.TYPE_CODES, gpu_device)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), codes)
        paths.append(p)
    got = parquet.read_string_codes(paths, 'type', {'clicks': 7, 'carts': -1, 'orders': 300}, gpu_device, dtype=torch.int32)
    assert np.array_equal(got.cpu().numpy(), np.tile(np.array([7, -1, 300], dtype=np.int32)[codes], len(paths)))
    with pytest.raises(ValueError, match='does not fit'):
        parquet.read_string_codes(paths[0], 'type', {'clicks': 256, 'carts': 1, 'orders': 2}, gpu_device)
    with pytest.raises(_lib.OttoError, match="dictionary string 'orders' is not in the mapping"):
        parquet.read_string_codes(paths[0], 'type', {'clicks': 0, 'carts': 1}, gpu_device)


# ---- the calling contract of otto_pqlist_levels ---------------------------------------------------------------------------------
def _job(path):
    """the uncompressed chunks of a file as one byte string, and the level job over them"""
    from otto_amd import parquet
    meta, table = parquet.list_page_table(path, I.COLUMN)
    buf, items = bytearray(), []
    with open(path, 'rb') as f:
        for g, pages in table.items():
            n, c = meta.row_groups[g]
            f.seek(c.start)
            b = f.read(c.length)
            items.append((f'row group {g}', meta.leaf, n, len(buf), pages))
            buf += b + bytes(-len(b) % 16)
    pl, infos, _, streams, at = parquet._list_plan(items, len(buf))
    assert not streams and at == len(buf)
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), pl, infos, meta.num_rows


def _levels(dev, d_bytes, job, work=None, base=0, outs=None):
    from otto_amd import parquet
    _, pl, infos, n_rows = job
    off = torch.full((n_rows + 1,), -7, dtype=torch.int64, device=dev) if outs is None else outs[0]
    null = torch.full((n_rows,), 9, dtype=torch.uint8, device=dev) if outs is None else outs[1]
    report = parquet._list_levels(dev, d_bytes, int(d_bytes.numel()), pl, infos, off, null, n_rows, base, work)
    return off, null, report


@pytest.fixture(scope='module')
def jobs(tmp_path_factory):
    import pyarrow.parquet as pq
    d = tmp_path_factory.mktemp('jobs')
    out = {}
    for name, rws in (('real', I.rows(seed=1)), ('decoy', I.rows(seed=2)), ('large', I.rows(1500, seed=4) + I.rows(1500, seed=5))):
        path = I.write(d / f'{name}.parquet', rws, compression='none', data_page_size=1024, row_group_size=700)
        out[name] = (_job(path), I.from_pylist(pq.read_table(path)[I.COLUMN].to_pylist()))
    return out


def _check(got, want, base=0):
    off, null, report = got
    assert np.array_equal(off.cpu().numpy(), want[0] + base) and np.array_equal(null.cpu().numpy(), want[2])
    assert int(report[:, 1].sum()) == len(want[1]) and int(report[:, 2].sum()) == len(want[2])


def test_levels_on_reused_scratch_after_a_larger_job(gpu_device, jobs):
    dev = gpu_device
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    dev_bytes = {k: torch.from_numpy(v[0][0]).to(dev) for k, v in jobs.items()}
    assert len(jobs['large'][0][1]) > 2 * len(jobs['real'][0][1])
    for name in ('real', 'real', 'decoy', 'real', 'large', 'real'):
        _check(_levels(dev, dev_bytes[name], jobs[name][0], work), jobs[name][1])
    _check(_levels(dev, dev_bytes['real'], jobs['real'][0], work, base=12345), jobs['real'][1], 12345)


def test_levels_on_a_side_stream_with_late_inputs(gpu_device, jobs):
    """The byte buffer holds zeros; on a side stream a delay is followed by the copy of the real bytes and by the call. An
    entry point that launched on another stream than the job's would walk the zeros and refuse them."""
    dev = gpu_device
    job, want = jobs['real']
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                                     # about 30 ms
    d_in = torch.zeros(len(job[0]), dtype=torch.uint8, device=dev)
    pinned = torch.from_numpy(job[0]).pin_memory()
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        d_in.copy_(pinned, non_blocking=True)
        got = _levels(dev, d_in, job, work)
    side.synchronize()
    assert e0.elapsed_time(e1) >= 10.0
    _check(got, want)


def test_canaries_around_off_and_null(gpu_device, jobs, tmp_path):
    """off and null lie inside larger buffers; nothing outside them is written, by a clean job and by one whose chunk holds
    more rows than its row group declares"""
    from otto_amd import _lib
    dev = gpu_device
    job, want = jobs['real']
    n_rows, pad = job[3], 4096
    d_bytes = torch.from_numpy(job[0]).to(dev)
    rws, rep, dfn, vals, cuts = I.hand_case()
    over = _job(I.hand_file(tmp_path / 'over.parquet', rep, dfn, vals, cuts, num_rows=len(rws) - 300))
    for jb, bytes_, clean in ((job, d_bytes, True), (over, torch.from_numpy(over[0]).to(dev), False)):
        bufs = [torch.full((pad + n + pad,), CANARY, dtype=torch.uint8, device=dev) for n in ((jb[3] + 1) * 8, jb[3])]
        outs = (bufs[0][pad:pad + (jb[3] + 1) * 8].view(torch.int64), bufs[1][pad:pad + jb[3]])
        if clean:
            _check(_levels(dev, bytes_, jb, outs=outs), want)
        else:
            with pytest.raises(_lib.OttoError, match="page 0: the count of rows differs from the row group's num_rows"):
                _levels(dev, bytes_, jb, outs=outs)
        torch.cuda.synchronize(dev)
        for b in bufs:
            h = b.cpu().numpy()
            assert (h[:pad] == CANARY).all() and (h[-pad:] == CANARY).all()
