"""Device side of the Parquet decode (include/otto_parquet.h, otto_amd/parquet.py): every decoded column bit-exact against
pyarrow's own decode on every writer variant, bit width, run shape and dtype; the Snappy kernel against
``pyarrow.Codec('snappy')`` and on hand-encoded streams of every tag kind; malformed streams (status set, guard bytes
untouched -- the same streams ``test_parquet_cpu.py`` runs through the sanitizer build first); device refusals;
``parquet_to_events_device`` against the frame path and the builder switch."""
import importlib
import os

import numpy as np
import pytest
import torch

import parquet_inputs as pi

pytestmark = pytest.mark.gpu


def _np(t, like):
    """a decoded tensor as the NumPy dtype of pyarrow's array (same width: a view of the bits)"""
    a = t.cpu().numpy()
    like = np.dtype('int64') if like.kind == 'M' else like
    assert a.dtype.itemsize == like.itemsize, (a.dtype, like)
    return a.view(like)


def _check(paths, columns, gpu_device, **kw):
    from otto_amd import parquet
    want = pi.expected(paths, columns)
    got = parquet.read_columns(paths, columns, gpu_device, **kw)
    assert len(got) == len(columns)
    for g, c in zip(got, columns):
        w = want[c]
        assert g.device == gpu_device and g.shape == w.shape
        assert np.array_equal(_np(g, w.dtype), w.view(np.int64) if w.dtype.kind == 'M' else w), (paths, c)
    return got


@pytest.mark.parametrize('n', pi.ROWS)
@pytest.mark.parametrize('writer', list(pi.WRITERS))
def test_read_columns_equals_pyarrow(gpu_device, tmp_path, writer, n):
    got = _check(pi.WRITERS[writer](tmp_path, n), pi.COLUMNS, gpu_device)
    assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.int64, torch.uint8]


def test_read_columns_in_several_batches(gpu_device, tmp_path):
    """row groups of 30 000 rows and a batch size that takes one or two of them: the staging sets alternate and are reused"""
    from otto_amd import parquet
    paths = pi.w_rowgroups(tmp_path, 200003) + pi.w_twofile(tmp_path, 1000)
    for batch_bytes in (1, 1 << 20, 3 << 20):
        _check(paths, pi.COLUMNS, gpu_device, batch_bytes=batch_bytes)
    _check(paths, ['ts', 'aid'], gpu_device, batch_bytes=1 << 20)                 # a subset, in another order
    assert all(t.numel() == 0 for t in parquet.read_columns([], pi.COLUMNS, gpu_device))


@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('width', pi.WIDTHS)
def test_dictionary_bit_widths(gpu_device, tmp_path, width, dtype):
    _check(pi.w_width(tmp_path, width, dtype), ['v'], gpu_device)


def test_dictionary_bit_width_20_and_0(gpu_device, tmp_path):
    from otto_amd import parquet
    _check(pi.w_width(tmp_path, 20, np.int32), ['v'], gpu_device)
    got, = parquet.read_columns(pi.width0_file(tmp_path), ['v'], gpu_device)
    assert got.dtype == torch.int32 and got.cpu().tolist() == [42] * 1000


def test_run_shapes(gpu_device, tmp_path):
    for col, path in pi.w_runs(tmp_path).items():
        _check([path], [col], gpu_device)


def test_dtypes_default_and_explicit(gpu_device, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_amd import parquet
    rng = np.random.default_rng(3)
    n = 5000
    cols = {'u8': rng.integers(0, 256, n).astype(np.uint8), 'i8': rng.integers(-128, 128, n).astype(np.int8),
            'i16': rng.integers(-2 ** 15, 2 ** 15, n).astype(np.int16), 'u16': rng.integers(0, 2 ** 16, n).astype(np.uint16),
            'u32': rng.integers(0, 2 ** 32, n).astype(np.uint32), 'i32': rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
            'i64': rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64), 'u64': rng.integers(0, 2 ** 63, n).astype(np.uint64) * 2 + 1,
            'ms': rng.integers(0, 2 ** 40, n).astype('datetime64[ms]')}
    for k, kw in enumerate(({}, {'use_dictionary': False}, {'data_page_version': '2.0', 'compression': 'none'})):
        path = str(tmp_path / f'dtypes{k}.parquet')
        pq.write_table(pa.table(cols), path, **kw)
        got = _check([path], list(cols), gpu_device)
        assert [g.dtype for g in got] == [torch.uint8, torch.int8, torch.int16, torch.int16, torch.int32, torch.int32, torch.int64,
                                          torch.int64, torch.int64]
        # explicit dtypes: numpy.astype of pyarrow's array, narrowing and widening
        casts = {'u8': torch.int64, 'i8': torch.int32, 'i16': torch.int64, 'u16': torch.int32, 'u32': torch.int64, 'i32': torch.int64,
                 'i64': torch.int16, 'u64': torch.uint8, 'ms': torch.int32}
        got = parquet.read_columns(path, list(cols), gpu_device, dtypes=casts)
        for g, (c, dt) in zip(got, casts.items()):
            nd = torch.empty(0, dtype=dt).numpy().dtype
            src = cols[c].view(np.int64) if cols[c].dtype.kind == 'M' else cols[c]
            assert g.dtype == dt and np.array_equal(g.cpu().numpy(), src.astype(nd)), (c, dt)
    with pytest.raises(ValueError, match='dtypes'):
        parquet.read_columns(path, ['u8'], gpu_device, dtypes={'u8': torch.float32})


def _decompress(streams, gpu_device, guard=64):
    """run the streams [(bytes, declared)] in ONE call; the outputs lie between guard bytes. -> (outputs, status)"""
    from otto_amd import parquet
    src_off = np.cumsum([0] + [len(b) for b, _ in streams])[:-1]
    buf = torch.from_numpy(np.frombuffer(b''.join(b for b, _ in streams) or b'\0', dtype=np.uint8).copy()).to(gpu_device)
    dst_len = np.array([n for _, n in streams], dtype=np.int64)
    dst_off = guard + np.cumsum(np.r_[0, dst_len[:-1] + guard])
    total = int(dst_off[-1] + dst_len[-1] + guard)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu_device)
    got, status = parquet.snappy_decompress(buf, src_off, [len(b) for b, _ in streams], dst_len, out=out, dst_off=dst_off)
    assert got is out and status.dtype == np.int32 and len(status) == len(streams)
    host = out.cpu().numpy()
    is_guard = np.ones(total, dtype=bool)
    for o, n in zip(dst_off, dst_len):
        is_guard[o:o + n] = False
    assert (host[is_guard] == 0xA5).all(), 'a byte outside every output extent was written'
    return [host[o:o + n].tobytes() for o, n in zip(dst_off, dst_len)], status


def test_snappy_equals_the_codec(gpu_device, tmp_path):
    import pyarrow as pa
    from otto_amd import parquet
    codec = pa.Codec('snappy')
    inputs = dict(pi.codec_inputs())
    # a real `aid` page, as it lies in a file
    path = pi.w_default(tmp_path, 200003)[0]
    meta, pages = parquet.page_table(path, ['aid'])
    page = max((p for p in pages[0, 'aid']), key=lambda p: p.comp_size)
    assert page.is_compressed
    with open(path, 'rb') as f:
        f.seek(meta.row_groups[0].chunks['aid'].start + page.src_off)
        raw = f.read(page.comp_size)
    streams = [(codec.compress(d, asbytes=True), len(d)) for d in inputs.values()] + [(raw, page.uncomp_size)]
    want = list(inputs.values()) + [codec.decompress(raw, decompressed_size=page.uncomp_size).to_pybytes()]
    for s, w in zip(streams, want):                                          # one call per stream, fresh output
        buf = torch.from_numpy(np.frombuffer(s[0], dtype=np.uint8).copy()).to(gpu_device)
        out, status = parquet.snappy_decompress(buf, 0, len(s[0]), s[1])
        assert status.tolist() == [0] and out.cpu().numpy().tobytes() == w
    # 300 streams of mixed sizes in one call
    rng = np.random.default_rng(9)
    mixed = []
    for i in range(300):
        n = int(rng.choice([0, 1, 5, 63, 64, 65, 1000, 5000, 20000]))
        kind = i % 4
        d = (rng.integers(0, 256, n, dtype=np.uint8) if kind == 0 else rng.integers(0, 3, n, dtype=np.uint8) if kind == 1 else
             np.full(n, i & 255, dtype=np.uint8) if kind == 2 else (np.arange(n) % (1 + i % 11)).astype(np.uint8)).tobytes()
        mixed.append(d)
    outs, status = _decompress([(codec.compress(d, asbytes=True), len(d)) for d in mixed], gpu_device)
    assert not status.any() and outs == mixed


def test_snappy_hand_encoded_streams(gpu_device):
    hs = pi.hand_streams()
    outs, status = _decompress(list(hs.values()), gpu_device)
    for (name, (buf, n)), o, st in zip(hs.items(), outs, status):
        assert st == 0 and o == pi.decode(buf, n), name


def test_snappy_malformed_streams(gpu_device):
    """every stream comes back with its status set; _decompress checks the guard bytes around every output extent. Valid
    streams between the malformed ones still decode."""
    bad = pi.malformed_streams()
    good = pi.hand_streams()['copy2']
    streams = []
    for s in bad.values():
        streams += [s, good]
    outs, status = _decompress(streams, gpu_device, guard=256)
    for i, name in enumerate(bad):
        assert status[2 * i] != 0, name
        assert status[2 * i + 1] == 0 and outs[2 * i + 1] == pi.decode(*good), name
    from otto_amd import _lib, parquet
    buf = torch.zeros(16, dtype=torch.uint8, device=gpu_device)
    for args in (([8], [16], [4]), ([0], [4], [4]), ([-1], [4], [4])):          # an extent outside the buffers: refused before any launch
        out = torch.zeros(2, dtype=torch.uint8, device=gpu_device)
        with pytest.raises(_lib.OttoError, match='extent outside'):
            parquet.snappy_decompress(buf, *args, out=out, dst_off=[0])


def test_device_refusals_leave_outputs_untouched(gpu_device, tmp_path):
    from otto_amd import _lib, parquet
    for make, reason in ((pi.null_v1_file, 'a null'), (pi.bad_index_file, "dictionary index not below the dictionary's size")):
        path, page = make(tmp_path)
        out = (torch.full((3000,), -7, dtype=torch.int32, device=gpu_device),)
        with pytest.raises(_lib.OttoError) as e:
            parquet.read_columns(path, ['aid'], gpu_device, out=out)
        msg = str(e.value)
        assert os.path.basename(path) in msg and "column 'aid', row group 0, page %d: " % page in msg and reason in msg, msg
        assert (out[0] == -7).all()
    good = pi.w_default(tmp_path, 3000)[0]                                   # a good file in front of the bad one: still nothing
    out = (torch.full((6000,), -7, dtype=torch.int32, device=gpu_device),)
    with pytest.raises(_lib.OttoError, match='bad_index.parquet'):
        parquet.read_columns([good, path], ['aid'], gpu_device, out=out, batch_bytes=1)
    assert (out[0] == -7).all()
    out = (torch.full((3000,), -7, dtype=torch.int32, device=gpu_device),)
    assert parquet.read_columns(good, ['aid'], gpu_device, out=out)[0] is out[0] and not (out[0] == -7).all()


def _events_equal(a, b):
    for k in ('aid', 'ts', 'type', 'sess_off', 'session_ids', 'order'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x, y), k
    assert a.n_aids == b.n_aids


@pytest.mark.parametrize('case', ['shuffled3', 'seconds_int32', 'ms_int64', 'timestamp'])
def test_parquet_to_events_device_equals_the_frame_path(gpu_device, tmp_path, case):
    import pandas as pd
    import pyarrow.parquet as pq
    from otto_amd import events
    f = pi.frame(50000, seed=4)
    if case == 'shuffled3':
        perm = np.random.default_rng(2).permutation(50000)
        f = {k: v[perm] for k, v in f.items()}
    df = pd.DataFrame(f)
    if case == 'seconds_int32':
        df['ts'] = (df['ts'] // 1000).astype(np.int32)
    if case == 'timestamp':
        df['ts'] = df['ts'].to_numpy().astype('datetime64[ms]')
    cuts = [0, 17000, 17001, 50000] if case == 'shuffled3' else [0, 50000]
    paths = []
    for i in range(len(cuts) - 1):
        paths.append(str(tmp_path / f'{case}{i}.parquet'))
        df.iloc[cuts[i]:cuts[i + 1]].to_parquet(paths[-1])
    want = events.frame_to_events_device([pq.read_table(p, columns=pi.COLUMNS) for p in paths], device=gpu_device)
    got = events.parquet_to_events_device(paths, device=gpu_device)
    assert got.n_events == 50000
    _events_equal(got, want)
    if case == 'ms_int64':
        _events_equal(events.parquet_to_events_device(paths, device=gpu_device, ts_unit='ms', n_aids=70000),
                      events.frame_to_events_device([pq.read_table(p, columns=pi.COLUMNS) for p in paths], device=gpu_device,
                                                    ts_unit='ms', n_aids=70000))


def test_negative_timestamp_is_refused(gpu_device, tmp_path):
    import pandas as pd
    from otto_amd import _lib, events
    df = pd.DataFrame(pi.frame(100))
    df['ts'] = (df['ts'].to_numpy() - df['ts'].to_numpy()[50]).astype('datetime64[ms]')
    df.to_parquet(str(tmp_path / 'neg.parquet'))
    with pytest.raises(_lib.OttoError, match='negative timestamp'):
        events.parquet_to_events_device(str(tmp_path / 'neg.parquet'), device=gpu_device)


def test_builder_switch_writes_identical_parts(gpu_device, tmp_path, monkeypatch):
    import pyarrow.parquet as pq
    monkeypatch.setenv('OTTO_ROOT', str(tmp_path))
    import otto_amd.settings as settings
    importlib.reload(settings)
    from otto_amd.covisitation import builder
    from otto_amd.synth import generate_sessions
    monkeypatch.setattr(builder, 'settings', settings)
    fr = generate_sessions(1200, n_aids=400, seed=8).to_frame()
    fr['session'] = fr['session'] + 11_000_000
    splits = tmp_path / 'data' / 'splits'
    splits.mkdir(parents=True)
    cut = int(np.searchsorted(fr['session'].to_numpy(), fr['session'].iloc[len(fr) // 2]))
    fr.iloc[:cut].to_parquet(splits / 'train.parquet')
    fr.iloc[cut:].to_parquet(splits / 'val.parquet')
    out = tmp_path / 'data' / 'covisitation' / 'validation'
    builder.main(['validation'])
    first = {n: pq.read_table(out / n) for n in sorted(os.listdir(out))}
    for n in first:
        os.remove(out / n)
    builder.main(['validation', '--device-parquet'])
    assert sorted(os.listdir(out)) == list(first) and len(first) > 60
    for n, t in first.items():
        assert pq.read_table(out / n).equals(t), n
    with pytest.raises(ValueError, match='--device-parquet'):
        builder.main(['submission', '--device-parquet'])
