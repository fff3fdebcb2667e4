"""Host side of the Parquet decode (include/otto_parquet.h, otto_amd/parquet.py): the Thrift footer and page-header reader
against pyarrow's own metadata on every writer variant, the page shapes the device tests rely on, the host refusals
SPEC-PARQUET names, and the element decoders of ``csrc/parquet_decode.h`` on the CPU: ``tools/parquet_host_main.cpp`` is
compiled as a stand-alone program with the address and undefined-behaviour sanitizers and must decode every fixture to
pyarrow's arrays and give the reference verdict on every hand-built and malformed Snappy stream (the streams
``test_parquet_gpu.py`` sends to the device afterwards)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parquet_inputs as pi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BIG = 40001


def _body(path, chunk, page):
    """the decoded body of a V1 / dictionary page, through pyarrow's codec"""
    import pyarrow as pa
    with open(path, 'rb') as f:
        f.seek(chunk.start + page.src_off)
        raw = f.read(page.comp_size)
    if page.is_compressed:
        raw = pa.Codec('snappy').decompress(raw, decompressed_size=page.uncomp_size).to_pybytes()
    return raw


def _index_start(body, page):
    """where the bit-width byte of a dictionary-coded V1 page lies"""
    return 4 + int.from_bytes(body[:4], 'little') if page.def_len == -1 else 0


def _flat(path, columns):
    """(records with file offsets, column records 'elem phys zext rows', expected arrays) for the host program"""
    from otto_amd import parquet
    meta, pages = parquet.page_table(path, columns)
    leaves = [parquet.check_column(meta, c) for c in columns]
    rows = sum(g.num_rows for g in meta.row_groups)
    recs, row0 = [], 0
    for g, rg in enumerate(meta.row_groups):
        for j, c in enumerate(columns):
            ch, dict_slot, r = rg.chunks[c], -1, row0
            for p in pages[g, c]:
                if p.page_type == parquet.DICTIONARY_PAGE:
                    dict_slot = len(recs)
                recs.append((ch.start + p.src_off, p.comp_size, p.uncomp_size, p.page_type, p.encoding, p.def_len, p.rep_len,
                             p.num_values, p.is_compressed, r, j, dict_slot if p.page_type != 2 and p.encoding == 8 else -1))
                if p.page_type != parquet.DICTIONARY_PAGE:
                    r += p.num_values
        row0 += rg.num_rows
    cols = [(8, 4 if l.physical == 1 else 8, int(l.physical == 1 and l.logical == ('INT', 32, False)), rows) for l in leaves]
    return recs, cols


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """{(writer, n): paths} of every writer variant at the sizes the CPU tests use"""
    d = tmp_path_factory.mktemp('parquet_cpu')
    out = {}
    for n in (0, 7, 1000, N_BIG):
        sub = d / str(n)
        sub.mkdir()
        for name, w in pi.WRITERS.items():
            out[name, n] = w(sub, n)
    return out


@pytest.mark.parametrize('writer', list(pi.WRITERS))
def test_host_parser_equals_pyarrow_metadata(files, writer):
    import pyarrow.parquet as pq
    from otto_amd import parquet
    for n in (0, 7, 1000, N_BIG):
        for path in files[writer, n]:
            want = pq.ParquetFile(path).metadata
            meta, pages = parquet.page_table(path, pi.COLUMNS)
            assert meta.num_rows == want.num_rows and len(meta.row_groups) == want.num_row_groups
            assert [l.name for l in meta.leaves] == [want.schema.column(i).name for i in range(want.num_columns)]
            for g in range(want.num_row_groups):
                wg = want.row_group(g)
                assert meta.row_groups[g].num_rows == wg.num_rows
                for i in range(wg.num_columns):
                    wc = wg.column(i)
                    c = meta.row_groups[g].chunks[wc.path_in_schema]
                    assert c.data_page_offset == wc.data_page_offset and c.length == wc.total_compressed_size
                    assert (c.dictionary_page_offset or None) == (wc.dictionary_page_offset if wc.has_dictionary_page else None)
                    assert parquet.CODECS[c.codec] == wc.compression and c.num_values == wc.num_values
                    assert parquet.PHYSICAL[c.physical] == wc.physical_type and c.uncompressed == wc.total_uncompressed_size
                    if wc.num_values:                         # an empty chunk has no pages to start at
                        assert c.start == (wc.dictionary_page_offset if wc.has_dictionary_page else wc.data_page_offset)
                    assert {parquet.ENCODINGS[e] for e in c.encodings} == set(wc.encodings)
                    if c.name in pi.COLUMNS and wc.num_values:
                        pg = pages[g, c.name]
                        assert sum(p.num_values for p in pg if p.page_type != parquet.DICTIONARY_PAGE) == wc.num_values
                        assert sum(p.comp_size for p in pg) < c.length and pg[-1].src_off + pg[-1].comp_size == c.length
                        assert [p.page_type for p in pg].count(parquet.DICTIONARY_PAGE) == int(wc.has_dictionary_page)


def test_logical_annotations_and_default_dtypes(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import torch
    from otto_amd import parquet
    cols = {'u8': np.arange(5, dtype=np.uint8), 'i8': np.arange(5, dtype=np.int8), 'i16': np.arange(5, dtype=np.int16),
            'u16': np.arange(5, dtype=np.uint16), 'u32': np.arange(5, dtype=np.uint32), 'i32': np.arange(5, dtype=np.int32),
            'u64': np.arange(5, dtype=np.uint64), 'i64': np.arange(5, dtype=np.int64),
            'ms': np.arange(5).astype('datetime64[ms]'), 'us': np.arange(5).astype('datetime64[us]'), 'ns': np.arange(5).astype('datetime64[ns]')}
    pq.write_table(pa.table(cols), str(tmp_path / 'a.parquet'))
    meta = parquet.read_metadata(tmp_path / 'a.parquet')
    got = {l.name: (l.logical, parquet.default_dtype(l)) for l in meta.leaves}
    assert got['u8'] == (('INT', 8, False), torch.uint8) and got['i8'] == (('INT', 8, True), torch.int8)
    assert got['i16'] == (('INT', 16, True), torch.int16) and got['u16'] == (('INT', 16, False), torch.int16)
    assert got['u32'] == (('INT', 32, False), torch.int32) and got['i32'][1] == torch.int32
    assert got['u64'] == (('INT', 64, False), torch.int64) and got['i64'][1] == torch.int64
    assert [got[k][0] for k in ('ms', 'us', 'ns')] == [('TIMESTAMP', 'MILLIS'), ('TIMESTAMP', 'MICROS'), ('TIMESTAMP', 'NANOS')]
    assert all(got[k][1] == torch.int64 for k in ('ms', 'us', 'ns'))
    pq.write_table(pa.table({k: cols[k] for k in ('u8', 'u16', 'ms')}), str(tmp_path / 'b.parquet'), version='1.0')
    old = {l.name: l.logical for l in parquet.read_metadata(tmp_path / 'b.parquet').leaves}
    assert old['u8'] == ('INT', 8, False) and old['u16'] == ('INT', 16, False) and old['ms'] == ('TIMESTAMP', 'MILLIS')


def test_fixtures_have_the_shapes_the_device_tests_rely_on(files, tmp_path):
    from otto_amd import parquet
    P = parquet
    # the fallback: one column chunk with RLE_DICTIONARY and PLAIN data pages
    _, pages = P.page_table(files['fallback', N_BIG][0], pi.COLUMNS)
    encs = [p.encoding for p in pages[0, 'aid'] if p.page_type != P.DICTIONARY_PAGE]
    assert 8 in encs and 0 in encs and pages[0, 'aid'][0].page_type == P.DICTIONARY_PAGE
    # many pages per chunk, at the size the device test reads (the 2-bit `type` indices fill a 4 KiB page slowly)
    _, pages = P.page_table(pi.w_page4k(tmp_path, pi.ROWS[-1])[0], pi.COLUMNS)
    for c in pi.COLUMNS:
        assert sum(p.page_type == P.DATA_PAGE for p in pages[0, c]) >= 8, c
    # V2 headers, levels outside the body
    _, pages = P.page_table(files['v2', N_BIG][0], pi.COLUMNS)
    assert all(p.page_type in (P.DICTIONARY_PAGE, P.DATA_PAGE_V2) for pg in pages.values() for p in pg)
    assert any(p.def_len > 0 for pg in pages.values() for p in pg)
    # no compression, no dictionary, no levels, several row groups, the index column
    _, pages = P.page_table(files['none', N_BIG][0], pi.COLUMNS)
    assert not any(p.is_compressed for pg in pages.values() for p in pg)
    _, pages = P.page_table(files['nodict', N_BIG][0], pi.COLUMNS)
    assert all(p.page_type == P.DATA_PAGE and p.encoding == 0 for pg in pages.values() for p in pg)
    _, pages = P.page_table(files['required', N_BIG][0], pi.COLUMNS)
    assert all(p.def_len == 0 for pg in pages.values() for p in pg)
    meta, _ = P.page_table(files['rowgroups', N_BIG][0], pi.COLUMNS)
    assert [g.num_rows for g in meta.row_groups] == [30000, N_BIG - 30000]
    meta, _ = P.page_table(files['index', N_BIG][0], pi.COLUMNS)
    assert [l.name for l in meta.leaves] == pi.COLUMNS + ['__index_level_0__']
    assert len(files['twofile', N_BIG]) == 2
    # version='1.0': the writer emits the legacy dictionary encoding enum, so PLAIN_DICTIONARY is covered
    meta, pages = P.page_table(files['v1_0', N_BIG][0], pi.COLUMNS)
    ch = meta.row_groups[0].chunks['aid']
    with open(files['v1_0', N_BIG][0], 'rb') as f:
        f.seek(ch.start)
        raw = f.read(ch.length)
    enums = []
    for p in pages[0, 'aid']:
        h = P._Thrift(raw, p.header_off).struct()
        enums.append(h[7][2] if p.page_type == P.DICTIONARY_PAGE else h[5][2])
    assert enums[0] == 2 and set(enums[1:]) == {2}, enums            # PLAIN_DICTIONARY on the dictionary and the data pages
    meta, pages = P.page_table(files['default', N_BIG][0], pi.COLUMNS)
    # bit widths
    for dtype in (np.int32, np.int64):
        for w in pi.WIDTHS + (20,):
            if w == 20 and dtype is np.int64:
                continue
            path = pi.w_width(tmp_path, w, dtype)[0]
            meta, pages = P.page_table(path, ['v'])
            data = [p for p in pages[0, 'v'] if p.page_type != P.DICTIONARY_PAGE]
            assert data and all(p.encoding == 8 for p in data), (w, dtype)
            for p in data:
                body = _body(path, meta.row_groups[0].chunks['v'], p)
                assert body[_index_start(body, p)] == max(w, 1), (w, dtype)     # the constant column: a 1-bit index, all 0
    path = pi.width0_file(tmp_path)
    meta, pages = P.page_table(path, ['v'])
    assert _body(path, meta.row_groups[0].chunks['v'], pages[0, 'v'][1])[0] == 0
    # run shapes
    rp = pi.w_runs(tmp_path)

    def runs_of(col):
        path = rp[col]
        meta, pages = P.page_table(path, [col])
        out = []
        for p in pages[0, col]:
            if p.page_type == P.DICTIONARY_PAGE:
                continue
            body = _body(path, meta.row_groups[0].chunks[col], p)
            pos, seen = _index_start(body, p), 0
            width = body[pos]
            pos += 1
            while seen < p.num_values:
                t = P._Thrift(body, pos)
                h = t.varint()
                n = (h >> 1) * 8 if h & 1 else h >> 1
                out.append((bool(h & 1), n, t.i - pos))
                pos = t.i + ((h >> 1) * width if h & 1 else (width + 7) // 8)
                seen += n
        return out
    r = runs_of('runs')
    assert any(not packed and hdr >= 3 and n >= 8192 for packed, n, hdr in r), r
    assert any(packed for packed, _, _ in r) and any(not packed for packed, _, _ in r)
    assert all(packed for packed, _, _ in runs_of('alternating'))
    _, pages = P.page_table(rp['padded'], ['padded'])
    assert sum(p.num_values for p in pages[0, 'padded']) % 8 != 0 and all(packed for packed, _, _ in runs_of('padded'))


def test_host_refusals(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_amd import _lib, parquet
    f = pi.frame(100)
    good = pi._write(tmp_path / 'good.parquet', f)[0]
    pi._write(tmp_path / 'zstd.parquet', f, compression='zstd')
    with pytest.raises(_lib.OttoError, match=r"zstd.parquet: column 'session', row group 0: codec ZSTD"):
        parquet.page_table(tmp_path / 'zstd.parquet', pi.COLUMNS)
    pq.write_table(pa.table({'session': f['session'], 'x': f['ts'].astype(np.float32)}), str(tmp_path / 'float.parquet'))
    with pytest.raises(_lib.OttoError, match=r"float.parquet: column 'x': physical type FLOAT"):
        parquet.page_table(tmp_path / 'float.parquet', ['session', 'x'])
    assert parquet.page_table(tmp_path / 'float.parquet', ['session'])[0].num_rows == 100      # an unrequested column is skipped
    pq.write_table(pa.table({'aid': pa.array([1, None, 3] * 10, type=pa.int32())}), str(tmp_path / 'null.parquet'), data_page_version='2.0')
    with pytest.raises(_lib.OttoError, match=r"null.parquet: column 'aid', row group 0, page 1: 10 null"):
        parquet.page_table(tmp_path / 'null.parquet', ['aid'])
    nested = pa.table({'session': pa.array([1, 2], type=pa.int32()), 'labels': pa.array([[1, 2], [3]], type=pa.list_(pa.int32())),
                       's': pa.array([{'a': 1, 'b': 2}, {'a': 3, 'b': 4}]), 'aid': pa.array([5, 6], type=pa.int32())})
    pq.write_table(nested, str(tmp_path / 'nested.parquet'))
    for col in ('labels', 's'):
        with pytest.raises(_lib.OttoError, match=f"nested.parquet: column '{col}': a repeated or nested column"):
            parquet.page_table(tmp_path / 'nested.parquet', ['session', col])
    meta, pages = parquet.page_table(tmp_path / 'nested.parquet', ['session', 'aid'])    # the groups are walked over by num_children
    assert [l.name for l in meta.leaves] == ['session', 'labels', 's', 'aid'] and pages[0, 'aid'][-1].num_values == 2
    with pytest.raises(_lib.OttoError, match=r"column 'nope': not in the file"):
        parquet.page_table(good, ['nope'])
    raw = open(good, 'rb').read()
    (tmp_path / 'cut.parquet').write_bytes(raw[len(raw) // 2:])
    with pytest.raises(_lib.OttoError, match=r'cut.parquet: (truncated footer|not a Parquet file)'):
        parquet.read_metadata(tmp_path / 'cut.parquet')
    (tmp_path / 'cut2.parquet').write_bytes(b'PAR1' + raw[-40:])
    with pytest.raises(_lib.OttoError, match=r'cut2.parquet: truncated footer'):
        parquet.read_metadata(tmp_path / 'cut2.parquet')
    (tmp_path / 'magic.parquet').write_bytes(b'PARQ' + raw[4:])
    with pytest.raises(_lib.OttoError, match=r'magic.parquet: not a Parquet file'):
        parquet.read_metadata(tmp_path / 'magic.parquet')
    (tmp_path / 'magic2.parquet').write_bytes(raw[:-4] + b'PAR2')
    with pytest.raises(_lib.OttoError, match=r'magic2.parquet: not a Parquet file'):
        parquet.read_metadata(tmp_path / 'magic2.parquet')
    (tmp_path / 'pare.parquet').write_bytes(raw[:-4] + b'PARE')
    with pytest.raises(_lib.OttoError, match=r'pare.parquet: encrypted footer'):
        parquet.read_metadata(tmp_path / 'pare.parquet')
    (tmp_path / 'tiny.parquet').write_bytes(b'PAR1')
    with pytest.raises(_lib.OttoError, match=r'tiny.parquet: not a Parquet file'):
        parquet.read_metadata(tmp_path / 'tiny.parquet')


def test_no_cpu_fallback_and_signatures():
    import torch
    from otto_amd import _lib, events, parquet
    with pytest.raises(_lib.OttoError, match='ROCm device'):
        parquet.read_columns([], pi.COLUMNS, 'cpu')
    with pytest.raises(_lib.OttoError, match='ROCm device'):
        parquet.snappy_decompress(torch.zeros(4, dtype=torch.uint8), [0], [4], [4])
    with pytest.raises(_lib.OttoError, match='ROCm device'):
        events.parquet_to_events_device('nowhere.parquet', device='cpu')
    for name in ('otto_parquet_workspace', 'otto_parquet_decode', 'otto_parquet_snappy', 'otto_parquet_snappy_workspace'):
        assert name in _lib.SIGNATURES
    assert parquet.TILE == 1024 and len(parquet.FIELDS) == 12
    src = open(parquet.__file__).read()
    assert 'import pyarrow' not in src and 'from pyarrow' not in src


def test_snappy_builders_against_pyarrow():
    """the hand encoder and its decoder against the real codec: pyarrow decompresses every hand-built stream to what the
    reference decoder gives, and refuses every malformed one that carries a preamble of its declared length"""
    import pyarrow as pa
    codec = pa.Codec('snappy')
    hs = pi.hand_streams()
    assert {'literal0_60', 'literal1_61', 'literal2_257', 'literal3_300', 'literal4_17', 'copy1', 'copy2', 'copy4'} <= set(hs)
    for name, (buf, n) in hs.items():
        want = pi.decode(buf, n)
        assert len(want) == n and codec.decompress(buf, decompressed_size=n).to_pybytes() == want, name
    for name, (buf, n) in pi.malformed_streams().items():
        with pytest.raises(pi.SnappyError):
            pi.decode(buf, n)
    for data in pi.codec_inputs().values():
        buf = codec.compress(data, asbytes=True)
        assert pi.decode(buf, len(data)) == data


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/parquet_host_main.cpp with the sanitizers, as a stand-alone program."""
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build tools/parquet_host_main.cpp'
    exe = tmp_path_factory.mktemp('parquet_host') / 'parquet_host_main'
    subprocess.run([cxx, '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall',
                    '-I', os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'parquet_host_main.cpp'), '-o', str(exe)], check=True)
    return exe


def _host_decode(exe, tmp_path, path, columns):
    recs, cols = _flat(path, columns)
    t = tmp_path / 'table.txt'
    t.write_text(f'{len(recs)} {len(cols)}\n' + '\n'.join(' '.join(map(str, c)) for c in cols) + '\n' +
                 '\n'.join(' '.join(map(str, r)) for r in recs) + '\n')
    r = subprocess.run([str(exe), 'decode', str(path), str(t)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = r.stdout.split('\n')
    if lines[0] != 'OK':
        return lines[0]
    return [np.array(ln.split(), dtype=np.uint64) for ln in lines[1:1 + len(cols)]]


def _same_as_pyarrow(got, path, columns):
    want = pi.expected([path], columns)
    assert isinstance(got, list), got
    for g, c in zip(got, columns):
        w = want[c]
        w = w.astype('datetime64[ns]').astype(np.int64) if w.dtype.kind == 'M' else w
        assert np.array_equal(g, w.astype(np.int64).view(np.uint64)), (path, c)


@pytest.mark.parametrize('writer', list(pi.WRITERS))
def test_host_program_decodes_every_fixture(host_program, files, tmp_path, writer):
    for n in (0, 7, 1000, N_BIG):
        for path in files[writer, n]:
            _same_as_pyarrow(_host_decode(host_program, tmp_path, path, pi.COLUMNS), path, pi.COLUMNS)


def test_host_program_widths_and_runs(host_program, tmp_path):
    for dtype in (np.int32, np.int64):
        for w in pi.WIDTHS:
            path = pi.w_width(tmp_path, w, dtype)[0]
            _same_as_pyarrow(_host_decode(host_program, tmp_path, path, ['v']), path, ['v'])
    path = pi.w_width(tmp_path, 20, np.int32)[0]
    _same_as_pyarrow(_host_decode(host_program, tmp_path, path, ['v']), path, ['v'])
    got = _host_decode(host_program, tmp_path, pi.width0_file(tmp_path), ['v'])
    assert np.array_equal(got[0], np.full(1000, 42, dtype=np.uint64))
    for col, path in pi.w_runs(tmp_path).items():
        _same_as_pyarrow(_host_decode(host_program, tmp_path, path, [col]), path, [col])


def test_host_program_refuses_nulls_and_bad_indices(host_program, tmp_path):
    from otto_amd import parquet
    path, page = pi.null_v1_file(tmp_path)
    assert _host_decode(host_program, tmp_path, path, ['aid']) == f'ERR {page} 7'           # PQ_E_NULL
    path, page = pi.bad_index_file(tmp_path)
    assert _host_decode(host_program, tmp_path, path, ['aid']) == f'ERR {page} 10'          # PQ_E_INDEX
    assert parquet.page_table(path, ['aid'])[0].num_rows == 3000


def test_host_program_on_snappy_streams(host_program, tmp_path):
    import pyarrow as pa
    codec = pa.Codec('snappy')
    named = dict(pi.hand_streams())
    named.update(pi.malformed_streams())
    named.update({k: (codec.compress(d, asbytes=True), len(d)) for k, d in pi.codec_inputs().items()})
    args = []
    for i, (name, (buf, n)) in enumerate(named.items()):
        (tmp_path / f'{i}.snappy').write_bytes(buf)
        args += [str(n), str(tmp_path / f'{i}.snappy')]
    r = subprocess.run([str(host_program), 'snappy'] + args, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(named)
    for (name, (buf, n)), ln in zip(named.items(), lines):
        try:
            want = pi.decode(buf, n)
        except pi.SnappyError:
            assert ln.startswith('ERR '), name
            continue
        assert ln == 'OK ' + want.hex(), name
