"""Host side of the Parquet encoder (otto_amd/parquet_write.py) without a GPU: the Thrift compact writer against the reader
of otto_amd/parquet.py, the page table and the assembly of the images with the restatement (tests/parquet_write_restatement.py)
standing in for the device -- every file must read back through pyarrow and pandas with equal values and dtypes and through
``parquet.read_metadata`` -- and the element encoders of ``csrc/parquet_encode.h`` on the CPU: ``tools/pqwrite_host_main.cpp``
is compiled as a stand-alone program with the address and undefined-behaviour sanitizers and must give the restatement's
bytes on every edge list ``test_parquet_write_gpu.py`` sends to the device afterwards."""
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pyarrow.parquet as pq
import pytest

import parquet_write_restatement as R
from conftest import ROOT
from otto_amd import parquet, parquet_write as pw
from test_parquet_cpu import _host_decode, host_program as decode_program  # noqa: F401  (the decoder's program, PLAIN files)

EDGE = dict(page_rows=256, row_group_rows=512)


def _write(tmp_path, name, columns, cuts=None, encodings=None, **kw):
    n = len(next(iter(columns.values())))
    images = pw.encode_tables_host(columns, cuts or [0, n], encodings, body=R.page_body, **kw)
    paths = []
    for i, image in enumerate(images):
        paths.append(tmp_path / f'{name}_{i}.parquet')
        paths[-1].write_bytes(image)
    return paths


def _reads_back(path, columns, lo=0, hi=None):
    t = pq.read_table(path)
    df = pd.read_parquet(path)
    meta = parquet.read_metadata(path)
    assert t.column_names == list(columns) == list(df.columns) == [l.name for l in meta.leaves]
    for name, a in columns.items():
        a = a[lo:hi]
        got = t.column(name).to_numpy()
        assert got.dtype == a.dtype and df[name].dtype == a.dtype, (path, name, got.dtype, df[name].dtype)
        assert np.array_equal(got.view(np.uint8), a.view(np.uint8)) and np.array_equal(df[name].to_numpy().view(np.uint8), a.view(np.uint8)), (path, name)
    assert meta.num_rows == len(a) == sum(g.num_rows for g in meta.row_groups)
    assert isinstance(df.index, pd.RangeIndex)
    return meta


# ---- the Thrift writer -----------------------------------------------------------------------------------------------
def test_thrift_round_trip():
    W = pw
    inner = [(1, W.T_I32, -7), (2, W.T_BINARY, b'name'), (19, W.T_I64, -(2 ** 63)), (20, W.T_BOOL, True), (21, W.T_BOOL, False)]
    fields = [(1, W.T_I32, 2 ** 31 - 1), (2, W.T_I64, -1), (3, W.T_I64, 2 ** 63 - 1), (4, W.T_BYTE, 200), (5, W.T_I16, -32768),
              (6, W.T_DOUBLE, 1.5), (7, W.T_BINARY, 'schéma'), (8, W.T_LIST, (W.T_I32, list(range(14)))),
              (9, W.T_LIST, (W.T_I64, [-(2 ** 40)] * 15)), (10, W.T_LIST, (W.T_BINARY, [b'x'] * 16)),
              (26, W.T_LIST, (W.T_STRUCT, [inner, inner])), (27, W.T_STRUCT, inner), (300, W.T_I32, 5), (301, W.T_LIST, (W.T_I32, [])),
              (30000, W.T_LIST, (1, [True, False]))]
    raw = pw.thrift_bytes(fields)
    t = parquet._Thrift(raw)
    got = t.struct()
    assert t.i == len(raw)
    want_inner = {1: -7, 2: b'name', 19: -(2 ** 63), 20: True, 21: False}
    assert got == {1: 2 ** 31 - 1, 2: -1, 3: 2 ** 63 - 1, 4: 200 - 256, 5: -32768, 6: 1.5, 7: 'schéma'.encode(), 8: list(range(14)),
                   9: [-(2 ** 40)] * 15, 10: [b'x'] * 16, 26: [want_inner, want_inner], 27: want_inner, 300: 5, 301: [],
                   30000: [True, False]}
    assert raw[0] == 0x15 and raw[-1] == 0                   # field 1 as a delta of 1 with type i32; the stop byte
    with pytest.raises(ValueError):
        pw.thrift_bytes([(2, W.T_I32, 1), (2, W.T_I32, 1)])
    with pytest.raises(ValueError):
        pw.thrift_bytes([(1, W.T_I32, 2 ** 31)])


def test_page_header_is_what_the_reader_walks():
    h = parquet._Thrift(pw.page_header(1000, pw.DELTA, 123456)).struct()
    assert h == {1: 0, 2: 123456, 3: 123456, 5: {1: 1000, 2: 5, 3: 3, 4: 3}}


# ---- the page table ---------------------------------------------------------------------------------------------------
def test_layout_pages_never_cross_a_row_group_or_a_file():
    lay = pw.Layout(2, [0, 0, 1, 700, 700, 1900], 256, 512)
    assert [len(f) for f in lay.files] == [1, 1, 2, 1, 3]
    assert [[rows for rows, _ in f] for f in lay.files] == [[0], [1], [512, 187], [0], [512, 512, 176]]
    seen = np.zeros((2, 1900), dtype=int)
    for r, k, j in lay.pages.tolist():
        assert 0 <= k <= 256
        seen[j, r:r + k] += 1
    assert (seen == 1).all()
    for f in lay.files:
        for rows, per_column in f:
            for idx in per_column:
                assert sum(int(lay.pages['n_values'][p]) for p in idx) == rows and len(idx) == max(1, -(-rows // 256))
    for bad in (dict(page_rows=100), dict(page_rows=256, row_group_rows=384), dict(page_rows=0)):
        with pytest.raises(ValueError):
            pw.Layout(1, [0, 10], **{**dict(row_group_rows=512), **bad})
    with pytest.raises(ValueError):
        pw.Layout(1, [0, 10, 5], 256, 512)


# ---- files through pyarrow, pandas and the project's own footer reader -------------------------------------------------
@pytest.mark.parametrize('n', R.EDGE_ROWS)
def test_delta_edge_sizes_read_back(tmp_path, n):
    cols = {'aid_x': R.pattern('runs_of_20', n), 'aid_y': R.pattern('random_aids', n, seed=n), 'big': R.pattern('alt_int64', n)}
    path, = _write(tmp_path, 'edge', cols, encodings={k: 'delta' for k in cols}, **EDGE)
    meta = _reads_back(path, cols)
    assert len(meta.row_groups) == max(1, -(-n // 512))
    for g in meta.row_groups:
        assert all(c.encodings == (5, 3) and c.codec == 0 for c in g.chunks.values())


@pytest.mark.parametrize('name', R.PATTERNS)
def test_delta_patterns_read_back(tmp_path, name):
    for n in R.PATTERN_ROWS:
        cols = {'v': R.pattern(name, n)}
        _reads_back(_write(tmp_path, f'{name}{n}', cols, encodings={'v': 'delta'}, **EDGE)[0], cols)


def test_delta_every_width_reads_back(tmp_path):
    for w, v in R.width_cases():
        _reads_back(_write(tmp_path, f'w{w}', {'v': v}, encodings={'v': 'delta'}, **EDGE)[0], {'v': v})


@pytest.mark.parametrize('dtype', R.PLAIN_DTYPES)
def test_plain_every_element_type_reads_back_as_its_dtype(tmp_path, dtype, decode_program):
    for n in R.PLAIN_ROWS:
        cols = {'v': R.plain_column(dtype, n), 'w': R.plain_column(dtype, n, seed=5)}
        path, = _write(tmp_path, f'{dtype}{n}', cols, **EDGE)
        meta = _reads_back(path, cols)                       # the converted_type of the narrow and unsigned kinds included
        leaf = meta.leaves[0]
        dt = np.dtype(dtype)
        if dt.kind == 'f':
            assert leaf.physical == (4 if dt.itemsize == 4 else 5) and leaf.logical is None
            continue
        assert leaf.physical == (2 if dt.itemsize == 8 else 1)
        assert leaf.logical == (None if dtype in ('int32', 'int64') else ('INT', 8 * dt.itemsize, dt.kind == 'i'))
        # the decoder of this project reads the PLAIN pages too (its stand-alone program, under the sanitizers)
        got = _host_decode(decode_program, tmp_path, path, ['v', 'w'])
        assert isinstance(got, list), got
        for g, name in zip(got, ('v', 'w')):
            assert np.array_equal(g, cols[name].astype(np.int64).view(np.uint64)), (dtype, n, name)


def test_delta_of_narrow_and_unsigned_columns(tmp_path):
    cols = {'a': np.arange(300, dtype=np.uint8), 'b': (np.arange(300) * 100).astype(np.uint16), 'c': np.arange(300, dtype=np.int8) & 0x7F,
            'd': np.arange(300, dtype=np.uint32) * 7000000, 'e': np.arange(300, dtype=np.uint64) << 53}
    _reads_back(_write(tmp_path, 'narrow', cols, encodings={k: 'delta' for k in cols}, **EDGE)[0], cols)


def test_six_segments_with_empty_ones(tmp_path):
    n = 1400
    cols = {'aid_x': R.pattern('runs_of_20', n), 'aid_y': R.pattern('random_aids', n), 'wgt': np.random.default_rng(1).random(n).astype(np.float32)}
    cuts = [0, 0, 1, 600, 1399, 1400, 1400]
    paths = _write(tmp_path, 'seg', cols, cuts=cuts, encodings={'aid_x': 'delta', 'aid_y': 'delta'}, **EDGE)
    assert len(paths) == 6
    for p, lo, hi in zip(paths, cuts, cuts[1:]):
        _reads_back(p, cols, lo, hi)


def test_default_page_and_row_group_sizes(tmp_path):
    n = (1 << 16) + 3
    cols = {'v': R.pattern('random_aids', n)}
    path, = _write(tmp_path, 'default', cols, encodings={'v': 'delta'})
    meta = _reads_back(path, cols)
    assert len(meta.row_groups) == 1
    _, pages = parquet_pages(path)
    assert [p.num_values for p in pages] == [1 << 16, 3]


def parquet_pages(path):
    meta = parquet.read_metadata(path)
    c = meta.row_groups[0].chunks['v']
    with open(path, 'rb') as f:
        f.seek(c.start)
        buf = f.read(c.length)
    pages, pos = [], 0
    while pos < len(buf):                                     # walk_pages refuses delta pages; only the headers are read here
        t = parquet._Thrift(buf, pos)
        h = t.struct()
        pages.append(parquet.Page(pos, t.i, h[3], h[2], h[1], h[5][2], 0, 0, h[5][1], 0))
        pos = t.i + h[3]
    return meta, pages


def test_refusals_of_the_host_side():
    a = np.arange(10, dtype=np.int32)
    with pytest.raises(ValueError, match='integer'):
        pw.encode_tables_host({'f': a.astype(np.float32)}, [0, 10], {'f': 'delta'}, body=R.page_body)
    with pytest.raises(ValueError, match='rows'):
        pw.encode_tables_host({'a': a, 'b': a[:5]}, [0, 5], body=R.page_body)
    with pytest.raises(ValueError, match='cuts'):
        pw.encode_tables_host({'a': a}, [0, 11], body=R.page_body)
    with pytest.raises(ValueError, match='not there'):
        pw.encode_tables_host({'a': a}, [0, 10], {'b': 'delta'}, body=R.page_body)
    with pytest.raises(ValueError, match='element type'):
        pw.encode_tables_host({'a': a.astype(np.float16)}, [0, 10], body=R.page_body)


# ---- csrc/parquet_encode.h under the sanitizers -------------------------------------------------------------------------
@pytest.fixture(scope='module')
def encode_program(tmp_path_factory):
    """tools/pqwrite_host_main.cpp with the sanitizers, as a stand-alone program."""
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build tools/pqwrite_host_main.cpp'
    exe = tmp_path_factory.mktemp('pqwrite_host') / 'pqwrite_host_main'
    subprocess.run([cxx, '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall',
                    '-I', os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'pqwrite_host_main.cpp'), '-o', str(exe)], check=True)
    return exe


def _host_encode(exe, arrays):
    text = ''.join(f'{R.stored(a).dtype.itemsize} {len(a)}\n' + ' '.join(str(int(x)) for x in R.stored(a)) + '\n' for a in arrays)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(arrays)
    return lines


def test_host_program_gives_the_restatement_bytes(encode_program):
    arrays = [R.pattern('random_aids', n, seed=n) for n in R.EDGE_ROWS] + [R.pattern('runs_of_20', n) for n in R.EDGE_ROWS]
    arrays += [R.pattern(name, n) for name in R.PATTERNS for n in R.PATTERN_ROWS]
    arrays += [v for _, v in R.width_cases()]
    arrays += [R.pattern('alt_int64', 1025), np.array([2 ** 31 - 1], dtype=np.int32), np.array([2 ** 62 - 1, 0], dtype=np.int64)]
    for a, line in zip(arrays, _host_encode(encode_program, arrays)):
        assert line == R.delta_body(a).hex(), (a.dtype, len(a))


def test_host_program_names_the_smallest_row_outside_the_domain(encode_program):
    a = R.pattern('random_aids', 300)
    neg, big, u32 = a.copy(), a.astype(np.int64), a.astype(np.uint32)
    neg[[77, 200]] = -1
    big[[5, 6]] = 2 ** 62
    u32[130] = 2 ** 31                                        # stored as its bit pattern: negative as INT32
    lines = _host_encode(encode_program, [neg, big, u32])
    assert lines == ['DOMAIN 77', 'DOMAIN 5', 'DOMAIN 130']
    for bad, row in ((neg, 77), (big, 5), (u32, 130)):
        with pytest.raises(R.DomainError) as e:
            R.delta_body(bad)
        assert e.value.row == row
