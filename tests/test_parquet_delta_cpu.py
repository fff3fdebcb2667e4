"""DELTA_BINARY_PACKED pages and float columns without a GPU (SPEC-PARQUET, include/otto_parquet.h): the host side of
otto_amd/parquet.py accepts what it refused before; the restatement (tests/parquet_delta_restatement.py) decodes the pages
pyarrow writes and the pages the project's writer writes to pyarrow's own values, and pyarrow reads the restatement's
encoder at every block shape; the delta helpers of ``csrc/parquet_decode.h`` on the CPU: ``tools/parquet_delta_host_main.cpp``
is compiled as a stand-alone program with the address and undefined-behaviour sanitizers and must print the restatement's
values and refusal codes on the bodies ``test_parquet_delta_gpu.py`` sends to the device afterwards."""
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_delta_restatement as D
import parquet_write_restatement as R
from conftest import ROOT
from otto_amd import _lib, parquet, parquet_write as pw

PYARROW_ROWS = (1, 129, 130, 300, 777, 1000)


# ---- inputs shared with the GPU tests ----------------------------------------------------------------------------------
def arrow_columns(n, seed=0):
    """int32 and int64 columns with small steps, wrapping steps and arbitrary values"""
    return {'a32': D.random_column(32, n, seed), 'w32': D.wrap_around(32, n), 'r32': D.random_column(32, n, seed + 1, 'any'),
            'a64': D.random_column(64, n, seed + 2), 'w64': D.wrap_around(64, n), 'r64': D.random_column(64, n, seed + 3, 'any')}


def write_arrow(path, cols, required=False, **kw):
    """pyarrow's writer with every column delta-coded (``kw``: page version, compression, page and row group sizes)"""
    table = pa.table(cols)
    if required:
        table = pa.Table.from_arrays(table.columns, schema=pa.schema([pa.field(f.name, f.type, nullable=False) for f in table.schema]))
    kw.setdefault('compression', 'none')
    if 'data_page_size' in kw:
        kw.setdefault('write_batch_size', 64)             # the writer looks at the page size once per batch
    pq.write_table(table, str(path), use_dictionary=False, column_encoding={c: 'DELTA_BINARY_PACKED' for c in cols}, **kw)
    return str(path)


def page_bodies(path, column, floats=False):
    """(Page, the bytes behind its levels) of every data page of ``column`` of an uncompressed file, in file order"""
    meta, pages = parquet.page_table(path, [column], floats=floats)
    raw = open(path, 'rb').read()
    out = []
    for (g, _), plist in sorted(pages.items()):
        c = meta.row_groups[g].chunks[column]
        for p in plist:
            if p.page_type == parquet.DICTIONARY_PAGE:
                continue
            assert not p.is_compressed
            b = raw[c.start + p.src_off:c.start + p.src_off + p.comp_size]
            if p.page_type == parquet.DATA_PAGE and p.def_len == -1:
                b = b[4 + int.from_bytes(b[:4], 'little'):]
            elif p.page_type == parquet.DATA_PAGE_V2:
                b = b[p.def_len + p.rep_len:]
            out.append((p, b))
    return out


def own_file(path, cols, B=128, M=4, garbage=None, page_rows=4096, row_group_rows=None, bodies=None):
    """A file of the project's writer whose delta bodies come from the restatement's encoder at block shape (B, M).
    ``bodies``: {(column index, first row): bytes} to put in place of a page's body."""
    names = list(cols)

    def body(a, enc):
        if enc != pw.DELTA:
            return R.page_body(a, enc)
        v, bits = D.stored(a)
        return D.encode(v, bits, B, M, garbage)
    lay = pw.Layout(len(names), [0, len(cols[names[0]])], page_rows, row_group_rows or page_rows)
    order = iter(lay.pages.tolist())

    def placed(a, enc):
        r, k, j = next(order)
        return (bodies or {}).get((j, r)) or body(a, enc)
    image, = pw.encode_tables_host(cols, [0, len(cols[names[0]])], {c: 'delta' for c in names if np.asarray(cols[c]).dtype.kind in 'iu'},
                                   page_rows=page_rows, row_group_rows=row_group_rows or page_rows, body=placed)
    with open(path, 'wb') as f:
        f.write(image)
    return str(path)


def patched_header(body, B=None, M=None, raw_B=None):
    """``body`` with another block size / miniblock count in its header (``raw_B``: the bytes of the first varint)"""
    b0, p = D._varint(body, 0)
    m0, q = D._varint(body, p)
    return (raw_B if raw_B is not None else D.uleb(b0 if B is None else B)) + D.uleb(m0 if M is None else M) + body[q:]


def refusal_bodies():
    """name -> (a page body of 130 INT32 values, num_values, the code SPEC-PARQUET refuses it with)"""
    n = 130
    v, bits = D.stored(D.random_column(32, n, 5))
    good = D.encode(v, bits)
    assert D.as_array(D.decode(good, n, 32), np.int32).tolist() == v
    _, p = D._varint(good, 0)
    _, p = D._varint(good, p)
    _, p = D._varint(good, p)
    _, p = D._varint(good, p)
    _, widths = D._varint(good, p)                           # the first block's width bytes
    assert good[widths] > 0
    wide = bytearray(good)
    wide[widths] = 33
    return {'width_33': (bytes(wide), n, D.WIDTH), 'count': (D.encode(v, bits, header_n=n + 1), n, D.COUNT),
            'cut_short': (good[:-1], n, D.TRUNC), 'trailing': (good + b'\0', n, D.TRAILING),
            'B_0': (patched_header(good, B=0), n, D.SHAPE), 'B_192': (patched_header(good, B=192), n, D.SHAPE),
            'M_0': (patched_header(good, M=0), n, D.SHAPE), 'mini_48': (patched_header(good, B=384, M=8), n, D.SHAPE),
            'varint_11': (patched_header(good, raw_B=b'\x80' * 10 + b'\x01'), n, D.VARINT)}


def restatement_cases():
    """(bits, B, M, values, garbage) of every body the GPU tests decode from the restatement's encoder"""
    out = []
    for B, M in D.SHAPES:
        for bits in (32, 64):
            out.append((bits, B, M, D.every_width(bits, B, M), 0xFF))
            for n in D.counts(B):
                out.append((bits, B, M, D.wrap_around(bits, n), 0xFF))
                out.append((bits, B, M, D.random_column(bits, n, n), None))
    return out


# ---- the host side accepts delta pages and, when asked, float columns ------------------------------------------------------
@pytest.mark.parametrize('version', ['1.0', '2.0'])
def test_page_table_accepts_pyarrow_delta_files(tmp_path, version):
    for n in PYARROW_ROWS:
        cols = arrow_columns(n)
        path = write_arrow(tmp_path / f'd{n}.parquet', cols, data_page_version=version)
        meta, pages = parquet.page_table(path, list(cols))
        for c in cols:
            plist = pages[0, c]
            assert [p.encoding for p in plist] == [5] * len(plist) and sum(p.num_values for p in plist) == n
            assert all(p.page_type == (parquet.DATA_PAGE_V2 if version == '2.0' else parquet.DATA_PAGE) for p in plist)


@pytest.mark.parametrize('version', ['1.0', '2.0'])
def test_restatement_decodes_pyarrow_pages(tmp_path, version):
    """pyarrow's INT32 blocks are 128 / 4, its INT64 blocks 256 / 4, and every page ends at its last needed miniblock"""
    for n in PYARROW_ROWS:
        cols = arrow_columns(n, seed=n)
        path = write_arrow(tmp_path / f'd{n}.parquet', cols, data_page_version=version, data_page_size=300)
        want = pq.read_table(path)
        for c, a in cols.items():
            bits = 8 * a.dtype.itemsize
            got = []
            for p, b in page_bodies(path, c):
                assert D._varint(b, 0)[0] == (128 if bits == 32 else 256)
                got += D.decode(b, p.num_values, bits)
            assert np.array_equal(D.as_array(got, a.dtype), want.column(c).to_numpy()) and np.array_equal(want.column(c).to_numpy(), a), (n, c)


def test_restatement_decodes_the_projects_writer(tmp_path):
    for n in (0, 1, 2, 129, 300, 1000):
        cols = {'x': R.pattern('runs_of_20', n), 'y': R.pattern('random_aids', n, seed=n), 'big': R.pattern('alt_int64', n)}
        image, = pw.encode_tables_host(cols, [0, n], {k: 'delta' for k in cols}, page_rows=256, row_group_rows=512, body=R.page_body)
        path = tmp_path / f'own{n}.parquet'
        path.write_bytes(image)
        want = pq.read_table(path)
        for c, a in cols.items():
            got = []
            for p, b in page_bodies(str(path), c):
                got += D.decode(b, p.num_values, 8 * a.dtype.itemsize)
            assert np.array_equal(D.as_array(got, a.dtype), want.column(c).to_numpy()), (n, c)


@pytest.mark.parametrize('shape', D.SHAPES, ids=lambda s: f'{s[0]}_{s[1]}')
def test_pyarrow_reads_the_restatement_encoder(tmp_path, shape):
    B, M = shape
    for bits in (32, 64):
        ew = D.every_width(bits, B, M)
        body = D.encode(D.stored(ew)[0], bits, B, M)
        assert D.widths_seen(body, len(ew)) == set(range(bits + 1))
        path = own_file(tmp_path / f'ew{bits}.parquet', {'v': ew}, B, M, garbage=0xFF, page_rows=len(ew) // 128 * 128 + 128)
        assert np.array_equal(pq.read_table(path).column('v').to_numpy(), ew)
        for n in D.counts(B):
            cols = {'w': D.wrap_around(bits, n), 'r': D.random_column(bits, n, n)}
            path = own_file(tmp_path / f'c{bits}_{n}.parquet', cols, B, M, garbage=0xFF)
            t = pq.read_table(path)
            for c, a in cols.items():
                assert np.array_equal(t.column(c).to_numpy(), a), (bits, n, c)
                plist = parquet.page_table(path, [c])[1][0, c]              # (an empty chunk's page is not walked)
                assert [p.encoding for p in plist] == [5] * (n > 0)


def test_floats_are_opt_in(tmp_path):
    path = str(tmp_path / 'f.parquet')
    pq.write_table(pa.table({'i': np.arange(5, dtype=np.int32), 'f': np.arange(5, dtype=np.float32), 'd': np.arange(5, dtype=np.float64)}), path)
    meta = parquet.read_metadata(path)
    for name, phys in (('f', 'FLOAT'), ('d', 'DOUBLE')):
        with pytest.raises(_lib.OttoError, match=f'physical type {phys} is not supported'):
            parquet.check_column(meta, name)
        with pytest.raises(_lib.OttoError, match=f'physical type {phys} is not supported'):
            parquet.page_table(path, [name])
        assert parquet.check_column(meta, name, floats=True).physical == parquet.PHYSICAL.index(phys)
    import torch
    assert parquet.default_dtype(parquet.check_column(meta, 'f', floats=True)) == torch.float32
    assert parquet.default_dtype(parquet.check_column(meta, 'd', floats=True)) == torch.float64
    _, pages = parquet.page_table(path, ['i', 'f', 'd'], floats=True)
    assert all(sum(p.num_values for p in pages[0, c] if p.page_type != parquet.DICTIONARY_PAGE) == 5 for c in 'ifd')


def test_a_delta_coded_float_page_is_refused_by_name(tmp_path):
    """no writer emits one: the encoding of a PLAIN float page is patched in its page header"""
    a = np.arange(7, dtype=np.float32)
    image = bytearray(pw.encode_tables_host({'f': a}, [0, 7], body=R.page_body)[0])
    head = pw.page_header(7, pw.PLAIN, 28)
    at = bytes(image).index(head)
    image[at:at + len(head)] = pw.page_header(7, pw.DELTA, 28)
    path = tmp_path / 'deltafloat.parquet'
    path.write_bytes(image)
    with pytest.raises(_lib.OttoError, match="column 'f', row group 0, page 0: encoding DELTA_BINARY_PACKED is not supported for a FLOAT column"):
        parquet.page_table(str(path), ['f'], floats=True)


# ---- csrc/parquet_decode.h under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def delta_program(tmp_path_factory):
    """tools/parquet_delta_host_main.cpp with the sanitizers, as a stand-alone program."""
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build tools/parquet_delta_host_main.cpp'
    exe = tmp_path_factory.mktemp('delta_host') / 'parquet_delta_host_main'
    subprocess.run([cxx, '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall',
                    '-I', os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'parquet_delta_host_main.cpp'), '-o', str(exe)], check=True)
    return exe


def _host_decode(exe, cases):
    text = ''.join(f'{bits // 8} {n} {body.hex() or "-"}\n' for bits, n, body in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(cases)
    return lines


def _want_line(bits, n, body):
    try:
        return ' '.join(str(v) for v in D.decode(body, n, bits)) or '-'
    except D.Refused as e:
        return f'REFUSED {e.code}'


def test_host_program_gives_the_restatement_values(delta_program):
    cases = []
    for bits, B, M, a, garbage in restatement_cases():
        cases.append((bits, len(a), D.encode(D.stored(a)[0], bits, B, M, garbage)))
    for bits in (32, 64):                                    # 65536 / 1: the largest accepted block, one miniblock
        a = D.random_column(bits, 70000, 1)
        cases.append((bits, len(a), D.encode(D.stored(a)[0], bits, 65536, 1)))
    for c, line in zip(cases, _host_decode(delta_program, cases)):
        assert not line.startswith('REFUSED') and line == _want_line(*c), (c[0], c[1])


def test_host_program_gives_the_restatement_refusals(delta_program):
    bad = refusal_bodies()
    cases = [(32, n, body) for body, n, _ in bad.values()]
    good = D.encode(D.stored(D.random_column(64, 300, 2))[0], 64, 256, 4)
    for cut in range(len(good)):                             # every prefix of a valid body: cut short, never read past
        cases.append((64, 300, good[:cut]))
    cases += [(64, 300, patched_header(good, B=65536 + 128)), (64, 300, patched_header(good, B=128, M=8)),
              (64, 300, patched_header(good, raw_B=b'\xff' * 9 + b'\x02')), (32, 0, b'\x80\x01\x04\x00\x00'), (32, 0, b'\x80\x01\x04\x00\x00\x00'),
              (32, 1, b'\x80\x01\x04\x01\x05'), (64, 1, b'\x80\x01\x04\x01' + b'\xff' * 9 + b'\x01')]
    lines = _host_decode(delta_program, cases)
    for (name, (_, _, code)), line in zip(bad.items(), lines):
        assert line == f'REFUSED {code}', name
        assert parquet_reason(code) == D.REASONS[code]
    for c, line in zip(cases, lines):
        assert line == _want_line(*c), c[:2]
    assert all(l == f'REFUSED {D.TRUNC}' for l in lines[len(bad):len(bad) + len(good)])
    assert lines[-7:] == [f'REFUSED {D.SHAPE}', f'REFUSED {D.SHAPE}', f'REFUSED {D.VARINT}', '-', f'REFUSED {D.TRAILING}', '4294967293',
                          str(2 ** 63)]


def parquet_reason(code):
    """the text of ``pq_reason`` in csrc/parquet_decode.h, read from the source (the library is not loaded without a GPU build)"""
    import re
    src = open(os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc', 'parquet_decode.h')).read()
    names = re.search(r'names\[PQ_N_REASONS\] = \{(.*?)\};', src, re.S).group(1)
    return re.findall(r'"((?:[^"\\]|\\.)*)"', names)[code]
