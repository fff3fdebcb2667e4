"""List columns and dictionary-coded strings on the host (SPEC-PQLIST, include/otto_pqlist.h; otto_amd/parquet.py): the inputs
of the GPU tests meet the conditions they are there for, the restatement of the level decode (tests/pqlist_restatement.py)
equals pyarrow's own read on every one of them and refuses every damaged copy with the page and reason the device must name,
and every refusal the host makes without a device: the nested forms outside the three-level LIST, BIT_PACKED levels,
PLAIN / unmapped / oversized string dictionaries. ``read_columns`` keeps refusing nested and string columns as before."""
import numpy as np
import pytest

import pqlist_inputs as I
import pqlist_restatement as R

CASES = I.cases()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('pqlist')
    return {name: I.write(d / f'{name}.parquet', rws, **kw) for name, (rws, kw) in CASES.items()}


def _pyarrow(path):
    import pyarrow.parquet as pq
    return pq.read_table(path)[I.COLUMN].to_pylist()


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_equals_pyarrow(files, name):
    rws, kw = CASES[name]
    lists = _pyarrow(files[name])
    assert lists == ([r if r is not None else [] for r in rws] if not kw.get('outer_nullable', True) else rws)
    want = I.from_pylist(lists)
    off, null, n_values, _ = R.read_levels(files[name], I.COLUMN)
    assert np.array_equal(off, want[0]) and np.array_equal(null, want[2]) and n_values == len(want[1])


def test_the_inputs_hold_what_they_are_there_for(files):
    from otto_amd import parquet
    facts = {name: R.read_levels(path, I.COLUMN)[3] for name, path in files.items()}
    tables = {name: parquet.list_page_table(path, I.COLUMN) for name, path in files.items()}
    lens = sorted(len(r) for r in CASES['default'][0] if r)
    assert 1024 in lens and 2500 in lens and any(r is None for r in CASES['default'][0]) and [] in CASES['default'][0]
    for name in ('v1_page1k', 'v2_page1k', 'none_v1', 'plain', 'delta', 'int32', 'd1', 'd2_outer', 'd2_elem'):
        assert len(facts[name]) > 10, name                                       # many pages
        assert {'rle', 'packed'} <= set().union(*(f[4] for f in facts[name])), name
    assert all(f[2] == 0 for fs in facts.values() for f in fs)                   # pyarrow never cuts a page inside a row
    types = lambda name: {p.page_type for v in tables[name][1].values() for p in v}
    enc = lambda name: {p.encoding for v in tables[name][1].values() for p in v if p.page_type != 2}
    assert 3 in types('v2_page1k') and 3 in types('none_v2') and 3 not in types('v1_page1k')
    assert enc('plain') == {0} and enc('delta') == {5} and enc('delta_v2') == {5} and enc('v1_page1k') == {8}
    assert len(tables['rowgroups'][0].row_groups) > 3
    D = lambda name: 1 + tables[name][0].leaf.outer_optional + tables[name][0].leaf.elem_optional
    assert [D(n) for n in ('d1', 'd2_outer', 'd2_elem', 'default')] == [1, 2, 2, 3]
    assert tables['item_name'][0].leaf.path == (I.COLUMN, 'list', 'item') and tables['default'][0].leaf.path[2] == 'element'
    assert tables['int32'][0].leaf.physical == 1 and tables['default'][0].leaf.physical == 2
    assert tables['zero_rows'][0].num_rows == 0
    assert any(f[3] == 0 for f in facts['only_nulls'])                           # a page without a value
    codecs = lambda name: {c.codec for _, c in tables[name][0].row_groups}
    assert codecs('none_v1') == {0} and codecs('v1_page1k') == {1}


def test_the_hand_cut_file(tmp_path):
    rws, rep, dfn, vals, cuts = I.hand_case()
    path = I.hand_file(tmp_path / 'hand.parquet', rep, dfn, vals, cuts)
    assert _pyarrow(path) == rws
    off, null, n_values, facts = R.read_levels(path, I.COLUMN)
    want = I.expected(rws)
    assert np.array_equal(off, want[0]) and np.array_equal(null, want[2]) and n_values == len(vals)
    assert len(facts) >= 13 and sum(f[2] for f in facts) >= 8                    # pages that open inside a row
    assert any(f[3] == 0 for f in facts)                                         # a page made only of empty lists
    assert any(len(r) == 2500 for r in rws if r) and any(r is None for r in rws)
    for names in (('list', 'item'), ('bag', 'array_element')):                   # any field names
        p2 = I.hand_file(tmp_path / f'{names[1]}.parquet', rep, dfn, vals, cuts, names=names)
        assert np.array_equal(R.read_levels(p2, I.COLUMN)[0], want[0])


def test_every_damaged_copy_is_refused_by_the_restatement(tmp_path):
    for name, (path, page, code) in I.damaged(tmp_path).items():
        if code is None:
            R.read_levels(path, I.COLUMN)                                        # the levels are sound: the value decode refuses it
            continue
        with pytest.raises(R.Refused) as e:
            R.read_levels(path, I.COLUMN)
        assert (e.value.group, e.value.page, e.value.code) == (0, page, code), name


def test_hybrid_writer_round_trip():
    rng = np.random.default_rng(0)
    for width in (1, 2):
        for n in (0, 1, 7, 8, 9, 64, 1000):
            lev = np.where(rng.random(n) < 0.3, rng.integers(0, 1 << width, size=n), 1)
            lev[n // 2:n // 2 + 40] = 1
            b = I.hybrid(lev, width)
            got, _ = R.hybrid_decode(b, 0, len(b), width, n)
            assert got == lev.tolist()


# ---- host refusals ------------------------------------------------------------------------------------------------------------
def _refused(fn, *words):
    from otto_amd import _lib
    with pytest.raises(_lib.OttoError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def test_nested_forms_outside_the_list_form_are_refused_by_name(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from otto_amd import parquet
    REQ, OPT, REP = 0, 1, 2
    forms = {
        'two-level legacy list': [(I.COLUMN, OPT, None, 1, 3, 'top'), ('element', REP, 2, 0, None)],
        'a repeated primitive at top level': [(I.COLUMN, REP, 2, 0, None, 'top')],
        'a repeated group at top level': [(I.COLUMN, REP, None, 1, None, 'top'), ('x', REQ, 2, 0, None)],
        'a repeated group of 2 fields': [(I.COLUMN, OPT, None, 1, 3, 'top'), ('list', REP, None, 2, None), ('a', REQ, 2, 0, None),
                                         ('b', REQ, 2, 0, None)],
        'list element type DOUBLE': [(I.COLUMN, OPT, None, 1, 3, 'top'), ('list', REP, None, 1, None), ('element', OPT, 5, 0, None)],
    }
    for word, schema in forms.items():
        path = I.footer_file(tmp_path / 'form.parquet', schema)
        _refused(lambda: parquet.read_list_metadata(path, I.COLUMN), path, repr(I.COLUMN), word)
    tab = pa.table({'session': pa.array([1, 2]), 'll': pa.array([[[1], [2, 3]], []], type=pa.list_(pa.list_(pa.int64()))),
                    'st': pa.array([{'a': 1, 'b': 2}, {'a': 3, 'b': 4}]), 'one': pa.array([{'a': 1}, {'a': 3}]),
                    'mp': pa.array([[('k', 1)], []], type=pa.map_(pa.string(), pa.int64())),
                    'ls': pa.array([[{'a': 1}], []], type=pa.list_(pa.struct([('a', pa.int64())])))})
    path = str(tmp_path / 'nested.parquet')
    pq.write_table(tab, path)
    for col, word in (('ll', 'a list of lists'), ('st', 'a struct'), ('one', 'a struct'), ('mp', 'a map'), ('ls', 'a list of structs'),
                      ('session', 'not a list column'), ('nope', 'not in the file')):
        _refused(lambda: parquet.list_page_table(path, col), path, repr(col), word)
    for col in ('ll', 'st', 'mp'):                                               # read_columns: today's message
        _refused(lambda: parquet.page_table(path, [col]), 'a repeated or nested column is not supported')


def test_bit_packed_levels_are_refused_by_name(tmp_path):
    from otto_amd import parquet
    rws, rep, dfn, vals, cuts = I.hand_case()
    for enc, what in (((4, 3), 'definition'), ((3, 4), 'repetition')):
        path = I.hand_file(tmp_path / f'{what}.parquet', rep, dfn, vals, cuts, level_encodings=enc)
        _refused(lambda: parquet.list_page_table(path, I.COLUMN), path, 'row group 0, page 0', f'{what} level encoding BIT_PACKED')


def _strings(path, values, **kw):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({'type': pa.array(values)}), str(path), **kw)
    return str(path)


def test_string_columns_host_side(tmp_path):
    from otto_amd import parquet
    names = ['clicks', 'carts', 'orders']
    vals = [names[i % 3] for i in range(1000)]
    for kw in ({}, dict(compression='none'), dict(data_page_version='2.0'), dict(row_group_size=300)):
        path = _strings(tmp_path / 'ok.parquet', vals, **kw)
        n, groups = parquet.string_code_table(path, 'type', I.TYPE_CODES)
        assert n == 1000
        for where, c, buf, pages, dicts in groups:
            assert len(dicts) == 1 and sorted(next(iter(dicts.values())).tolist()) == [0, 1, 2]
    path = _strings(tmp_path / 'ok.parquet', vals)
    _refused(lambda: parquet.string_code_table(path, 'type', {'clicks': 0, 'carts': 1}), path, "column 'type', row group 0, page 0",
             "dictionary string 'orders' is not in the mapping")
    plain = _strings(tmp_path / 'plain.parquet', vals, use_dictionary=False)
    _refused(lambda: parquet.string_code_table(plain, 'type', I.TYPE_CODES), plain, 'row group 0, page 0', 'a PLAIN BYTE_ARRAY data page')
    big = _strings(tmp_path / 'big.parquet', [f'{i:040d}' for i in range(3000)])
    _refused(lambda: parquet.string_code_table(big, 'type', I.TYPE_CODES), big, 'page 0', 'a string dictionary page of', 'is not supported')
    _refused(lambda: parquet.page_table(path, ['type']), 'physical type BYTE_ARRAY is not supported (INT32, INT64)')      # read_columns: as before
    ints = I.write(tmp_path / 'ints.parquet', [[1]])
    _refused(lambda: parquet.string_code_table(ints, 'session', I.TYPE_CODES), 'is no string column')
    _refused(lambda: parquet.string_code_table(ints, I.COLUMN, I.TYPE_CODES), 'a repeated or nested column is not supported')


def test_snappy_host_equals_the_test_decoder():
    from otto_amd import parquet
    import parquet_inputs as PI
    for name, (buf, declared) in PI.hand_streams().items():
        assert parquet._snappy_host(buf, declared) == PI.decode(buf, declared), name
    for name, (buf, declared) in PI.malformed_streams().items():
        with pytest.raises(ValueError):
            parquet._snappy_host(buf, declared)


def test_read_lists_needs_a_device(files):
    from otto_amd import parquet
    _refused(lambda: parquet.read_lists(files['default'], I.COLUMN, 'cpu'), 'no CPU fallback')
    _refused(lambda: parquet.read_string_codes(files['default'], 'session', I.TYPE_CODES, 'cpu'), 'no CPU fallback')


# ---- the kernels' scalar code on the CPU, under the sanitizers ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tools/pqlist_host_main.cpp with the sanitizers, as a stand-alone program."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build tools/pqlist_host_main.cpp'
    exe = tmp_path_factory.mktemp('pqlist_host') / 'pqlist_host_main'
    subprocess.run([cxx, '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall',
                    '-I', os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'pqlist_host_main.cpp'), '-o', str(exe)], check=True)
    return exe


def _host_levels(exe, tmp_path, path, value_base=0):
    """the level job ``read_lists`` would hand the device for ``path``, run by the stand-alone program -> 'ERR page code' or
    (off, null, per-page report); the page of an ERR counts data pages, as the device's does"""
    import subprocess
    import parquet_inputs as PI
    from otto_amd import parquet
    meta, table = parquet.list_page_table(path, I.COLUMN)
    image, items = bytearray(), []
    with open(path, 'rb') as f:
        for g, pages in table.items():
            n, c = meta.row_groups[g]
            f.seek(c.start)
            b = f.read(c.length)
            items.append((f'row group {g}', meta.leaf, n, len(image), pages))
            image += b + bytes(-len(b) % 16)
    pl, infos, _, streams, end = parquet._list_plan(items, len(image))
    for src, n, dst, dst_len, *_ in streams:                                     # the V1 bodies, decoded behind the stored bytes
        assert dst == len(image)
        image += PI.decode(bytes(image[src:src + n]), dst_len)
    assert end == len(image)
    (tmp_path / 'image.bin').write_bytes(bytes(image))
    (tmp_path / 'table.txt').write_text(f'{len(pl)} {meta.num_rows} {value_base}\n' + '\n'.join(' '.join(map(str, r)) for r in pl) + '\n')
    r = subprocess.run([str(exe), str(tmp_path / 'image.bin'), str(tmp_path / 'table.txt')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = r.stdout.split('\n')
    if lines[0] != 'OK':
        return lines[0], infos
    return (np.array(lines[1].split(), dtype=np.int64), np.array(lines[2].split(), dtype=np.uint8),
            np.array([ln.split() for ln in lines[3:3 + len(pl)]], dtype=np.int64).reshape(-1, 3)), infos


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_program_equals_pyarrow(host_program, files, tmp_path, name):
    want = I.from_pylist(_pyarrow(files[name]))
    (off, null, report), _ = _host_levels(host_program, tmp_path, files[name], value_base=1000)
    assert np.array_equal(off, want[0] + 1000) and np.array_equal(null, want[2])
    assert report[:, 1].sum() == len(want[1]) and report[:, 2].sum() == len(want[2])


def test_host_program_on_the_hand_cut_and_damaged_files(host_program, tmp_path):
    rws, rep, dfn, vals, cuts = I.hand_case()
    for outer, elem in ((True, True), (False, False), (True, False), (False, True)):
        r2, d2, v2 = I.levels_of(rws, outer, elem)
        path = I.hand_file(tmp_path / 'hand.parquet', r2, d2, v2, cuts, outer, elem)
        (off, null, report), _ = _host_levels(host_program, tmp_path, path)
        want = I.expected(rws, outer)
        assert np.array_equal(off, want[0]) and np.array_equal(null, want[2])
    for name, (path, page, code) in I.damaged(tmp_path).items():
        got, _ = _host_levels(host_program, tmp_path, path)
        assert (got == f'ERR {page} {code}') if code else (not isinstance(got, str)), (name, got)


def test_host_program_and_restatement_agree_on_corrupted_level_bytes(host_program, tmp_path):
    """60 hand-cut files with a few random bytes of one page's levels overwritten: the stand-alone program stays inside every
    extent (the sanitizers are silent) and gives the restatement's verdict, page and reason, or its arrays"""
    from otto_amd import parquet
    rws, rep, dfn, vals, cuts = I.hand_case()
    clean = open(I.hand_file(tmp_path / 'clean.parquet', rep, dfn, vals, cuts), 'rb').read()
    meta, table = parquet.list_page_table(str(tmp_path / 'clean.parquet'), I.COLUMN)
    start = meta.row_groups[0][1].start
    report = _host_levels(host_program, tmp_path, str(tmp_path / 'clean.parquet'))[0][2]
    rng = np.random.default_rng(7)
    verdicts = set()
    for trial in range(60):
        k = int(rng.integers(0, len(table[0])))
        p = table[0][k]
        raw = bytearray(clean)
        for _ in range(int(rng.integers(1, 4))):
            raw[start + p.src_off + int(rng.integers(0, report[k, 0]))] = int(rng.integers(0, 256))
        path = str(tmp_path / 'bad.parquet')
        open(path, 'wb').write(bytes(raw))
        got, _ = _host_levels(host_program, tmp_path, path)
        try:
            off, null, n_values, _ = R.read_levels(path, I.COLUMN)
        except R.Refused as e:
            assert got == f'ERR {e.page} {e.code}', (trial, got, str(e))
            verdicts.add(e.code)
            continue
        assert not isinstance(got, str), (trial, got)
        assert np.array_equal(got[0], off) and np.array_equal(got[1], null)
        verdicts.add(0)
    assert len(verdicts) >= 4, verdicts                                          # several kinds of refusal were met
