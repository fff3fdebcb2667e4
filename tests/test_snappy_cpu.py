"""SPEC-SNAPPY on the host: the restatement's streams are Snappy that pyarrow and the project's host decoder read back, they
stay inside the bound, three tiny streams are pinned byte for byte, and the Parquet host path writes compressed files whose
footers tell the truth. No GPU."""
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_write_restatement as R
import snappy_inputs
import snappy_restatement as S

INPUTS = snappy_inputs.inputs()


@pytest.fixture(scope='module')
def streams():
    return {name: S.compress(x) for name, x in INPUTS.items()}


def test_the_inputs_cover_what_the_spec_names():
    assert snappy_inputs.HASH_BYTES == S.HASH_BYTES and snappy_inputs.FRAGMENT == S.FRAGMENT
    lengths = {len(x) for x in INPUTS.values()}
    H = S.HASH_BYTES
    assert {0, 1, 3, H - 1, H, H + 1, 59, 60, 61, 63, 64, 65, 256, 257, 65535, 65536, 65537, 131073} <= lengths
    assert max(lengths) <= 400_000
    tokens = lambda name: [t for t in S.tokens(INPUTS[name][:S.FRAGMENT]) if isinstance(t, tuple)]
    # a planted repeat shorter than MIN_MATCH is not matched, a longer one is, and one of 65 bytes is cut at the cap
    assert tokens('match_len_3') == [] and tokens('match_len_4') == []
    assert tokens('match_len_11') == [(11, 500)] and tokens('match_len_12') == [(12, 500)] and tokens('match_len_64') == [(64, 500)]
    assert tokens('match_len_65')[0] == (64, 500)
    for dist in (2047, 2048):                                # both sides of the 1-byte-offset form's reach, at its lengths and above
        found = {length for length, d in tokens(f'match_dist_{dist}') if d == dist}
        assert {7, 11, 12} <= found
    assert tokens('match_to_fragment_end') == [(20, 100)] and tokens('match_to_stream_end') == [(30, 100)]
    # the repeat over the cut: its first half is a copy inside fragment 0, its second half is literals of fragment 1
    x = INPUTS['repeat_straddles_cut']
    assert (40, 100) in tokens('repeat_straddles_cut') and [t for t in S.tokens(x[S.FRAGMENT:]) if isinstance(t, tuple)] == []


@pytest.mark.parametrize('name', list(INPUTS))
def test_streams_decompress_and_stay_inside_the_bound(streams, name):
    from otto_amd import parquet
    x, z = INPUTS[name], streams[name]
    assert len(z) <= S.bound(len(x))
    back = pa.Codec('snappy').decompress(z, decompressed_size=len(x), asbytes=True) if x else b''
    assert back == x
    assert parquet._snappy_host(z, len(x)) == x
    if not x:
        assert z == b'\x00'


def test_the_element_forms_appear(streams):
    """Every form of SPEC-SNAPPY is written by some input, and the 4-byte-offset copy by none."""
    seen = set()
    for name, z in streams.items():
        i = len(S.uleb128(len(INPUTS[name])))
        while i < len(z):
            tag = z[i]
            kind = tag & 3
            assert kind != 3, name
            if kind == 0:
                ln = tag >> 2
                assert ln <= 61, name
                extra = 0 if ln < 60 else ln - 59
                n = ln + 1 if ln < 60 else int.from_bytes(z[i + 1:i + 1 + extra], 'little') + 1
                assert (n <= 60) == (extra == 0) and (n <= 256) == (extra <= 1), name
                seen.add(('literal', extra))
                i += 1 + extra + n
            else:
                ln = 4 + ((tag >> 2) & 7) if kind == 1 else 1 + (tag >> 2)
                d = (tag >> 5) << 8 | z[i + 1] if kind == 1 else int.from_bytes(z[i + 1:i + 3], 'little')
                assert S.MIN_MATCH <= ln <= 64 and d >= 1, name
                assert (kind == 1) == (ln <= 11 and d < 2048), name
                seen.add(('copy', kind))
                i += 1 + kind
    assert seen == {('literal', 0), ('literal', 1), ('literal', 2), ('copy', 1), ('copy', 2)}


def test_three_streams_by_hand():
    assert S.MIN_MATCH <= 8, 'the hand-computed streams below hold copies of 8 and 9 bytes'
    # a literal alone: preamble 3, tag (3 - 1) << 2, the bytes
    assert S.compress(b'abc') == bytes([0x03, 0x08]) + b'abc'
    # a run at distance 1: the literal 'a', then 9 bytes at distance 1 in the 1-byte-offset form 01 | (9 - 4) << 2, 01
    assert S.compress(b'a' * 10) == bytes([0x0A, 0x00]) + b'a' + bytes([0x15, 0x01])
    # the candidate p - 8: a literal of 8 (tag 7 << 2), then 8 bytes at distance 8: 01 | (8 - 4) << 2, 08
    assert S.compress(b'abcdefgh' * 2) == bytes([0x10, 0x1C]) + b'abcdefgh' + bytes([0x11, 0x08])


def test_the_restatement_reads_the_header():
    text = open(S.HEADER).read()
    for name, value in (('MIN_MATCH', S.MIN_MATCH), ('HASH_BYTES', S.HASH_BYTES), ('HASH_BITS', S.HASH_BITS), ('BATCH', S.BATCH),
                        ('MAX_MATCH', S.MAX_MATCH), ('FRAGMENT', S.FRAGMENT)):
        assert re.search(rf'^#define OTTO_SNAPPY_{name} {value}$', text, flags=re.M), name
    assert S.MIN_MATCH >= 4 and S.MAX_MATCH == 64 and S.FRAGMENT == 65536


def test_stored_stream_is_snappy():
    from otto_amd import snappy
    for name in ('random_0', 'random_1', 'random_60', 'random_61', 'random_256', 'random_257', 'random_65537'):
        x = INPUTS[name]
        z = snappy.stored_stream(x)
        assert (pa.Codec('snappy').decompress(z, decompressed_size=len(x), asbytes=True) if x else b'') == x


# ---- Parquet files on the host path ---------------------------------------------------------------------------------------
CUTS = [0, 0, 1, 700, 1000, 1000]
EDGE = dict(page_rows=256, row_group_rows=512)


def _columns():
    rng = np.random.default_rng(11)
    n = 1000
    return {'aid_x': np.sort(rng.integers(0, 1000, n)).astype(np.int32), 'aid_y': rng.integers(0, R.N_AIDS, n).astype(np.int32),
            'ts': (1_661_724_000 + np.cumsum(rng.integers(1, 50, n))).astype(np.int64), 'wgt': rng.integers(1, 5, n).astype(np.float32)}


@pytest.mark.parametrize('compression', ['snappy', {'wgt': 'snappy'}, {'aid_x': 'snappy', 'ts': 'snappy', 'wgt': None}])
def test_host_files_with_snappy_pages(compression):
    from otto_amd import parquet_write as pw
    cols = _columns()
    enc = {'aid_x': 'delta'}
    plain = pw.encode_tables_host(cols, CUTS, enc, body=R.page_body, **EDGE)
    images = pw.encode_tables_host(cols, CUTS, enc, body=R.page_body, compression=compression, compress=S.compress, **EDGE)
    packed = set(cols) if compression == 'snappy' else {k for k, v in compression.items() if v}
    for image, before, lo, hi in zip(images, plain, CUTS, CUTS[1:]):
        image = bytes(image)
        t = pq.read_table(pa.BufferReader(image))
        for name, a in cols.items():
            got = t.column(name).to_numpy()
            assert got.dtype == a.dtype and np.array_equal(got, a[lo:hi]), name
        md, md0 = pq.ParquetFile(pa.BufferReader(image)).metadata, pq.ParquetFile(pa.BufferReader(bytes(before))).metadata
        assert md.num_rows == hi - lo
        at = 4                                               # the chunks lie back to back behind the magic
        for g in range(md.num_row_groups):
            for j, name in enumerate(cols):
                c, c0 = md.row_group(g).column(j), md0.row_group(g).column(j)
                assert c.compression == ('SNAPPY' if name in packed else 'UNCOMPRESSED')
                assert c.data_page_offset == at and c.total_uncompressed_size == c0.total_compressed_size == c0.total_uncompressed_size
                if name not in packed:
                    assert c.total_compressed_size == c.total_uncompressed_size
                at += c.total_compressed_size
            assert md.row_group(g).total_byte_size == md0.row_group(g).total_byte_size
        assert at == len(image) - 8 - int.from_bytes(image[-8:-4], 'little')      # the footer follows the last page: the sizes are the bytes present
    assert sum(map(len, images)) < sum(map(len, plain))


def test_compression_none_changes_nothing():
    from otto_amd import parquet_write as pw
    cols = _columns()
    enc = {'aid_x': 'delta', 'aid_y': 'delta'}
    before = [bytes(i) for i in pw.encode_tables_host(cols, CUTS, enc, body=R.page_body, **EDGE)]
    assert [bytes(i) for i in pw.encode_tables_host(cols, CUTS, enc, body=R.page_body, compression=None, **EDGE)] == before
    assert [bytes(i) for i in pw.encode_tables_host(cols, CUTS, enc, body=R.page_body, compression={'wgt': None}, **EDGE)] == before
    lay = pw.Layout(1, [0, 300], 256, 512)                   # Layout.place with the arguments its callers have always passed
    old = lay.place(['a'], [pw.element(np.dtype('int32'))], [pw.PLAIN], [1024, 176])
    new = lay.place(['a'], [pw.element(np.dtype('int32'))], [pw.PLAIN], [1024, 176], [pw.UNCOMPRESSED], [1024, 176])
    assert old[0] == new[0] and old[1].tolist() == new[1].tolist() and old[2:] == new[2:]
    assert pw.page_header(7, 0, 28) == pw.page_header(7, 0, 28, 28) != pw.page_header(7, 0, 28, 9)


def test_bad_compression_arguments():
    from otto_amd import parquet_write as pw
    cols = _columns()
    for bad in ('gzip', {'wgt': 'zstd'}, {'nope': 'snappy'}, 5):
        with pytest.raises(ValueError, match='compression'):
            pw.encode_tables_host(cols, CUTS, body=R.page_body, compression=bad)
