"""Input builders of the Parquet decode tests (include/otto_parquet.h, otto_amd/parquet.py): OTTO-shaped frames and the
writer settings that give every page shape SPEC-PARQUET accepts, a Snappy encoder that emits each tag kind on demand, its
pure-Python decoder, and the malformed streams. Files are written at test time with pyarrow; nothing is read from
outside the test's own directory."""
import numpy as np

COLUMNS = ['session', 'aid', 'ts', 'type']
ROWS = (0, 1, 7, 8, 9, 63, 64, 65, 1000, 200003)
WIDTHS = (0, 1, 2, 3, 4, 7, 8, 9, 12, 16, 17)
RUN_LENGTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 500, 8191, 8192, 70000)


def frame(n, seed=0, random_aid=False, n_aids=50000):
    """An OTTO-shaped table as a dict of NumPy columns: sessions of 1 .. 40 events in order, aid skewed (uniform over
    [0, 2^31) with ``random_aid``), ts in ms, type 0 / 1 / 2."""
    rng = np.random.default_rng(seed + 1000 * n)
    lens = rng.integers(1, 41, size=n // 10 + 2)
    session = np.repeat(np.arange(len(lens), dtype=np.int32) * 3 + 11, lens)[:n]
    if random_aid:
        aid = rng.integers(0, 2 ** 31 - 1, size=n).astype(np.int32)
    else:
        aid = np.minimum(rng.zipf(1.3, size=n) - 1, n_aids - 1).astype(np.int32)
    ts = (1659304800000 + np.cumsum(rng.integers(0, 90000, size=n))).astype(np.int64)
    typ = rng.choice(np.array([0, 0, 0, 0, 1, 2], dtype=np.uint8), size=n)
    return {'session': session, 'aid': aid, 'ts': ts, 'type': typ}


def table(cols, nullable=True):
    import pyarrow as pa
    arrays = [pa.array(v) for v in cols.values()]
    return pa.table(arrays, schema=pa.schema([pa.field(k, a.type, nullable=nullable) for k, a in zip(cols, arrays)]))


def _write(path, cols, **kw):
    import pyarrow.parquet as pq
    nullable = kw.pop('nullable', True)
    pq.write_table(table(cols, nullable), str(path), **kw)
    return [str(path)]


def w_default(d, n):
    return _write(d / 'default.parquet', frame(n))


def w_page4k(d, n):
    return _write(d / 'page4k.parquet', frame(n), data_page_size=4096)


def w_fallback(d, n):
    return _write(d / 'fallback.parquet', frame(n, random_aid=True), dictionary_pagesize_limit=1 << 16)


def w_v2(d, n):
    return _write(d / 'v2.parquet', frame(n), data_page_version='2.0')


def w_none(d, n):
    return _write(d / 'none.parquet', frame(n), compression='none')


def w_nodict(d, n):
    return _write(d / 'nodict.parquet', frame(n), use_dictionary=False)


def w_rowgroups(d, n):
    return _write(d / 'rowgroups.parquet', frame(n), row_group_size=30000)


def w_v1_0(d, n):
    return _write(d / 'v1_0.parquet', frame(n), version='1.0')


def w_required(d, n):
    return _write(d / 'required.parquet', frame(n), nullable=False)


def w_index(d, n):
    """DataFrame.loc[...] + to_parquet: the index is no range any more and becomes an INT64 __index_level_0__ column"""
    import pandas as pd
    df = pd.DataFrame(frame(n))
    df = df.loc[df.index % 5 != 2] if n > 1 else df.loc[df.index >= 0]
    if n > 1:
        assert not isinstance(df.index, pd.RangeIndex)
    df.to_parquet(str(d / 'index.parquet'))
    return [str(d / 'index.parquet')]


def w_twofile(d, n):
    f = frame(n)
    cut = n // 3
    return (_write(d / 'two_a.parquet', {k: v[:cut] for k, v in f.items()}) +
            _write(d / 'two_b.parquet', {k: v[cut:] for k, v in f.items()}, data_page_version='2.0'))


WRITERS = {'default': w_default, 'page4k': w_page4k, 'fallback': w_fallback, 'v2': w_v2, 'none': w_none, 'nodict': w_nodict,
           'rowgroups': w_rowgroups, 'v1_0': w_v1_0, 'required': w_required, 'index': w_index, 'twofile': w_twofile}


def expected(paths, columns=COLUMNS):
    """{column: NumPy array} of pyarrow's own decode of the files, concatenated"""
    import pyarrow.parquet as pq
    tabs = [pq.read_table(p, columns=list(columns)) for p in paths]
    return {c: np.concatenate([t.column(c).to_numpy() for t in tabs]) for c in columns}


def width_rows(width):
    return 2 ** 19 + 5 if width == 20 else max(1000, (1 << width) + 37 if width else 1000)


def width_column(width, dtype):
    """A column whose dictionary needs exactly ``width`` index bits: every one of 2^(width-1) + 1 values (2^19 + 5 for width
    20) occurs; ``width`` 0 is the constant column, which pyarrow writes with 1-bit indices (width0_file has a true 0), the first occurrences in front so that every page is written with the full dictionary."""
    n = width_rows(width)
    card = 1 if width == 0 else n if width == 20 else (1 << (width - 1)) + 1
    rng = np.random.default_rng(width)
    idx = np.r_[np.arange(card), rng.integers(0, card, size=n - card)]
    scale = 3 if np.dtype(dtype).itemsize == 4 else 10 ** 12 + 7
    return (idx.astype(np.int64) * scale - 5).astype(dtype)


def w_width(d, width, dtype):
    name = f'width{width}_{np.dtype(dtype).name}.parquet'
    kw = {'max_rows_per_page': 1 << 20, 'data_page_size': 1 << 22}      # one data page, written with the whole dictionary
    if width == 20:
        kw['dictionary_pagesize_limit'] = 1 << 24
    return _write(d / name, {'v': width_column(width, dtype)}, **kw)


def width0_file(d):
    """pyarrow writes a one-entry dictionary with 1-bit indices, so the constant column of WIDTHS[0] has width 1. This is
    the same file (1000 x 42, REQUIRED, uncompressed) with its four index bytes rewritten to width 0: the width byte 0,
    then two RLE runs of 937 and 63 values that carry no value bytes."""
    path = _write(d / 'width0_patched.parquet', {'v': np.full(1000, 42, dtype=np.int32)}, compression='none', nullable=False)[0]
    from otto_amd import parquet
    meta, pages = parquet.page_table(path, ['v'])
    pg = pages[0, 'v']
    assert [p.page_type for p in pg] == [2, 0] and pg[1].comp_size == 4
    raw = bytearray(open(path, 'rb').read())
    at = meta.row_groups[0].chunks['v'].start + pg[1].src_off
    assert bytes(raw[at:at + 4]) == b'\x01' + varint(1000 << 1) + b'\x00'
    raw[at:at + 4] = b'\x00' + varint(937 << 1) + varint(63 << 1)
    open(path, 'wb').write(bytes(raw))
    return path


def w_runs(d):
    """{name: path} of one single-column file per run shape"""
    return {k: _write(d / f'runs_{k}.parquet', {k: v})[0] for k, v in run_columns().items()}


def null_v1_file(d):
    """(path, index of the violating page in the file's page table): a V1 file of 3000 int32 `aid` in three data pages with
    one null in the last page"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    vals = [int(v) for v in np.arange(3000) * 7]
    vals[2500] = None
    path = str(d / 'null_v1.parquet')
    pq.write_table(pa.table({'aid': pa.array(vals, type=pa.int32())}), path, data_page_size=300, use_dictionary=False)
    return path, 2


def bad_index_file(d):
    """(path, index of the violating page): an uncompressed V1 file of 3000 `aid` over five values (3-bit indices, one
    dictionary page and three data pages) whose third page is patched: the first packed group becomes eight indices of 7"""
    path = str(d / 'bad_index.parquet')
    _write(path, {'aid': (np.arange(3000) % 5).astype(np.int32) * 11}, compression='none', data_page_size=300)
    from otto_amd import parquet
    meta, pages = parquet.page_table(path, ['aid'])
    pg = pages[0, 'aid']
    assert [p.page_type for p in pg] == [2, 0, 0, 0] and all(p.encoding == 8 for p in pg[1:])
    ch = meta.row_groups[0].chunks['aid']
    raw = bytearray(open(path, 'rb').read())
    at = ch.start + pg[2].src_off
    at += 4 + int.from_bytes(raw[at:at + 4], 'little')          # over the definition levels
    assert raw[at] == 3                                          # the bit width
    at += 1
    assert raw[at] & 1                                           # a bit-packed run
    while raw[at] & 0x80:
        at += 1
    raw[at + 1:at + 4] = b'\xff\xff\xff'
    open(path, 'wb').write(bytes(raw))
    return path, 2


def codec_inputs():
    """{name: bytes} that the real compressor turns into streams: its literal / copy choices, the 64 KiB block edge"""
    rng = np.random.default_rng(1)
    return {'empty': b'', 'one': b'a', 'random70000': rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), 'equal100000': b'q' * 100000,
            'period3': b'abc' * 30000, 'period7': b'abcdefg' * 10001, 'aid_page': frame(100000)['aid'].tobytes()}


def run_columns():
    """{name: column} of the run shapes: sorted runs of RUN_LENGTHS (RLE runs, the longest with a 3-byte header varint),
    two values alternating (bit-packed runs only), and a length that is no multiple of 8 (padded last group)."""
    runs = np.repeat(np.arange(len(RUN_LENGTHS), dtype=np.int64) * 1000003, RUN_LENGTHS)
    return {'runs': runs, 'alternating': (np.arange(100003) % 2).astype(np.int32) * 77 + 1,
            'padded': (np.arange(1013) % 5).astype(np.int32)}


# ---------------------------------------------------------------------------------------------------------------------
# Snappy by hand
# ---------------------------------------------------------------------------------------------------------------------
def varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def literal(data, extra=None):
    """A literal element; ``extra``: the number of length bytes behind the tag (1 .. 4), None: the shortest form"""
    n = len(data) - 1
    assert n >= 0
    if extra is None:
        extra = 0 if n < 60 else (n.bit_length() + 7) // 8
    if extra == 0:
        assert n < 60
        return bytes([n << 2]) + bytes(data)
    assert n < 1 << (8 * extra)
    return bytes([(59 + extra) << 2]) + n.to_bytes(extra, 'little') + bytes(data)


def copy(offset, length, kind):
    """A copy element with a 1-, 2- or 4-byte offset (``kind`` 1, 2, 4)"""
    if kind == 1:
        assert 4 <= length <= 11 and 0 <= offset < 2048
        return bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 0xFF])
    assert 1 <= length <= 64
    return bytes([(2 if kind == 2 else 3) | (length - 1) << 2]) + offset.to_bytes(kind, 'little')


def stream(elements, declared):
    return varint(declared) + b''.join(elements)


class SnappyError(ValueError):
    pass


def decode(buf, declared):
    """The reference decoder of the hand-built streams: the bytes, or SnappyError where SPEC-PARQUET names a violation"""
    def vi(i):
        v = s = 0
        while True:
            if i >= len(buf) or s > 28:
                raise SnappyError('preamble')
            b = buf[i]
            i += 1
            v |= (b & 0x7F) << s
            s += 7
            if not b & 0x80:
                return v, i
    n, i = vi(0)
    if n != declared:
        raise SnappyError('preamble')
    out = bytearray()
    while i < len(buf):
        tag = buf[i]
        i += 1
        if tag & 3 == 0:
            ln = tag >> 2
            if ln >= 60:
                k = ln - 59
                if i + k > len(buf):
                    raise SnappyError('cut')
                ln = int.from_bytes(buf[i:i + k], 'little')
                i += k
            ln += 1
            if i + ln > len(buf):
                raise SnappyError('cut')
            if len(out) + ln > declared:
                raise SnappyError('overrun')
            out += buf[i:i + ln]
            i += ln
            continue
        if tag & 3 == 1:
            k, ln = 1, 4 + ((tag >> 2) & 7)
        else:
            k, ln = (2 if tag & 3 == 2 else 4), 1 + (tag >> 2)
        if i + k > len(buf):
            raise SnappyError('cut')
        off = int.from_bytes(buf[i:i + k], 'little') | ((tag >> 5) << 8 if k == 1 else 0)
        i += k
        if off == 0 or off > len(out):
            raise SnappyError('offset')
        if len(out) + ln > declared:
            raise SnappyError('overrun')
        for _ in range(ln):
            out.append(out[-off])
    if len(out) != declared:
        raise SnappyError('short')
    return bytes(out)


def hand_streams():
    """{name: (stream, declared length)} of valid streams that hold every tag kind: the five literal forms, the 1-, 2- and
    4-byte-offset copies, overlapping and far copies, a window refill in the middle of a tag run"""
    rng = np.random.default_rng(5)
    rnd = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    out = {}
    for extra, n in ((0, 1), (0, 60), (1, 61), (1, 256), (2, 257), (2, 60000), (3, 300), (3, 70001), (4, 17), (4, 1 << 17)):
        out[f'literal{extra}_{n}'] = ([literal(rnd(n), extra)], n)
    out['copy1'] = ([literal(rnd(20)), copy(20, 11, 1), copy(1, 4, 1), copy(7, 9, 1)], 44)
    out['copy2'] = ([literal(rnd(3000)), copy(3000, 64, 2), copy(2047, 1, 2), copy(3, 64, 2), copy(64, 64, 2)], 3193)
    out['copy4'] = ([literal(rnd(70000)), copy(70000, 64, 4), copy(65537, 33, 4), copy(1, 64, 4), copy(5, 2, 4)], 70163)
    many = [literal(rnd(9))] + [copy(1 + (i * 7) % 9, 4 + i % 8, 1) if i % 3 else literal(rnd(1 + i % 5)) for i in range(1500)]
    out['many_small'] = (many, None)
    far = [literal(rnd(2000), 2)] + [copy(2000, 64, 2 if i % 2 else 4) for i in range(40)]
    out['far_copies'] = (far, 2000 + 64 * 40)
    res = {}
    for k, (els, n) in out.items():
        body = b''.join(els)
        if n is None:
            n = _length(els)
        res[k] = (varint(n) + body, n)
    return res


def _length(elements):
    n = 0
    for e in elements:
        tag = e[0]
        if tag & 3 == 0:
            ln = tag >> 2
            n += (ln if ln < 60 else int.from_bytes(e[1:1 + ln - 59], 'little')) + 1
        elif tag & 3 == 1:
            n += 4 + ((tag >> 2) & 7)
        else:
            n += 1 + (tag >> 2)
    return n


def malformed_streams():
    """{name: (stream, declared length)}: each must come back with its status set and nothing written outside its extent"""
    lit4, lit8 = literal(b'abcd'), literal(b'abcdefgh')
    return {
        'cut_after_tag': (stream([lit4, copy(4, 4, 2)[:1]], 8), 8),
        'cut_after_tag_copy4': (stream([lit4, copy(4, 4, 4)[:3]], 8), 8),
        'cut_after_long_literal_tag': (stream([literal(b'x' * 300, 2)[:2]], 300), 300),
        'cut_inside_literal': (stream([literal(b'0123456789')[:6]], 10), 10),
        'cut_inside_long_literal': (stream([literal(b'y' * 5000, 2)[:3000]], 5000), 5000),
        'offset_0': (stream([lit4, copy(0, 4, 1)], 8), 8),
        'offset_0_copy4': (stream([lit4, copy(0, 4, 4)], 8), 8),
        'offset_past_produced': (stream([lit4, copy(5, 4, 2)], 8), 8),
        'offset_far_past': (stream([lit4, copy(2 ** 32 - 1, 4, 4)], 8), 8),
        'offset_before_any_output': (stream([copy(1, 4, 1)], 4), 4),
        'copy_past_declared': (stream([lit4, copy(4, 4, 1)], 6), 6),
        'literal_past_declared': (stream([lit8], 6), 6),
        'huge_literal_length': (stream([bytes([63 << 2]) + b'\xff\xff\xff\xff' + b'z' * 16], 16), 16),
        'preamble_larger': (stream([lit8], 9), 8),
        'preamble_smaller': (stream([lit8], 7), 8),
        'preamble_cut': (b'\x80\x80', 0),
        'preamble_too_long': (b'\x80\x80\x80\x80\x80\x01' + lit4, 4),
        'ends_short': (stream([lit4], 8), 8),
        'empty_input': (b'', 0),
    }
