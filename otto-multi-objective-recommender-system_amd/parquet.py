"""Device-side Parquet decode: the split files ``DATA/splits/*.parquet`` and the
part files of the reference's chunk writers -> device columns, unpacked by HIP kernels (``include/otto_parquet.h``,
SPEC-PARQUET): a Snappy decompressor, an RLE / bit-packed hybrid decoder, a dictionary gather and a DELTA_BINARY_PACKED
decoder. With ``floats=True`` FLOAT / DOUBLE columns (the ``wgt`` column of the covisitation part files) come back as bit copies.
``DATA/splits/val_labels.parquet`` is read by :func:`read_lists` (a three-level LIST column -> offsets, values, null flags;
``include/otto_pqlist.h``, SPEC-PQLIST) and :func:`read_string_codes` (a dictionary-coded string column -> the caller's codes);
:func:`read_columns` keeps refusing nested and string columns.

Reference code replaced: the pyarrow / pandas host decode in front of every consumer of the split files
(``src/ranker/aid_feature_engineering.py:21-36``). The host side here is pure Python + NumPy and imports no pyarrow: a
Thrift compact-protocol reader for the footer and the page headers (:func:`read_metadata`, :func:`walk_pages`), and
:func:`read_columns`, which reads the byte ranges of the requested column chunks into page-locked staging buffers and
sends them across as they lie in the file.

Every reader is built from the same host pieces: ``_parse_footer``, :func:`walk_pages` for flat and
list leaves, ``_plan_batches``, the staging pipeline ``_stage_batches``, ``_chunk_records`` and ``_refusal``.
"""
import os
import struct
from collections import namedtuple

import numpy as np

TILE = 1024                  # OTTO_PQ_TILE
FIELDS = ('src_off', 'comp_size', 'uncomp_size', 'page_type', 'encoding', 'def_len', 'rep_len', 'num_values', 'is_compressed',
          'out_row', 'col_slot', 'dict_slot')                                            # OTTO_PQ_* of a page record
F = {k: i for i, k in enumerate(FIELDS)}
PL_FIELDS = ('body_off', 'body_len', 'page_type', 'rep_len', 'def_len', 'num_values', 'flags', 'chunk_rows', 'chunk_pages')   # OTTO_PL_*
PL_OUTER_OPTIONAL, PL_ELEM_OPTIONAL, PL_CHUNK_FIRST = 1, 2, 4
PHYSICAL = ('BOOLEAN', 'INT32', 'INT64', 'INT96', 'FLOAT', 'DOUBLE', 'BYTE_ARRAY', 'FIXED_LEN_BYTE_ARRAY')
FLOAT, DOUBLE, BYTE_ARRAY = 4, 5, 6
CODECS = ('UNCOMPRESSED', 'SNAPPY', 'GZIP', 'LZO', 'BROTLI', 'LZ4', 'ZSTD', 'LZ4_RAW')
ENCODINGS = {0: 'PLAIN', 2: 'PLAIN_DICTIONARY', 3: 'RLE', 4: 'BIT_PACKED', 5: 'DELTA_BINARY_PACKED', 6: 'DELTA_LENGTH_BYTE_ARRAY',
             7: 'DELTA_BYTE_ARRAY', 8: 'RLE_DICTIONARY', 9: 'BYTE_STREAM_SPLIT'}
DATA_PAGE, INDEX_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 1, 2, 3
REQUIRED, OPTIONAL, REPEATED = 0, 1, 2
TICKS_PER_SECOND = {'MILLIS': 10 ** 3, 'MICROS': 10 ** 6, 'NANOS': 10 ** 9}
MAX_STRING_DICTIONARY = 64 << 10

Leaf = namedtuple('Leaf', 'name physical repetition logical nested')
# logical: None | ('INT', bits, signed) | ('TIMESTAMP', unit) | ('OTHER', name);  nested: a group, not a leaf
Chunk = namedtuple('Chunk', 'name physical codec num_values start length data_page_offset dictionary_page_offset uncompressed encodings')
RowGroup = namedtuple('RowGroup', 'num_rows chunks')              # chunks: {top-level name: Chunk}
Metadata = namedtuple('Metadata', 'path num_rows leaves row_groups')
Page = namedtuple('Page', 'header_off ' + ' '.join(FIELDS[:9]))   # offsets relative to the chunk's first byte
ListLeaf = namedtuple('ListLeaf', 'name path physical logical outer_optional elem_optional')
ListMetadata = namedtuple('ListMetadata', 'path num_rows leaf row_groups')       # row_groups: [(num_rows, Chunk or None)]


def _error(msg):
    from . import _lib
    return _lib.OttoError(msg)


def _sizes():
    """{torch dtype: bytes} of the integer dtypes a decode can store into"""
    import torch
    return {torch.uint8: 1, torch.int8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}


# ---------------------------------------------------------------------------------------------------------------------
# Thrift compact protocol: structs as {field id: value}; every wire type is read, so unknown fields are skipped by reading them
# ---------------------------------------------------------------------------------------------------------------------
class _Thrift:
    def __init__(self, buf, pos=0):
        self.b, self.i = buf, pos

    def byte(self):
        if self.i >= len(self.b):
            raise ValueError('Thrift data cut short')
        v = self.b[self.i]
        self.i += 1
        return int(v)

    def varint(self):
        v = shift = 0
        while True:
            b = self.byte()
            v |= (b & 0x7F) << shift
            if not b & 0x80:
                return v
            shift += 7
            if shift > 70:
                raise ValueError('Thrift varint too long')

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t):
        if t in (1, 2):                       # a bool outside a struct field: one byte
            return self.byte() == 1
        if t == 3:
            v = self.byte()
            return v - 256 if v > 127 else v
        if t in (4, 5, 6):
            return self.zigzag()
        if t == 7:
            self.i += 8
            if self.i > len(self.b):
                raise ValueError('Thrift data cut short')
            return struct.unpack('<d', bytes(self.b[self.i - 8:self.i]))[0]
        if t == 8:
            n = self.varint()
            if self.i + n > len(self.b):
                raise ValueError('Thrift data cut short')
            self.i += n
            return bytes(self.b[self.i - n:self.i])
        if t in (9, 10):
            h = self.byte()
            n = h >> 4
            if n == 15:
                n = self.varint()
            return [self.value(h & 15) for _ in range(n)]
        if t == 11:
            n = self.varint()
            if n == 0:
                return {}
            kv = self.byte()
            return {self.value(kv >> 4): self.value(kv & 15) for _ in range(n)}
        if t == 12:
            return self.struct()
        raise ValueError(f'Thrift wire type {t}')

    def struct(self):
        out, fid = {}, 0
        while True:
            h = self.byte()
            if h == 0:
                return out
            t = h & 15
            fid = fid + (h >> 4) if h >> 4 else self.zigzag()
            out[fid] = (t == 1) if t in (1, 2) else self.value(t)


def _logical(el):
    lt, ct = el.get(10), el.get(6)
    if lt:
        if 10 in lt:
            return ('INT', int(lt[10].get(1, 0)), bool(lt[10].get(2, False)))
        if 8 in lt:
            unit = lt[8].get(2, {})
            return ('TIMESTAMP', 'MILLIS' if 1 in unit else 'MICROS' if 2 in unit else 'NANOS')
        return ('OTHER', str(sorted(lt)))
    if ct is not None:
        if 11 <= ct <= 18:                    # UINT_8 .. UINT_64, INT_8 .. INT_64
            return ('INT', 8 << ((ct - 11) % 4), ct >= 15)
        if ct in (9, 10):
            return ('TIMESTAMP', 'MILLIS' if ct == 9 else 'MICROS')
        return ('OTHER', f'converted type {ct}')
    return None


def _footer(path):
    """(path as str, the bytes of the Thrift footer); ``OttoError`` on a wrong magic, an encrypted or truncated footer"""
    path = os.fspath(path)
    size = os.path.getsize(path)
    with open(path, 'rb') as f:
        head = f.read(4)
        if size < 12 or head not in (b'PAR1', b'PARE'):
            raise _error(f'{path}: not a Parquet file (magic {head!r}, {size} bytes)')
        f.seek(size - 8)
        tail = f.read(8)
        if tail[4:] == b'PARE' or head == b'PARE':
            raise _error(f'{path}: encrypted footer (PARE) is not supported')
        if tail[4:] != b'PAR1':
            raise _error(f'{path}: not a Parquet file (closing magic {tail[4:]!r})')
        n = struct.unpack('<I', tail[:4])[0]
        if n + 12 > size:
            raise _error(f'{path}: truncated footer ({n} bytes declared, {size} in the file)')
        f.seek(size - 8 - n)
        foot = f.read(n)
    return path, foot


def _top_level(schema):
    """``(index, element)`` of the top-level schema elements, one at a time; the subtree of a group is stepped over by its
    ``num_children`` only after the caller has looked at the element."""
    def skip(j):                              # the element at j and its subtree -> the index behind it
        kids = schema[j].get(5, 0) or 0
        j += 1
        for _ in range(kids):
            j = skip(j)
        return j
    i = 1
    for _ in range(schema[0].get(5, 0) or 0):
        yield i, schema[i]
        i = skip(i)


def _parse_footer(path, consume):
    """The one footer pass: ``consume(path, Thrift dict of the footer, its schema list)`` -> the reader's metadata. Raises
    ``OttoError`` on a wrong magic, an encrypted, truncated or malformed footer."""
    path, foot = _footer(path)
    try:
        md = _Thrift(foot).struct()
        return consume(path, md, md[2])
    except (ValueError, KeyError, IndexError) as e:
        raise _error(f'{path}: malformed footer ({e})') from None


def _chunk(name, cm):
    """The column-chunk metadata struct ``cm`` -> :class:`Chunk`; the chunk starts at its dictionary page where it has one"""
    dpo, dico = cm[9], cm.get(11)
    start = dico if dico is not None and 0 < dico < dpo else dpo
    return Chunk(name, cm[1], cm[4], cm[5], start, cm[7], dpo, dico, cm[6], tuple(cm[2]))


def read_metadata(path):
    """The footer of a Parquet file -> :class:`Metadata`: the top-level schema leaves (nested groups marked), the row groups
    and, per top-level primitive column, the chunk's byte range, codec, ``num_values`` and sizes. Raises ``OttoError`` on a
    wrong magic, an encrypted or truncated footer."""
    def consume(path, md, schema):
        leaves = [Leaf(el[4].decode(), el.get(1), el.get(3, REQUIRED), _logical(el), bool(el.get(5, 0))) for _, el in _top_level(schema)]
        groups = []
        for rg in md.get(4, []):
            chunks = {}
            for cc in rg[1]:
                pathn = [p.decode() for p in cc[3][3]]
                if len(pathn) == 1:
                    chunks[pathn[0]] = _chunk(pathn[0], cc[3])
            groups.append(RowGroup(rg[3], chunks))
        return Metadata(path, md[3], leaves, groups)
    return _parse_footer(path, consume)


def _name(table, k):
    return table[k] if isinstance(table, tuple) and 0 <= k < len(table) else table.get(k, f'#{k}') if isinstance(table, dict) else f'#{k}'


def _flat_leaf(meta, name):
    """The top-level leaf ``name`` of the file; ``OttoError`` where there is none or it is repeated or a group"""
    leaf = next((l for l in meta.leaves if l.name == name), None)
    if leaf is None:
        raise _error(f'{meta.path}: column {name!r}: not in the file (top-level columns: {[l.name for l in meta.leaves]})')
    if leaf.nested or leaf.repetition == REPEATED:
        raise _error(f'{meta.path}: column {name!r}: a repeated or nested column is not supported')
    return leaf


def check_column(meta, name, floats=False):
    """The leaf ``name`` of the file, or the ``OttoError`` SPEC-PARQUET names for a column that cannot be read.
    ``floats``: FLOAT / DOUBLE columns are accepted too."""
    leaf = _flat_leaf(meta, name)
    if leaf.physical not in (1, 2) and not (floats and leaf.physical in (FLOAT, DOUBLE)):
        raise _error(f'{meta.path}: column {name!r}: physical type {_name(PHYSICAL, leaf.physical)} is not supported (INT32, INT64)')
    return leaf


def _data_encoding(enc, leaf, where, k):
    """The OTTO_PQ_ENCODING of a data page: 0 PLAIN, 5 DELTA_BINARY_PACKED (integer columns), 8 dictionary indices."""
    if enc == 5 and leaf.physical in (FLOAT, DOUBLE):
        raise _error(f'{where}, page {k}: encoding DELTA_BINARY_PACKED is not supported for a {_name(PHYSICAL, leaf.physical)} column')
    if enc not in (0, 2, 5, 8):
        raise _error(f'{where}, page {k}: encoding {_name(ENCODINGS, enc)} is not supported')
    return 5 if enc == 5 else 8 if enc else 0


def walk_pages(buf, chunk, leaf, where):
    """The page headers of one column chunk -> a list of :class:`Page`. ``buf`` holds the chunk's bytes (``chunk.length``
    of them, from ``chunk.start``); only header bytes are touched. ``where``: the text that opens an error message.
    ``leaf``: a :class:`Leaf` or a :class:`ListLeaf`. For a list column ``num_values`` counts level entries, so nulls are no
    refusal; a V1 page must declare RLE for both level streams (BIT_PACKED is refused by name), a V2 page level lengths that
    fit its body. For a flat column only an OPTIONAL one has definition levels to check, and a V2 page with nulls is refused."""
    is_list = isinstance(leaf, ListLeaf)
    optional = not is_list and leaf.repetition == OPTIONAL
    level_streams = ('definition', 'repetition') if is_list else ('definition',) if optional else ()    # whose V1 encoding is checked
    pages, pos, seen, k = [], 0, 0, 0
    n = min(len(buf), chunk.length)
    while seen < chunk.num_values and pos < n:
        t = _Thrift(buf, pos)
        try:
            h = t.struct()
            ptype, uncomp, comp = h[1], h[2], h[3]
        except (ValueError, KeyError) as e:
            raise _error(f'{where}, page {k}: malformed page header ({e})') from None
        body = t.i
        if comp < 0 or uncomp < 0 or body + comp > n:
            raise _error(f'{where}, page {k}: the page runs past its column chunk')
        snappy = chunk.codec == 1
        if ptype == DICTIONARY_PAGE:
            d = h.get(7, {})
            if d.get(2, 0) not in (0, 2):
                raise _error(f'{where}, page {k}: dictionary page encoding {_name(ENCODINGS, d.get(2))} is not supported')
            pages.append(Page(pos, body, comp, uncomp, ptype, 0, 0, 0, d.get(1, 0), int(snappy)))
        elif ptype == DATA_PAGE:
            d = h.get(5, {})
            enc = _data_encoding(d.get(2, 0), leaf, where, k)
            for what, e in zip(level_streams, (d.get(3, 3), d.get(4, 3))):
                if e != 3:
                    raise _error(f'{where}, page {k}: {what} level encoding {_name(ENCODINGS, e)} is not supported{" (RLE)" if is_list else ""}')
            pages.append(Page(pos, body, comp, uncomp, ptype, enc, -1 if optional else 0, 0, d.get(1, 0), int(snappy)))
            seen += d.get(1, 0)
        elif ptype == DATA_PAGE_V2:
            d = h.get(8, {})
            enc = _data_encoding(d.get(4, 0), leaf, where, k)
            dl, rl = d.get(5, 0), d.get(6, 0)
            if is_list:
                if dl < 0 or rl < 0 or dl + rl > comp or dl + rl > uncomp:
                    raise _error(f'{where}, page {k}: level lengths run past the page body')
            elif d.get(2, 0) != 0:
                raise _error(f'{where}, page {k}: {d.get(2)} null(s): nulls are not supported')
            pages.append(Page(pos, body, comp, uncomp, ptype, enc, dl, rl, d.get(1, 0), int(snappy and d.get(7, True))))
            seen += d.get(1, 0)
        elif ptype != INDEX_PAGE:
            raise _error(f'{where}, page {k}: page type {ptype} is not supported')
        pos = body + comp
        k += 1
    if seen != chunk.num_values:
        raise _error(f'{where}: the pages hold {seen} {"level entries" if is_list else "values"}, the column chunk declares {chunk.num_values}')
    return pages


def _where(meta, name, g):
    return f'{meta.path}: column {name!r}, row group {g}'


def _check_chunk(c, where):
    """The chunk ``c`` of a requested column, or the ``OttoError`` for a missing one or a codec that cannot be read"""
    if c is None:
        raise _error(f'{where}: no column chunk')
    if c.codec not in (0, 1):
        raise _error(f'{where}: codec {_name(CODECS, c.codec)} is not supported (UNCOMPRESSED, SNAPPY)')
    return c


def check_row_group(meta, g, columns):
    """The chunks of the requested columns of row group ``g``, checked: codec, agreement on ``num_rows``."""
    rg = meta.row_groups[g]
    out = []
    for name in columns:
        c = _check_chunk(rg.chunks.get(name), _where(meta, name, g))
        if c.num_values != rg.num_rows:
            raise _error(f'{_where(meta, name, g)}: {c.num_values} values in a row group of {rg.num_rows} rows')
        out.append(c)
    return out


def page_table(path, columns, floats=False):
    """Host only: ``(metadata, {(row group, column): [Page]})`` of one file -- what :func:`read_columns` walks batch by batch,
    with every refusal the host can make (tests, tools)."""
    meta = read_metadata(path)
    leaves = [check_column(meta, c, floats) for c in columns]
    out = {}
    with open(meta.path, 'rb') as f:
        for g in range(len(meta.row_groups)):
            for leaf, c in zip(leaves, check_row_group(meta, g, columns)):
                f.seek(c.start)
                out[g, leaf.name] = walk_pages(f.read(c.length), c, leaf, _where(meta, leaf.name, g))
    return meta, out


def default_dtype(leaf):
    """The torch dtype of a column without an explicit one: what pyarrow's ``to_numpy`` gives where torch has it; unsigned
    16 / 32 / 64 as the signed type of the same width; a TIMESTAMP as its int64 ticks."""
    import torch
    lg = leaf.logical
    if leaf.physical in (FLOAT, DOUBLE):
        return torch.float32 if leaf.physical == FLOAT else torch.float64
    if lg and lg[0] == 'INT':
        bits, signed = lg[1], lg[2]
        if bits == 8:
            return torch.int8 if signed else torch.uint8
        return {16: torch.int16, 32: torch.int32, 64: torch.int64}[bits]
    return torch.int32 if leaf.physical == 1 else torch.int64


def _refusal(infos, i, code, reason_of, explain=None):
    """The ``OttoError`` for a device call that came back with violation ``code`` at record ``i``: ``infos[i]`` names file,
    column, row group and page, ``reason_of`` the library's ``*_reason`` by name; ``explain(i, reason)`` rewords the reason."""
    from . import _lib
    where, k = infos[i]
    reason = getattr(_lib.lib(), reason_of)(code).decode()
    return _error(f'{where}, page {k}: {explain(i, reason) if explain else reason}')


def _call(name, dev, *args, infos, reason_of, explain=None, **kw):
    """``_lib.call`` of an entry point whose last argument is the ``int64 [2]`` report (record, violation): a reported
    violation raises the :func:`_refusal` for it, any other failure the call's own ``OttoError``."""
    from . import _lib
    err = np.full(2, -1, dtype=np.int64)
    try:
        _lib.call(name, dev, *args, err, **kw)
    except _lib.OttoError:
        if err[0] < 0:
            raise
        raise _refusal(infos, int(err[0]), int(err[1]), reason_of, explain) from None


def _decode(dev, d_bytes, n_bytes, table, cols, infos, phases=3, work=None, explain=None):
    """One ``otto_parquet_decode`` call; a violation raises the ``OttoError`` that names file, column, row group and page.
    ``explain(record, reason)``: the text behind the page instead of the bare reason (``read_lists``)."""
    import ctypes as C
    from . import _lib
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(FIELDS))
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    need = int(_lib.lib().otto_parquet_workspace(table.ctypes.data_as(C.c_void_p), len(table)))
    if need < 0:
        _lib.check(need, 'otto_parquet_workspace')
    if work is None:
        work = _lib.workspace(need, dev)
    _call('otto_parquet_decode', dev, d_bytes, int(n_bytes), table, len(table), cols, len(cols), int(phases), work, int(work.numel()),
          infos=infos, reason_of='otto_parquet_reason', explain=explain)
    return work


def _read_full(f, view):
    got = 0
    while got < len(view):
        k = f.readinto(view[got:])
        if not k:
            break
        got += k
    return got


def _read_chunk(f, view, o, c, where):
    """The bytes of chunk ``c`` of the open file ``f``, read to ``view[o:]`` (a NumPy uint8 array) -> that stretch of ``view``"""
    f.seek(c.start)
    if _read_full(f, memoryview(view)[o:o + c.length]) != c.length:
        raise _error(f'{where}: the column chunk runs past the end of the file')
    return view[o:o + c.length]


def _paths(paths):
    return [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)


def _plan_batches(sizes, batch_bytes):
    """``sizes``: ``(stored bytes, budget bytes)`` per row group, in reading order -> the batches as lists of indices: greedy
    runs of whole row groups whose budgets add up to ``batch_bytes`` at most; a single larger row group is its own batch."""
    batches, cur, cur_bytes = [], [], 0
    for i, (_, budget) in enumerate(sizes):
        if cur and cur_bytes + budget > batch_bytes:
            batches.append(cur)
            cur, cur_bytes = [], 0
        cur.append(i)
        cur_bytes += budget
    if cur:
        batches.append(cur)
    return batches


def _largest_batch(sizes, batches):
    """``(stored bytes, budget bytes)`` of the largest batch, each on its own: what the staging sets must hold"""
    return tuple(max([sum(sizes[i][k] for i in b) for b in batches], default=0) for k in (0, 1))


def _stage_batches(dev, paths, batches, stage, room, fill, decode):
    """The staging pipeline of :func:`read_columns` and :func:`read_lists`: two page-locked host sets of ``stage`` bytes and
    two device sets of ``room`` bytes alternate; batch i + 1 is read and sent on a copy stream before batch i decodes on the
    caller's stream. ``fill(batch, view, file)`` reads the batch into the NumPy ``view`` of a host set (``file(i)``: ``paths[i]``,
    opened at first use and closed here) and returns ``(bytes, payload)``; ``decode(device set, bytes, payload)`` launches the
    batch on the caller's stream. Returns, or raises, with every file closed and the device synchronised."""
    import torch
    if batches:
        host = [torch.empty(max(stage, 16), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        devb = [torch.empty(max(room, 16), dtype=torch.uint8, device=dev) for _ in range(2)]
        copy_stream = torch.cuda.Stream(device=dev)
        compute = torch.cuda.current_stream(dev)
        # the device sets come from the caller's stream's allocator: a block it freed may still be read by work queued there
        copy_stream.wait_stream(compute)
        sent = [torch.cuda.Event(), torch.cuda.Event()]      # H2D of the set finished
        used = [torch.cuda.Event(), torch.cuda.Event()]      # the decode no longer reads the set
    files = {}

    def file(i):
        if i not in files:
            files[i] = open(paths[i], 'rb', buffering=0)
        return files[i]

    def prepared():
        """(staging set, bytes, payload) per batch, read and on its way to the device"""
        for i, batch in enumerate(batches):
            b = i & 1
            if i >= 2:
                used[b].synchronize()                        # the set is free again, host and device side
            n, payload = fill(batch, host[b].numpy(), file)
            with torch.cuda.stream(copy_stream):
                devb[b][:n].copy_(host[b][:n], non_blocking=True)
                sent[b].record(copy_stream)
            yield b, n, payload

    try:
        it = prepared()
        cur = next(it, None)
        while cur is not None:
            nxt = next(it, None)                             # read and send batch i + 1 before batch i decodes
            b, n, payload = cur
            compute.wait_event(sent[b])
            decode(devb[b], n, payload)
            used[b].record(compute)
            cur = nxt
    finally:
        for f in files.values():
            f.close()
        torch.cuda.synchronize(dev)


def _chunk_records(table, infos, where, pages, row, slot, place):
    """The OTTO_PQ records of one chunk's ``pages``, appended to ``table``, and their ``(where, page number)`` to ``infos``.
    ``place(k, page)`` says how page k lies in the device buffer: ``(src_off, comp_size, uncomp_size, page_type, def_len,
    rep_len, num_values, is_compressed)``, or None for a page that has no value to decode. ``row``: the output row of the
    chunk's first value, ``slot``: its column record. Returns the row behind the chunk's last value."""
    dict_slot = -1
    for k, p in enumerate(pages):
        is_dict = p.page_type == DICTIONARY_PAGE
        coded = not is_dict and p.encoding == 8
        if is_dict:
            dict_slot = len(table)
        elif coded and dict_slot < 0:
            raise _error(f'{where}, page {k}: dictionary-coded page without a dictionary page')
        rec = place(k, p)
        if rec is not None:
            table.append((*rec[:4], p.encoding, *rec[4:], row, slot, dict_slot if coded else -1))
            infos.append((where, k))
            row += 0 if is_dict else rec[6]
    return row


def _as_stored(p, src, num_values=None):
    """The ``place`` of a page that is decoded as it lies in the file, its body at ``src`` of the device buffer"""
    return src, p.comp_size, p.uncomp_size, p.page_type, p.def_len, p.rep_len, p.num_values if num_values is None else num_values, p.is_compressed


def _column_slot(cols, slots, j, physical, logical, out):
    """The slot of the column record that stores values of ``physical`` / ``logical`` type into ``out``, the tensor of output
    column ``j``: one record per (column, physical size, uint32 extension), appended to ``cols`` when it is new"""
    key = (j, 4 if physical in (1, FLOAT) else 8, int(physical == 1 and logical == ('INT', 32, False)))
    if key not in slots:
        slots[key] = len(cols)
        cols.append((out.data_ptr(), out.element_size(), out.numel(), key[1], key[2]))
    return slots[key]


def _fill_out(out, result, what):
    """``result`` copied into the caller's ``out`` tensors, which must match it in number, shape, dtype and device"""
    out = tuple(out)
    if len(out) != len(result) or any(o.shape != r.shape or o.dtype != r.dtype or o.device != r.device for o, r in zip(out, result)):
        raise ValueError(f'out: expected {what} with the shape, dtype and device of the result')
    for o, r in zip(out, result):
        o.copy_(r)
    return out


def read_columns(paths, columns, device, dtypes=None, batch_bytes=256 << 20, out=None, floats=False):
    """The columns ``columns`` of the files ``paths`` (one path or a list) -> a tuple of device tensors, the rows in file and
    row-group order. ``dtypes``: ``{name: torch.dtype}`` for columns that should not get :func:`default_dtype`; the cast
    (two's-complement truncation or sign extension, as ``numpy.astype``) happens in the decode kernel's store.
    ``floats=True``: FLOAT columns come back as ``torch.float32``, DOUBLE as ``torch.float64``, bit for bit, and no other
    dtype may be asked of them; without it such a column is refused.

    Only the byte ranges of the requested column chunks are read, into two page-locked staging buffers that alternate;
    batch i + 1 is read, its page headers walked and its bytes copied on a side stream while batch i decodes (the event
    hand-over of ``jsonl.read_columns``). A batch is a run of whole row groups whose compressed plus uncompressed bytes
    fit ``batch_bytes``; a single larger row group is its own batch. A refused file raises ``OttoError`` and writes nothing
    the caller can see: ``out`` (a tuple of tensors to fill instead of fresh ones) is written only after every batch came
    back clean."""
    import torch
    from . import _lib
    dev = _lib.rocm_device(device, 'parquet.read_columns')
    _lib.lib()
    paths = _paths(paths)
    columns = list(columns)
    dtypes = dict(dtypes or {})
    sizes = _sizes()
    metas = [read_metadata(p) for p in paths]
    leaves = [[check_column(m, c, floats) for c in columns] for m in metas]
    col_dt = []
    for j, c in enumerate(columns):
        dt = dtypes.get(c) or (default_dtype(leaves[0][j]) if metas else torch.int64)
        for lv in leaves:                                     # a float column is a bit copy: its own dtype or none
            if lv[j].physical in (FLOAT, DOUBLE) and dt != default_dtype(lv[j]):
                raise ValueError(f'dtypes[{c!r}]: {dt} for a {_name(PHYSICAL, lv[j].physical)} column; only {default_dtype(lv[j])} is possible')
            if lv[j].physical not in (FLOAT, DOUBLE) and dt not in sizes:
                raise ValueError(f'dtypes[{c!r}]: {dt} is not one of {sorted(map(str, sizes))}')
        if dt not in sizes and not dt.is_floating_point:
            raise ValueError(f'dtypes[{c!r}]: {dt} is not one of {sorted(map(str, sizes))}')
        col_dt.append(dt)
    # the batches: runs of whole row groups, over all files
    groups, extents, row = [], [], 0                          # (file, row group, chunks, first row); (compressed bytes, both)
    for fi, m in enumerate(metas):
        for g in range(len(m.row_groups)):
            chunks = check_row_group(m, g, columns)
            comp = sum((c.length + 15) & ~15 for c in chunks)
            groups.append((fi, g, chunks, row))
            extents.append((comp, comp + sum(c.uncompressed for c in chunks)))
            row += m.row_groups[g].num_rows
    n_rows = row
    batches = _plan_batches(extents, batch_bytes)
    stage, _ = _largest_batch(extents, batches)
    if stage >= 1 << 31:
        raise _lib.OttoError(f'a row group of {stage} compressed bytes does not fit one call (2^31)')
    with torch.cuda.device(dev):
        result = [torch.empty(n_rows, dtype=dt, device=dev) for dt in col_dt]

        def fill(batch, view, file):
            table, infos, o = [], [], 0
            cols, slots = [], {}                             # one record per (column, physical size, extension) of the batch
            for fi, g, chunks, row0 in (groups[i] for i in batch):
                f = file(fi)
                for j, c in enumerate(chunks):
                    where, leaf = _where(metas[fi], c.name, g), leaves[fi][j]
                    pages = walk_pages(_read_chunk(f, view, o, c, where), c, leaf, where)
                    slot = _column_slot(cols, slots, j, leaf.physical, leaf.logical, result[j])
                    _chunk_records(table, infos, where, pages, row0, slot, lambda k, p: _as_stored(p, o + p.src_off))
                    o += (c.length + 15) & ~15
            return o, (table, cols, infos)

        def decode(d_bytes, n, payload):
            if payload[0]:
                _decode(dev, d_bytes, n, *payload)
        _stage_batches(dev, [m.path for m in metas], batches, stage, stage, fill, decode)
        if out is not None:
            return _fill_out(out, result, 'one tensor per column')
    return tuple(result)


def snappy_decompress(d_bytes, src_off, src_len, dst_len, out=None, dst_off=None):
    """The decompressor alone (test seam): stream i is ``d_bytes[src_off[i] : src_off[i] + src_len[i]]`` and must decompress to
    exactly ``dst_len[i]`` bytes. Returns ``(out, status)``: ``out`` a device uint8 tensor that holds stream i at
    ``dst_off[i]`` (default: the streams back to back, in a fresh tensor), ``status`` an int32 NumPy array, 0 or the
    violation of stream i. Nothing outside a stream's own extent of ``out`` is written."""
    import torch
    from . import _lib
    if not isinstance(d_bytes, torch.Tensor) or d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1:
        raise ValueError('snappy_decompress: expected a 1-d uint8 tensor')
    if d_bytes.device.type != 'cuda':
        raise _lib.OttoError('snappy_decompress needs a ROCm device (no CPU fallback)')
    dev = d_bytes.device
    a = lambda v: np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.int64)))
    src_off, src_len, dst_len = a(src_off), a(src_len), a(dst_len)
    n = len(src_off)
    if len(src_len) != n or len(dst_len) != n:
        raise ValueError('snappy_decompress: src_off, src_len and dst_len must have one entry per stream')
    dst_off = a(np.r_[0, np.cumsum(dst_len)[:-1]] if dst_off is None else dst_off)
    if len(dst_off) != n:
        raise ValueError('snappy_decompress: dst_off must have one entry per stream')
    if out is None:
        out = torch.zeros(int((dst_off + dst_len).max()) if n else 0, dtype=torch.uint8, device=dev)
    _lib.need(out, 'snappy_decompress: out', torch.uint8, dim=1, device=dev)
    if not d_bytes.is_contiguous():
        d_bytes = d_bytes.contiguous()
    status = np.zeros(n, dtype=np.int32)
    with torch.cuda.device(dev):
        wb = int(_lib.lib().otto_parquet_snappy_workspace(n))
        work = _lib.workspace(wb, dev)
        _lib.call('otto_parquet_snappy', dev, d_bytes, int(d_bytes.numel()), src_off, src_len, dst_off, dst_len, n, out,
                  int(out.numel()), status, work, int(work.numel()))
    return out, status


# ---------------------------------------------------------------------------------------------------------------------
# list columns (include/otto_pqlist.h, SPEC-PQLIST) and dictionary-coded string columns: val_labels.parquet
# ---------------------------------------------------------------------------------------------------------------------
def read_list_metadata(path, column):
    """The footer of ``path`` for the list column ``column`` -> :class:`ListMetadata`. Accepted is the three-level LIST form
    of SPEC-PQLIST under any field names; every other nested form raises the ``OttoError`` that names it."""
    def consume(path, md, schema):
        at, names = None, []
        for i, el in _top_level(schema):
            names.append(el[4].decode())
            if names[-1] == column and at is None:
                at = i
        pre = f'{path}: column {column!r}'
        if at is None:
            raise _error(f'{pre}: not in the file (top-level columns: {names})')
        top = schema[at]
        kids = top.get(5, 0) or 0
        rep = top.get(3, REQUIRED)
        is_map = top.get(6) in (1, 2) or 2 in (top.get(10) or {})
        if not kids:
            if rep == REPEATED:
                raise _error(f'{pre}: a repeated primitive at top level (a list without its LIST group) is not supported')
            raise _error(f'{pre}: not a list column (a flat {_name(PHYSICAL, top.get(1))} column)')
        if rep == REPEATED:
            raise _error(f'{pre}: a repeated group at top level is not supported')
        if is_map:
            raise _error(f'{pre}: a map is not supported')
        mid = schema[at + 1]
        if kids != 1 or mid.get(3, REQUIRED) != REPEATED:
            raise _error(f'{pre}: a struct (a group of {kids} field(s) that is no LIST) is not supported')
        mkids = mid.get(5, 0) or 0
        if not mkids:
            raise _error(f'{pre}: a two-level legacy list (a repeated primitive inside the group) is not supported')
        if mkids != 1:
            raise _error(f'{pre}: a repeated group of {mkids} fields (a map or a two-level list of structs) is not supported')
        el = schema[at + 2]
        if el.get(5, 0):
            inner = schema[at + 3]
            form = 'a list of lists' if inner.get(3, REQUIRED) == REPEATED or (inner.get(5, 0) and el.get(5, 0) == 1) else 'a list of structs'
            raise _error(f'{pre}: {form} is not supported')
        if el.get(3, REQUIRED) == REPEATED:
            raise _error(f'{pre}: a repeated element inside the list group (a list of lists in legacy form) is not supported')
        if el.get(1) not in (1, 2):
            raise _error(f'{pre}: list element type {_name(PHYSICAL, el.get(1))} is not supported (INT32, INT64)')
        pathn = [top[4].decode(), mid[4].decode(), el[4].decode()]
        leaf = ListLeaf(column, tuple(pathn), el[1], _logical(el), rep == OPTIONAL, el.get(3, REQUIRED) == OPTIONAL)
        groups = []
        for rg in md.get(4, []):
            chunk = None
            for cc in rg[1]:
                if [p.decode() for p in cc[3][3]] == pathn:
                    chunk = _chunk(column, cc[3])
            groups.append((rg[3], chunk))
        return ListMetadata(path, md[3], leaf, groups)
    return _parse_footer(path, consume)


def _list_chunk(meta, g):
    n_rows, c = meta.row_groups[g]
    where = _where(meta, meta.leaf.name, g)
    if _check_chunk(c, where).physical != meta.leaf.physical:
        raise _error(f'{where}: the chunk holds {_name(PHYSICAL, c.physical)}, the schema declares {_name(PHYSICAL, meta.leaf.physical)}')
    return n_rows, c, where


def list_page_table(path, column):
    """Host only: ``(ListMetadata, {row group: [Page]})`` of the list column ``column`` of one file -- what :func:`read_lists`
    walks batch by batch, with every refusal the host can make (tests, tools)."""
    meta = read_list_metadata(path, column)
    out = {}
    with open(meta.path, 'rb') as f:
        for g in range(len(meta.row_groups)):
            _, c, where = _list_chunk(meta, g)
            f.seek(c.start)
            out[g] = walk_pages(f.read(c.length), c, meta.leaf, where)
    return meta, out


def _list_levels(dev, buf, n_bytes, table, infos, d_off, d_null, n_rows, value_base, work=None):
    """One ``otto_pqlist_levels`` call -> the per-page report ``int64 [pages, 3]`` (level bytes, values, rows)."""
    import ctypes as C
    import torch
    from . import _lib
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(PL_FIELDS))
    report = np.zeros((len(table), 3), dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    job = _lib.PqlistJob(_lib.ptr(buf, dev), int(n_bytes), vp(table), len(table), _lib.ptr(d_off, dev), _lib.ptr(d_null, dev), int(n_rows),
                         int(value_base), vp(report), None, 0, _lib.stream(dev))
    need = int(_lib.lib().otto_pqlist_workspace(C.byref(job)))
    if need < 0:
        _lib.check(need, 'otto_pqlist_workspace')
    if work is None:
        work = _lib.workspace(need, dev)
    elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
        raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
    job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
    _call('otto_pqlist_levels', dev, C.byref(job), infos=infos, reason_of='otto_pqlist_reason', stream=False)
    return report


def _list_plan(items, o):
    """The level job of one batch: ``items`` are ``(where, ListLeaf, rows of the row group, offset of the chunk's bytes, [Page])``
    per chunk, ``o`` the first free byte behind the chunks. Returns ``(pl, infos, bodies, streams, end)``: the OTTO_PL page
    records and their ``(where, page number)``, per record ``(body, body_len)``, the Snappy streams of the V1 pages
    ``(src, n, dst, dst_len, where, page number)`` -- their bodies are laid out from ``o`` on -- and the end of the last body."""
    from . import _lib
    at = o
    streams, pl, infos, bodies = [], [], [], []
    for where, leaf, rows, base, pages in items:
        flags = (PL_OUTER_OPTIONAL if leaf.outer_optional else 0) | (PL_ELEM_OPTIONAL if leaf.elem_optional else 0)
        n_data = sum(p.page_type != DICTIONARY_PAGE for p in pages)
        first = True
        for k, p in enumerate(pages):
            if p.page_type == DICTIONARY_PAGE:
                continue
            if p.page_type == DATA_PAGE_V2:
                body, blen = base + p.src_off, p.rep_len + p.def_len
            elif p.is_compressed:
                body, blen = at, p.uncomp_size
                streams.append((base + p.src_off, p.comp_size, body, blen, where, k))
                at += blen
            else:
                body, blen = base + p.src_off, p.comp_size
                if p.comp_size != p.uncomp_size:
                    raise _lib.OttoError(f'{where}, page {k}: decoded size differs from the page header')
            v2 = p.page_type == DATA_PAGE_V2
            pl.append((body, blen, p.page_type, p.rep_len if v2 else 0, p.def_len if v2 else 0, p.num_values,
                       flags | (PL_CHUNK_FIRST if first else 0), rows if first else 0, n_data if first else 0))
            infos.append((where, k))
            bodies.append((body, blen))
            first = False
        if rows and not n_data:
            raise _lib.OttoError(f'{where}: no data page in a row group of {rows} rows')
    return pl, infos, bodies, streams, at


def _decode_list_batch(dev, buf, o, items, d_off, d_null, n_rows, value_base, dt, work=None):
    """The chunks ``items`` of one batch, whose bytes lie in ``buf[:o]`` -> the values of the batch as a fresh tensor; the
    rows' offsets and null flags go to ``d_off`` / ``d_null``. ``buf`` has room behind ``o`` for the decoded V1 bodies."""
    import torch
    from . import _lib
    pl, pl_infos, bodies, streams, at = _list_plan(items, o)
    if at > buf.numel() or at >= 1 << 31:
        raise _lib.OttoError(f'{items[0][0]}: the pages decode to more bytes than the column chunks declare')
    if streams:
        a = lambda i: np.ascontiguousarray([s[i] for s in streams], dtype=np.int64)
        status = np.zeros(len(streams), dtype=np.int32)
        sw = _lib.workspace(int(_lib.lib().otto_parquet_snappy_workspace(len(streams))), dev)
        _lib.call('otto_parquet_snappy', dev, buf, at, a(0), a(1), a(2), a(3), len(streams), buf, at, status, sw, int(sw.numel()))
        bad = np.flatnonzero(status)
        if len(bad):
            raise _refusal([s[4:] for s in streams], int(bad[0]), int(status[bad[0]]), 'otto_parquet_reason')
    report = _list_levels(dev, buf, at, pl, pl_infos, d_off, d_null, n_rows, value_base, work)
    n_values = int(report[:, 1].sum()) if len(report) else 0
    values = torch.empty(n_values, dtype=dt, device=dev)
    table, infos, cols, slots, announced = [], [], [], {}, []
    data_pages = iter(zip(bodies, report.tolist()))           # in the order of _list_plan's records
    row = 0
    for where, leaf, rows, base, pages in items:
        def place(k, p):
            """a dictionary page as it lies in the file, a V2 data page too, a V1 data page as the level-free rest of its body"""
            if p.page_type == DICTIONARY_PAGE:
                announced.append(None)
                return _as_stored(p, base + p.src_off)
            (body, blen), (lev, nv, _) = next(data_pages)
            if nv == 0 and (p.comp_size if p.page_type == DATA_PAGE_V2 else blen) == lev:
                return None
            announced.append(nv)
            if p.page_type == DATA_PAGE_V2:
                return _as_stored(p, base + p.src_off, nv)
            return body + lev, blen - lev, blen - lev, DATA_PAGE, 0, 0, nv, 0
        row = _chunk_records(table, infos, where, pages, row, _column_slot(cols, slots, 0, leaf.physical, leaf.logical, values), place)
    if table:
        _decode(dev, buf, at, table, cols, infos,
                explain=lambda i, reason: reason if announced[i] is None else
                f'the value stream does not hold the {announced[i]} values its definition levels announce ({reason})')
    return values


def read_lists(paths, column, device, dtype=None, batch_bytes=256 << 20, out=None):
    """The list column ``column`` (SPEC-PQLIST: a three-level LIST of INT32 / INT64) of the files ``paths`` ->
    ``(off int64 [R + 1], values [V], null uint8 [R])``, rows in file and row-group order: the values of row r are
    ``values[off[r]:off[r + 1]]``; ``null[r]`` is 1 for a null list, whose span is empty like an empty list's. ``dtype``:
    the dtype of ``values`` instead of :func:`default_dtype` of the element, cast as in :func:`read_columns`.

    The batches, the two page-locked staging buffers and the hand-over between the copy stream and the caller's stream
    are those of :func:`read_columns`. Per batch: V1 bodies are decompressed whole (the levels lie inside), the level
    kernels leave offsets, null flags and a per-page report (level bytes, values), and the values run through
    ``otto_parquet_decode`` as level-free pages. A refused file raises ``OttoError`` (file, column, row group, page, reason)
    and writes nothing the caller can see: ``out`` (three tensors to fill instead of fresh ones) is written only after
    every batch came back clean."""
    import torch
    from . import _lib
    dev = _lib.rocm_device(device, 'parquet.read_lists')
    _lib.lib()
    metas = [read_list_metadata(p, column) for p in _paths(paths)]
    dt = dtype or (default_dtype(metas[0].leaf) if metas else torch.int64)
    if dt not in _sizes():
        raise ValueError(f'dtype: {dt} is not an integer dtype of 1, 2, 4 or 8 bytes')
    groups, extents, row = [], [], 0                          # (file, chunk, where, rows, first row); (stored bytes, with bodies)
    for fi, m in enumerate(metas):
        for g in range(len(m.row_groups)):
            n, c, where = _list_chunk(m, g)
            comp = (c.length + 15) & ~15
            groups.append((fi, c, where, n, row))
            extents.append((comp, comp + (c.uncompressed if c.codec == 1 else 0)))
            row += n
    n_rows = row
    batches = _plan_batches(extents, batch_bytes)
    stage, room = _largest_batch(extents, batches)
    if room >= 1 << 31:
        raise _lib.OttoError(f'a row group of {room} stored plus decoded bytes does not fit one call (2^31)')
    with torch.cuda.device(dev):
        off = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        null = torch.zeros(n_rows, dtype=torch.uint8, device=dev)
        parts, n_values = [], 0

        def fill(batch, view, file):
            items, o = [], 0
            for fi, c, where, n, _ in (groups[i] for i in batch):
                leaf = metas[fi].leaf
                items.append((where, leaf, n, o, walk_pages(_read_chunk(file(fi), view, o, c, where), c, leaf, where)))
                o += (c.length + 15) & ~15
            return o, (items, groups[batch[0]][4], sum(groups[i][3] for i in batch))

        def decode(d_bytes, o, payload):
            nonlocal n_values
            items, row0, rows = payload
            parts.append(_decode_list_batch(dev, d_bytes, o, items, off[row0:], null[row0:], rows, n_values, dt))
            n_values += int(parts[-1].numel())
        _stage_batches(dev, [m.path for m in metas], batches, stage, room, fill, decode)
        values = parts[0] if len(parts) == 1 else torch.cat(parts) if parts else torch.empty(0, dtype=dt, device=dev)
        if out is not None:
            return _fill_out(out, (off, values, null), '(off, values, null)')
    return off, values, null


def _snappy_host(data, n):
    """A raw Snappy stream -> its ``n`` bytes, on the host (the small dictionary page of a string column)."""
    data = bytes(data)
    t = _Thrift(data)
    if t.varint() != n or t.i > 5:
        raise ValueError('snappy: preamble disagrees with the declared uncompressed size')
    i, out = t.i, bytearray()
    cut = ValueError('snappy: stream cut short inside an element')
    while i < len(data):
        tag = data[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if i + nb > len(data):
                    raise cut
                ln = int.from_bytes(data[i:i + nb], 'little')
                i += nb
            ln += 1
            if i + ln > len(data):
                raise cut
            out += data[i:i + ln]
            i += ln
        else:
            nb = 1 if kind == 1 else 2 if kind == 2 else 4
            if i + nb > len(data):
                raise cut
            if kind == 1:
                ln, offset = 4 + ((tag >> 2) & 7), (tag >> 5) << 8 | data[i]
                i += 1
            else:
                ln, offset = 1 + (tag >> 2), int.from_bytes(data[i:i + nb], 'little')
                i += nb
            if offset == 0 or offset > len(out):
                raise ValueError('snappy: copy offset is 0 or reaches before the output')
            for _ in range(ln):
                out.append(out[-offset])
        if len(out) > n:
            raise ValueError('snappy: output runs past the declared uncompressed size')
    if len(out) != n:
        raise ValueError('snappy: stream ends before the declared uncompressed size')
    return bytes(out)


def string_dictionary(buf, page, where, k):
    """The strings (bytes) of the PLAIN BYTE_ARRAY dictionary page ``page`` of the chunk bytes ``buf``, decoded on the host."""
    if page.uncomp_size > MAX_STRING_DICTIONARY:
        raise _error(f'{where}, page {k}: a string dictionary page of {page.uncomp_size} bytes is not supported ({MAX_STRING_DICTIONARY} at most)')
    raw = bytes(buf[page.src_off:page.src_off + page.comp_size])
    try:
        if page.is_compressed:
            raw = _snappy_host(raw, page.uncomp_size)
        elif page.comp_size != page.uncomp_size:
            raise ValueError('decoded size differs from the page header')
        out, i = [], 0
        for _ in range(page.num_values):
            if i + 4 > len(raw):
                raise ValueError('the dictionary ends inside a length')
            n = struct.unpack_from('<I', raw, i)[0]
            if i + 4 + n > len(raw):
                raise ValueError('the dictionary ends inside a string')
            out.append(raw[i + 4:i + 4 + n])
            i += 4 + n
    except (ValueError, IndexError) as e:
        raise _error(f'{where}, page {k}: malformed string dictionary ({e})') from None
    return out


def string_code_table(path, column, mapping):
    """Host only: the plan of :func:`read_string_codes` for one file, with every refusal the host can make ->
    ``(num_rows, [(where, chunk, [Page], {page number: int32 codes of that dictionary page})] per row group)``."""
    meta = read_metadata(path)
    leaf = _flat_leaf(meta, column)
    if leaf.physical != BYTE_ARRAY:
        raise _error(f'{meta.path}: column {column!r}: physical type {_name(PHYSICAL, leaf.physical)} is no string column (BYTE_ARRAY)')
    codes = {(k.encode() if isinstance(k, str) else bytes(k)): int(v) for k, v in mapping.items()}
    out = []
    with open(meta.path, 'rb') as f:
        for g in range(len(meta.row_groups)):
            c, = check_row_group(meta, g, [column])
            where = _where(meta, column, g)
            f.seek(c.start)
            buf = f.read(c.length)
            pages = walk_pages(buf, c, leaf, where)
            dicts = {}
            for k, p in enumerate(pages):
                if p.page_type == DICTIONARY_PAGE:
                    strings = string_dictionary(buf, p, where, k)
                    for s in strings:
                        if s not in codes:
                            raise _error(f'{where}, page {k}: dictionary string {s.decode("utf-8", "replace")!r} is not in the mapping '
                                         f'({sorted(x.decode("utf-8", "replace") for x in codes)})')
                    dicts[k] = np.array([codes[s] for s in strings], dtype=np.int32)
                elif p.encoding != 8:
                    raise _error(f'{where}, page {k}: a {"PLAIN" if p.encoding == 0 else "DELTA_BINARY_PACKED"} BYTE_ARRAY data page is not '
                                 'supported (dictionary-coded strings only)')
                elif not dicts:
                    raise _error(f'{where}, page {k}: dictionary-coded page without a dictionary page')
            out.append((where, c, buf, pages, dicts))
    return meta.num_rows, out


def read_string_codes(paths, column, mapping, device, dtype=None):
    """The dictionary-coded string column ``column`` of the files ``paths`` -> one device tensor of ``mapping[string]`` per row
    (``dtype``: ``torch.uint8`` unless given). The host reads every chunk's dictionary page (PLAIN BYTE_ARRAY, at most 64 KiB),
    maps its strings through ``mapping`` and hands the device an INT32 dictionary in its place; the index pages run through
    the dictionary gather of ``otto_parquet_decode`` as they lie in the file. Refused by name: a dictionary string that is
    not in ``mapping``, a PLAIN or DELTA data page, a larger dictionary page. The index pages of all files go across in one
    piece (a string column of three values is a few bytes per thousand rows)."""
    import torch
    from . import _lib
    dev = _lib.rocm_device(device, 'parquet.read_string_codes')
    _lib.lib()
    dt = dtype or torch.uint8
    sizes = _sizes()
    if dt not in sizes:
        raise ValueError(f'dtype: {dt} is not one of {sorted(map(str, sizes))}')
    lo, hi = (0, 1 << 8 * sizes[dt]) if dt == torch.uint8 else (-(1 << 8 * sizes[dt] - 1), 1 << 8 * sizes[dt] - 1)
    for s, v in mapping.items():
        if not lo <= int(v) < min(hi, 1 << 31):
            raise ValueError(f'mapping[{s!r}]: {v} does not fit {dt}')
    plans = [string_code_table(p, column, mapping) for p in _paths(paths)]
    n_rows = sum(p[0] for p in plans)
    pieces, table, infos, cols, o, row = [], [], [], [], 0, 0

    def put(b):
        nonlocal o
        at = o
        pieces.append(b)
        pad = -len(b) % 16
        if pad:
            pieces.append(bytes(pad))
        o += len(b) + pad
        return at
    with torch.cuda.device(dev):
        result = torch.empty(n_rows, dtype=dt, device=dev)
        slot = _column_slot(cols, {}, 0, 1, None, result)      # the device sees an INT32 dictionary
        for _, groups in plans:
            for where, c, buf, pages, dicts in groups:
                def place(k, p):
                    """the host-built INT32 dictionary in place of the string one, an index page as it lies in the file"""
                    if p.page_type == DICTIONARY_PAGE:
                        n = len(dicts[k])
                        return put(dicts[k].tobytes()), 4 * n, 4 * n, DICTIONARY_PAGE, 0, 0, n, 0
                    return _as_stored(p, put(bytes(buf[p.src_off:p.src_off + p.comp_size])))
                row = _chunk_records(table, infos, where, pages, row, slot, place)
        if o >= 1 << 31:
            raise _lib.OttoError(f'column {column!r}: {o} bytes of index pages do not fit one call (2^31)')
        if table:
            d_bytes = torch.from_numpy(np.frombuffer(b''.join(pieces) or bytes(16), dtype=np.uint8).copy()).to(dev)
            _decode(dev, d_bytes, o, table, cols, infos)
    return result
