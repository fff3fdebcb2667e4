"""Device-side Parquet decode: the split files ``DATA/splits/*.parquet`` and the
part files of the reference's chunk writers -> device columns, unpacked by HIP kernels (``include/otto_parquet.h``,
SPEC-PARQUET): a Snappy decompressor, an RLE / bit-packed hybrid decoder, a dictionary gather and a DELTA_BINARY_PACKED
decoder. With ``floats=True`` FLOAT / DOUBLE columns (the ``wgt`` column of the covisitation part files) come back as bit copies.

Reference code replaced: the pyarrow / pandas host decode in front of every consumer of the split files
(``src/ranker/aid_feature_engineering.py:21-36``). The host side here is pure Python + NumPy and imports no pyarrow: a
Thrift compact-protocol reader for the footer and the page headers (:func:`read_metadata`, :func:`walk_pages`), and
:func:`read_columns`, which reads the byte ranges of the requested column chunks into page-locked staging buffers and
sends them across as they lie in the file.
"""
import os
import struct
from collections import namedtuple

import numpy as np

TILE = 1024                  # OTTO_PQ_TILE
FIELDS = ('src_off', 'comp_size', 'uncomp_size', 'page_type', 'encoding', 'def_len', 'rep_len', 'num_values', 'is_compressed',
          'out_row', 'col_slot', 'dict_slot')                                            # OTTO_PQ_* of a page record
F = {k: i for i, k in enumerate(FIELDS)}
PHYSICAL = ('BOOLEAN', 'INT32', 'INT64', 'INT96', 'FLOAT', 'DOUBLE', 'BYTE_ARRAY', 'FIXED_LEN_BYTE_ARRAY')
CODECS = ('UNCOMPRESSED', 'SNAPPY', 'GZIP', 'LZO', 'BROTLI', 'LZ4', 'ZSTD', 'LZ4_RAW')
ENCODINGS = {0: 'PLAIN', 2: 'PLAIN_DICTIONARY', 3: 'RLE', 4: 'BIT_PACKED', 5: 'DELTA_BINARY_PACKED', 6: 'DELTA_LENGTH_BYTE_ARRAY',
             7: 'DELTA_BYTE_ARRAY', 8: 'RLE_DICTIONARY', 9: 'BYTE_STREAM_SPLIT'}
DATA_PAGE, INDEX_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 1, 2, 3
REQUIRED, OPTIONAL, REPEATED = 0, 1, 2
TICKS_PER_SECOND = {'MILLIS': 10 ** 3, 'MICROS': 10 ** 6, 'NANOS': 10 ** 9}

Leaf = namedtuple('Leaf', 'name physical repetition logical nested')
# logical: None | ('INT', bits, signed) | ('TIMESTAMP', unit) | ('OTHER', name);  nested: a group, not a leaf
Chunk = namedtuple('Chunk', 'name physical codec num_values start length data_page_offset dictionary_page_offset uncompressed encodings')
RowGroup = namedtuple('RowGroup', 'num_rows chunks')              # chunks: {top-level name: Chunk}
Metadata = namedtuple('Metadata', 'path num_rows leaves row_groups')
Page = namedtuple('Page', 'header_off ' + ' '.join(FIELDS[:9]))   # offsets relative to the chunk's first byte


def _error(msg):
    from . import _lib
    return _lib.OttoError(msg)


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


def read_metadata(path):
    """The footer of a Parquet file -> :class:`Metadata`: the top-level schema leaves (nested groups marked), the row groups
    and, per top-level primitive column, the chunk's byte range, codec, ``num_values`` and sizes. Raises ``OttoError`` on a
    wrong magic, an encrypted or truncated footer."""
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
    try:
        md = _Thrift(foot).struct()
        schema = md[2]
        leaves, i = [], 1

        def skip(j):                          # the element at j and its subtree -> the index behind it
            kids = schema[j].get(5, 0) or 0
            j += 1
            for _ in range(kids):
                j = skip(j)
            return j
        for _ in range(schema[0].get(5, 0) or 0):
            el = schema[i]
            nested = bool(el.get(5, 0))
            leaves.append(Leaf(el[4].decode(), el.get(1), el.get(3, REQUIRED), _logical(el), nested))
            i = skip(i)
        groups = []
        for rg in md.get(4, []):
            chunks = {}
            for cc in rg[1]:
                cm = cc[3]
                pathn = [p.decode() for p in cm[3]]
                if len(pathn) != 1:
                    continue
                dpo, dico = cm[9], cm.get(11)
                start = dico if dico is not None and 0 < dico < dpo else dpo
                chunks[pathn[0]] = Chunk(pathn[0], cm[1], cm[4], cm[5], start, cm[7], dpo, dico, cm[6], tuple(cm[2]))
            groups.append(RowGroup(rg[3], chunks))
        return Metadata(path, md[3], leaves, groups)
    except (ValueError, KeyError, IndexError) as e:
        raise _error(f'{path}: malformed footer ({e})') from None


def _name(table, k):
    return table[k] if isinstance(table, tuple) and 0 <= k < len(table) else table.get(k, f'#{k}') if isinstance(table, dict) else f'#{k}'


FLOAT, DOUBLE = 4, 5           # PHYSICAL


def check_column(meta, name, floats=False):
    """The leaf ``name`` of the file, or the ``OttoError`` SPEC-PARQUET names for a column that cannot be read.
    ``floats``: FLOAT / DOUBLE columns are accepted too."""
    leaf = next((l for l in meta.leaves if l.name == name), None)
    if leaf is None:
        raise _error(f'{meta.path}: column {name!r}: not in the file (top-level columns: {[l.name for l in meta.leaves]})')
    if leaf.nested or leaf.repetition == REPEATED:
        raise _error(f'{meta.path}: column {name!r}: a repeated or nested column is not supported')
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
    of them, from ``chunk.start``); only header bytes are touched. ``where``: the text that opens an error message."""
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
            if leaf.repetition == OPTIONAL and d.get(3, 3) != 3:
                raise _error(f'{where}, page {k}: definition level encoding {_name(ENCODINGS, d.get(3))} is not supported')
            pages.append(Page(pos, body, comp, uncomp, ptype, enc, -1 if leaf.repetition == OPTIONAL else 0, 0, d.get(1, 0),
                              int(snappy)))
            seen += d.get(1, 0)
        elif ptype == DATA_PAGE_V2:
            d = h.get(8, {})
            enc = _data_encoding(d.get(4, 0), leaf, where, k)
            if d.get(2, 0) != 0:
                raise _error(f'{where}, page {k}: {d.get(2)} null(s): nulls are not supported')
            pages.append(Page(pos, body, comp, uncomp, ptype, enc, d.get(5, 0), d.get(6, 0), d.get(1, 0),
                              int(snappy and d.get(7, True))))
            seen += d.get(1, 0)
        elif ptype != INDEX_PAGE:
            raise _error(f'{where}, page {k}: page type {ptype} is not supported')
        pos = body + comp
        k += 1
    if seen != chunk.num_values:
        raise _error(f'{where}: the pages hold {seen} values, the column chunk declares {chunk.num_values}')
    return pages


def _where(meta, name, g):
    return f'{meta.path}: column {name!r}, row group {g}'


def check_row_group(meta, g, columns):
    """The chunks of the requested columns of row group ``g``, checked: codec, agreement on ``num_rows``."""
    rg = meta.row_groups[g]
    out = []
    for name in columns:
        c = rg.chunks.get(name)
        if c is None:
            raise _error(f'{_where(meta, name, g)}: no column chunk')
        if c.codec not in (0, 1):
            raise _error(f'{_where(meta, name, g)}: codec {_name(CODECS, c.codec)} is not supported (UNCOMPRESSED, SNAPPY)')
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


def _decode(dev, d_bytes, n_bytes, table, cols, infos, phases=3, work=None):
    """One ``otto_parquet_decode`` call; a violation raises the ``OttoError`` that names file, column, row group and page."""
    import ctypes as C
    from . import _lib
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(FIELDS))
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    need = int(_lib.lib().otto_parquet_workspace(table.ctypes.data_as(C.c_void_p), len(table)))
    if need < 0:
        _lib.check(need, 'otto_parquet_workspace')
    if work is None:
        work = _lib.workspace(need, dev)
    err = np.full(2, -1, dtype=np.int64)
    try:
        _lib.call('otto_parquet_decode', dev, d_bytes, int(n_bytes), table, len(table), cols, len(cols), int(phases), work,
                  int(work.numel()), err)
    except _lib.OttoError:
        if err[0] < 0:
            raise
        where, k = infos[int(err[0])]
        reason = _lib.lib().otto_parquet_reason(int(err[1])).decode()
        raise _lib.OttoError(f'{where}, page {k}: {reason}') from None
    return work


def _read_full(f, view):
    got = 0
    while got < len(view):
        k = f.readinto(view[got:])
        if not k:
            break
        got += k
    return got


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
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.OttoError('parquet.read_columns needs a ROCm device (no CPU fallback)')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    _lib.lib()
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
    columns = list(columns)
    dtypes = dict(dtypes or {})
    sizes = {torch.uint8: 1, torch.int8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}
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
    sizes = {**sizes, torch.float32: 4, torch.float64: 8}
    # the batches: runs of whole row groups, over all files
    groups = []                                               # (file, row group, chunks, first row, compressed bytes, both)
    row = 0
    for fi, m in enumerate(metas):
        for g in range(len(m.row_groups)):
            chunks = check_row_group(m, g, columns)
            comp = sum((c.length + 15) & ~15 for c in chunks)
            groups.append((fi, g, chunks, row, comp, comp + sum(c.uncompressed for c in chunks)))
            row += m.row_groups[g].num_rows
    n_rows = row
    batches, cur, cur_bytes = [], [], 0
    for gr in groups:
        if cur and cur_bytes + gr[5] > batch_bytes:
            batches.append(cur)
            cur, cur_bytes = [], 0
        cur.append(gr)
        cur_bytes += gr[5]
    if cur:
        batches.append(cur)
    stage = max([sum(gr[4] for gr in b) for b in batches], default=0)
    if stage >= 1 << 31:
        raise _lib.OttoError(f'a row group of {stage} compressed bytes does not fit one call (2^31)')
    with torch.cuda.device(dev):
        result = [torch.empty(n_rows, dtype=dt, device=dev) for dt in col_dt]
        if batches:
            host = [torch.empty(max(stage, 16), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            devb = [torch.empty(max(stage, 16), dtype=torch.uint8, device=dev) for _ in range(2)]
            copy_stream = torch.cuda.Stream(device=dev)
            compute = torch.cuda.current_stream(dev)
            # the device sets come from the caller's stream's allocator: a block it freed may still be read by work queued there
            copy_stream.wait_stream(compute)
            sent = [torch.cuda.Event(), torch.cuda.Event()]      # H2D of the set finished
            used = [torch.cuda.Event(), torch.cuda.Event()]      # the decode no longer reads the set
        files = {}

        def prepared():
            """(staging set, bytes, page table, column records, page infos) per batch, read and on its way to the device"""
            for i, batch in enumerate(batches):
                b = i & 1
                if i >= 2:
                    used[b].synchronize()                        # the set is free again, host and device side
                view = host[b].numpy()
                table, infos, o = [], [], 0
                cols, slots = [], {}                             # one record per (column, physical size, extension) of the batch
                for fi, g, chunks, row0, _, _ in batch:
                    m = metas[fi]
                    if fi not in files:
                        files[fi] = open(m.path, 'rb', buffering=0)
                    f = files[fi]
                    for j, c in enumerate(chunks):
                        where = _where(m, c.name, g)
                        f.seek(c.start)
                        if _read_full(f, memoryview(view)[o:o + c.length]) != c.length:
                            raise _lib.OttoError(f'{where}: the column chunk runs past the end of the file')
                        leaf = leaves[fi][j]
                        key = (j, 4 if leaf.physical in (1, FLOAT) else 8, int(leaf.physical == 1 and leaf.logical == ('INT', 32, False)))
                        if key not in slots:
                            slots[key] = len(cols)
                            cols.append((result[j].data_ptr(), sizes[col_dt[j]], n_rows, key[1], key[2]))
                        dict_slot, r = -1, row0
                        for k, p in enumerate(walk_pages(view[o:o + c.length], c, leaf, where)):
                            if p.page_type == DICTIONARY_PAGE:
                                dict_slot = len(table)
                            elif p.encoding == 8 and dict_slot < 0:
                                raise _lib.OttoError(f'{where}, page {k}: dictionary-coded page without a dictionary page')
                            table.append((o + p.src_off, p.comp_size, p.uncomp_size, p.page_type, p.encoding, p.def_len, p.rep_len,
                                          p.num_values, p.is_compressed, r, slots[key],
                                          dict_slot if p.page_type != DICTIONARY_PAGE and p.encoding == 8 else -1))
                            infos.append((where, k))
                            if p.page_type != DICTIONARY_PAGE:
                                r += p.num_values
                        o += (c.length + 15) & ~15
                with torch.cuda.stream(copy_stream):
                    devb[b][:o].copy_(host[b][:o], non_blocking=True)
                    sent[b].record(copy_stream)
                yield b, o, table, cols, infos

        try:
            it = prepared()
            cur = next(it, None)
            while cur is not None:
                nxt = next(it, None)                             # read and send batch i + 1 before batch i decodes
                b, n, table, cols, infos = cur
                compute.wait_event(sent[b])
                if table:
                    _decode(dev, devb[b], n, table, cols, infos)
                used[b].record(compute)
                cur = nxt
        finally:
            for f in files.values():
                f.close()
            torch.cuda.synchronize(dev)
        if out is not None:
            out = tuple(out)
            if len(out) != len(result) or any(o.shape != r.shape or o.dtype != r.dtype or o.device != r.device for o, r in zip(out, result)):
                raise ValueError('out: expected one tensor per column with the shape, dtype and device of the result')
            for o, r in zip(out, result):
                o.copy_(r)
            return out
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
