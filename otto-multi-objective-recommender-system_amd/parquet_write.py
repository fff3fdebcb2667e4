"""Device-side Parquet encode (SPEC-PQWRITE, ``include/otto_pqwrite.h``): named device columns -> the
bytes of Parquet files whose data pages are sized and bit-packed by HIP kernels (``csrc/otto_pqwrite.hip``). Only the encoded
bytes cross PCIe; the host adds the Thrift-compact page headers and the footer. ``pyarrow.parquet.read_table`` and
``pandas.read_parquet`` read the files with the dtypes of the input columns. With ``compression='snappy'`` the page bodies
of the chosen columns are Snappy streams made on the device as well (SPEC-SNAPPY, ``include/otto_snappy.h``, section 2h).

Reference code replaced: the pyarrow encode behind ``DataFrame.to_parquet`` of ``src/covisitation/covisitation.py`` (the
matrix part files) and of ``src/utilities/split_dataset_writer_parquet.py`` (the 100,000-session chunks).

The host side is pure Python + NumPy and imports no pyarrow: a Thrift compact-protocol writer (the counterpart of
``parquet._Thrift``), the page table (files and row groups exist only here) and the assembly of the images.
"""
import ctypes as C
import os
import re
import struct

import numpy as np

PLAIN, DELTA = 0, 5                          # OTTO_PQW_PLAIN, OTTO_PQW_DELTA: the Parquet Encoding codes
RLE = 3
SIGNED, UNSIGNED, FLOAT = 0, 1, 2            # OTTO_PQW_SIGNED ...
PAGE_ROWS, ROW_GROUP_ROWS = 1 << 16, 1 << 20
MAX_PAGE_VALUES = 1 << 26                    # OTTO_PQW_MAX_PAGE_VALUES
MAGIC = b'PAR1'
CREATED_BY = b'otto_amd SPEC-PQWRITE'
PAGE_DTYPE = np.dtype([('first_row', '<i8'), ('n_values', '<i4'), ('column', '<i4')])        # otto_pqw_page
INT32, INT64, FLOAT32, DOUBLE = 1, 2, 4, 5   # parquet.PHYSICAL
UNCOMPRESSED, SNAPPY = 0, 1                  # the Parquet CompressionCodec codes
ENCODING_NAMES = {'plain': PLAIN, 'delta': DELTA, 'PLAIN': PLAIN, 'DELTA_BINARY_PACKED': DELTA, PLAIN: PLAIN, DELTA: DELTA}

# element type name -> (bytes, kind, physical type, converted_type or None)
ELEMENTS = {
    'int8': (1, SIGNED, INT32, 15), 'int16': (2, SIGNED, INT32, 16), 'int32': (4, SIGNED, INT32, None), 'int64': (8, SIGNED, INT64, None),
    'uint8': (1, UNSIGNED, INT32, 11), 'uint16': (2, UNSIGNED, INT32, 12), 'uint32': (4, UNSIGNED, INT32, 13),
    'uint64': (8, UNSIGNED, INT64, 14), 'float32': (4, FLOAT, FLOAT32, None), 'float64': (8, FLOAT, DOUBLE, None),
}


# ---------------------------------------------------------------------------------------------------------------------
# Thrift compact protocol, writing. A struct is a list of (field id, wire type, value) in ascending field id; a list value
# is (element wire type, [values]); a bool field is written with type T_BOOL and a Python bool.
# ---------------------------------------------------------------------------------------------------------------------
T_BOOL, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_STRUCT = 1, 3, 4, 5, 6, 7, 8, 9, 12


class ThriftWriter:
    def __init__(self):
        self.b = bytearray()

    def varint(self, v):
        if v < 0:
            raise ValueError('a varint is unsigned')
        while v >= 0x80:
            self.b.append((v & 0x7F) | 0x80)
            v >>= 7
        self.b.append(v)

    def zigzag(self, v, bits=64):
        if not -(1 << (bits - 1)) <= v < 1 << (bits - 1):
            raise ValueError(f'{v} does not fit {bits} bits')
        self.varint((v << 1) ^ (v >> (bits - 1)))

    def value(self, t, v):
        if t in (1, 2):                       # a bool outside a struct field: one byte
            self.b.append(1 if v else 2)
        elif t == T_BYTE:
            self.b.append(v & 0xFF)
        elif t in (T_I16, T_I32, T_I64):
            self.zigzag(int(v), {T_I16: 16, T_I32: 32, T_I64: 64}[t])
        elif t == T_DOUBLE:
            self.b += struct.pack('<d', v)
        elif t == T_BINARY:
            v = v.encode() if isinstance(v, str) else bytes(v)
            self.varint(len(v))
            self.b += v
        elif t == T_LIST:
            et, items = v
            if len(items) < 15:
                self.b.append(len(items) << 4 | et)
            else:
                self.b.append(0xF0 | et)
                self.varint(len(items))
            for x in items:
                self.value(et, x)
        elif t == T_STRUCT:
            self.struct(v)
        else:
            raise ValueError(f'Thrift wire type {t}')

    def struct(self, fields):
        last = 0
        for fid, t, v in fields:
            if fid <= last:
                raise ValueError('field ids must ascend')
            wire = (1 if v else 2) if t == T_BOOL else t
            if fid - last <= 15:
                self.b.append((fid - last) << 4 | wire)
            else:
                self.b.append(wire)
                self.zigzag(fid, 16)
            if t != T_BOOL:
                self.value(t, v)
            last = fid
        self.b.append(0)
        return self


def thrift_bytes(fields):
    return bytes(ThriftWriter().struct(fields).b)


def page_header(n_values, encoding, body_bytes, compressed_bytes=None):
    """The PageHeader of a V1 data page of a REQUIRED column; ``compressed_bytes``: the bytes present, where a codec made them."""
    return thrift_bytes([(1, T_I32, 0), (2, T_I32, body_bytes), (3, T_I32, body_bytes if compressed_bytes is None else compressed_bytes),
                         (5, T_STRUCT, [(1, T_I32, n_values), (2, T_I32, encoding), (3, T_I32, RLE), (4, T_I32, RLE)])])


# ---------------------------------------------------------------------------------------------------------------------
# the page table and the images
# ---------------------------------------------------------------------------------------------------------------------
def element(dtype):
    """``ELEMENTS`` entry of a torch or NumPy dtype."""
    name = str(dtype).split('.')[-1]
    if name not in ELEMENTS:
        raise ValueError(f'element type {dtype} is not one of {sorted(ELEMENTS)}')
    return ELEMENTS[name]


def _check_rows(page_rows, row_group_rows):
    if not isinstance(page_rows, int) or page_rows < 128 or page_rows % 128 or page_rows > MAX_PAGE_VALUES:
        raise ValueError(f'page_rows must be a multiple of 128 in [128, {MAX_PAGE_VALUES}] (got {page_rows!r})')
    if not isinstance(row_group_rows, int) or row_group_rows < page_rows or row_group_rows % page_rows:
        raise ValueError(f'row_group_rows must be a multiple of page_rows (got {row_group_rows!r})')


class Layout:
    """Files, row groups and pages of ``n_columns`` columns cut at ``cuts``: ``pages`` is the table the device sees
    (``PAGE_DTYPE``, in file order), ``files[i]`` a list of row groups ``(rows, [[page index, ...] per column])``."""

    def __init__(self, n_columns, cuts, page_rows, row_group_rows):
        _check_rows(page_rows, row_group_rows)
        cuts = [int(c) for c in cuts]
        if len(cuts) < 2 or cuts[0] < 0 or any(b < a for a, b in zip(cuts, cuts[1:])):
            raise ValueError('cuts: at least two non-negative row numbers that never descend')
        pages, self.files = [], []
        for r0, r1 in zip(cuts, cuts[1:]):
            groups = []
            for g0 in range(r0, max(r1, r0 + 1), row_group_rows):
                g1 = min(g0 + row_group_rows, r1)
                per_column = []
                for j in range(n_columns):
                    idx = []
                    for p0 in range(g0, max(g1, g0 + 1), page_rows):
                        idx.append(len(pages))
                        pages.append((p0, min(p0 + page_rows, g1) - p0, j))
                    per_column.append(idx)
                groups.append((g1 - g0, per_column))
            self.files.append(groups)
        self.pages = np.array(pages, dtype=PAGE_DTYPE)
        self.cuts = cuts

    def place(self, names, elements, encodings, page_bytes, codecs=None, stored_bytes=None):
        """Given the body size of every page: the headers and footers, where each body goes. Returns ``(total, page_dst,
        spans, fills)``: the bytes of all images back to back, the offset of every page body, the ``(first, end)`` of each
        image, and the ``(offset, bytes)`` pieces the host writes (everything but the bodies). ``codecs``: the
        CompressionCodec of each column (default UNCOMPRESSED); ``stored_bytes``: the bytes of every page as it is stored,
        which for a page of a compressed column is its compressed size (default ``page_bytes``)."""
        codecs = [UNCOMPRESSED] * len(names) if codecs is None else codecs
        stored_bytes = page_bytes if stored_bytes is None else stored_bytes
        page_dst = np.zeros(len(self.pages), dtype=np.int64)
        fills, spans, at = [], [], 0
        for fi, groups in enumerate(self.files):
            start = at
            fills.append((at, MAGIC))
            at += 4
            rgs = []
            for rows, per_column in groups:
                chunks, rg_plain = [], 0
                for j, idx in enumerate(per_column):
                    first, plain = at, 0                     # plain: the chunk's bytes before the codec, page headers included
                    for p in idx:
                        stored = int(stored_bytes[p]) if codecs[j] else int(page_bytes[p])
                        h = page_header(int(self.pages['n_values'][p]), encodings[j], int(page_bytes[p]), stored)
                        fills.append((at, h))
                        page_dst[p] = at + len(h)
                        at += len(h) + stored
                        plain += len(h) + int(page_bytes[p])
                    meta = [(1, T_I32, elements[j][2]), (2, T_LIST, (T_I32, [encodings[j], RLE])), (3, T_LIST, (T_BINARY, [names[j]])),
                            (4, T_I32, codecs[j]), (5, T_I64, rows), (6, T_I64, plain), (7, T_I64, at - first), (9, T_I64, first - start)]
                    chunks.append([(2, T_I64, first - start), (3, T_STRUCT, meta)])
                    rg_plain += plain
                rgs.append([(1, T_LIST, (T_STRUCT, chunks)), (2, T_I64, rg_plain), (3, T_I64, rows)])
            schema = [[(4, T_BINARY, 'schema'), (5, T_I32, len(names))]]
            for name, el in zip(names, elements):
                leaf = [(1, T_I32, el[2]), (3, T_I32, 0), (4, T_BINARY, name)]
                if el[3] is not None:
                    leaf.append((6, T_I32, el[3]))
                schema.append(leaf)
            foot = thrift_bytes([(1, T_I32, 1), (2, T_LIST, (T_STRUCT, schema)), (3, T_I64, self.cuts[fi + 1] - self.cuts[fi]),
                                 (4, T_LIST, (T_STRUCT, rgs)), (6, T_BINARY, CREATED_BY)])
            fills.append((at, foot + struct.pack('<I', len(foot)) + MAGIC))
            at += len(foot) + 8
            spans.append((start, at))
        return at, page_dst, spans, fills


def _normalise(columns, encodings):
    names = list(columns)
    if not names:
        raise ValueError('columns: at least one named column')
    encodings = encodings or {}
    unknown = set(encodings) - set(names)
    if unknown:
        raise ValueError(f'encodings names columns that are not there: {sorted(unknown)}')
    enc = []
    for n in names:
        e = encodings.get(n, PLAIN)
        if e not in ENCODING_NAMES:
            raise ValueError(f'encodings[{n!r}]: {e!r} is not "plain" or "delta"')
        enc.append(ENCODING_NAMES[e])
    return names, enc


def _codecs(names, compression):
    """``compression``: None, 'snappy' or ``{column: None | 'snappy'}`` -> the CompressionCodec of each column."""
    if compression is None or isinstance(compression, str):
        compression = {n: compression for n in names}
    elif not isinstance(compression, dict):
        raise ValueError(f"compression: None, 'snappy' or a dict of them by column (got {compression!r})")
    unknown = set(compression) - set(names)
    if unknown:
        raise ValueError(f'compression names columns that are not there: {sorted(unknown)}')
    codecs = []
    for n in names:
        c = compression.get(n)
        if c not in (None, 'snappy'):
            raise ValueError(f"compression[{n!r}]: {c!r} is not None or 'snappy'")
        codecs.append(SNAPPY if c else UNCOMPRESSED)
    return codecs


def _check_columns(names, cols, elements, enc, cuts):
    n = len(cols[0])
    for name, c, el, e in zip(names, cols, elements, enc):
        if len(c) != n:
            raise ValueError(f'column {name!r}: {len(c)} rows, {names[0]!r} has {n}')
        if e == DELTA and el[1] == FLOAT:
            raise ValueError(f'column {name!r}: DELTA_BINARY_PACKED is for integer columns')
    if cuts[-1] > n:
        raise ValueError(f'cuts end at row {cuts[-1]}, the columns have {n}')


def encode_tables_host(columns, cuts, encodings=None, page_rows=PAGE_ROWS, row_group_rows=ROW_GROUP_ROWS, body=None, compression=None,
                       compress=None):
    """:func:`encode_tables` with host functions in the device's place (tests): ``columns`` are NumPy arrays,
    ``body(array, encoding)`` returns the bytes of one page body and ``compress(bytes)`` the Snappy stream of one (default:
    ``snappy.stored_stream``, literal elements alone). Everything else is the code the product runs."""
    names, enc = _normalise(columns, encodings)
    codecs = _codecs(names, compression)
    cols = [np.ascontiguousarray(columns[n]) for n in names]
    elements = [element(c.dtype) for c in cols]
    lay = Layout(len(names), cuts, page_rows, row_group_rows)
    _check_columns(names, cols, elements, enc, lay.cuts)
    bodies = [body(cols[j][r:r + k], enc[j]) for r, k, j in lay.pages.tolist()]
    page_bytes = [len(b) for b in bodies]
    if any(codecs):
        if compress is None:
            from .snappy import stored_stream as compress
        bodies = [compress(bytes(b)) if codecs[j] else b for b, (_, _, j) in zip(bodies, lay.pages.tolist())]
    total, page_dst, spans, fills = lay.place(names, elements, enc, page_bytes, codecs, [len(b) for b in bodies])
    buf = bytearray(total)
    for at, b in fills + list(zip(page_dst.tolist(), bodies)):
        buf[at:at + len(b)] = b
    return [memoryview(buf)[a:b] for a, b in spans]


class DeviceJob:
    """One ``otto_pqw_job``: the column records of 1-d device tensors ``cols`` with the ``encodings`` (PLAIN / DELTA), the page
    table ``pages`` (``PAGE_DTYPE``), scratch, and the stream that is current when the job is made. :meth:`plan` and
    :meth:`emit` are the two entry points; everything they enqueue goes to that stream."""

    def __init__(self, cols, encodings, pages, work=None):
        import torch
        from . import _lib
        self.dev = dev = cols[0].device
        if dev.type != 'cuda':
            raise _lib.OttoError('parquet_write needs tensors on a ROCm device (no CPU fallback)')
        self.cols = [_lib.need(c, f'column {j}', c.dtype, 1, device=dev) for j, c in enumerate(cols)]
        self.pages = np.ascontiguousarray(pages, dtype=PAGE_DTYPE)
        self._records = (_lib.PqwColumn * len(cols))()
        for j, (c, e) in enumerate(zip(self.cols, encodings)):
            el = element(c.dtype)
            self._records[j] = _lib.PqwColumn(_lib.ptr(c, dev) if c.numel() else None, int(c.numel()), el[0], el[1], int(e), 0)
        self.job = _lib.PqwJob(self._records, len(cols), self.pages.ctypes.data_as(C.POINTER(_lib.PqwPage)), len(self.pages), None, 0,
                               _lib.stream(dev))
        need = int(_lib.lib().otto_pqw_workspace(C.byref(self.job)))
        if need < 0:
            _lib.check(need, 'otto_pqw_workspace')
        self.work_bytes = max(need, 256)
        if work is None:
            with torch.cuda.device(dev):
                work = _lib.workspace(need, dev)
        elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
            raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
        self.work = work
        self.job.d_work, self.job.work_bytes = _lib.ptr(work, dev), int(work.numel())

    def plan(self):
        """The bytes of every page body (int64 array); ``OttoError`` for a value outside the delta domain."""
        from . import _lib
        page_bytes = np.zeros(max(len(self.pages), 1), dtype=np.int64)
        _lib.call('otto_pqw_plan', self.dev, C.byref(self.job), page_bytes, stream=False)
        return page_bytes[:len(self.pages)]

    def emit(self, page_dst, d_out):
        """Page p's body to ``d_out[page_dst[p]:]`` (a uint8 device tensor), after :meth:`plan` on the same scratch."""
        import torch
        from . import _lib
        page_dst = np.ascontiguousarray(page_dst, dtype=np.int64)
        if len(page_dst) != len(self.pages):
            raise ValueError(f'page_dst: {len(page_dst)} offsets for {len(self.pages)} pages')
        _lib.need(d_out, 'd_out', torch.uint8, 1, device=self.dev)
        _lib.call('otto_pqw_emit', self.dev, C.byref(self.job), page_dst if len(page_dst) else None, d_out if d_out.numel() else None,
                  int(d_out.numel()), stream=False)


def _plan(job, names):
    """``job.plan()``; a value outside the delta domain is reported under the column's name."""
    from . import _lib
    try:
        return job.plan()
    except _lib.OttoError as e:
        m = re.search(r'column (\d+), row (\d+): (.*)', str(e))
        if m:
            raise _lib.OttoError(f'column {names[int(m.group(1))]!r}, row {m.group(2)}: {m.group(3)}') from None
        raise


def _encode_compressed(names, cols, elements, enc, codecs, lay, work):
    """The device side of :func:`encode_tables` when a column has a codec: the pages of the compressed columns are planned
    and emitted back to back into a staging buffer, ``otto_snappy_plan`` sizes their streams, and with those sizes placed
    ``otto_snappy_emit`` writes the streams and ``otto_pqw_emit`` the pages of the other columns into the one image.
    Returns ``(d_out, spans, fills)``."""
    import torch
    from . import snappy
    dev = cols[0].device
    packed = np.array([bool(codecs[j]) for j in lay.pages['column'].tolist()], dtype=bool)
    page_bytes = np.zeros(len(lay.pages), dtype=np.int64)
    stored = np.zeros(len(lay.pages), dtype=np.int64)
    with torch.cuda.device(dev):
        inner = DeviceJob(cols, enc, lay.pages[packed])
        page_bytes[packed] = _plan(inner, names)
        stage_off = np.r_[0, np.cumsum(page_bytes[packed])]
        stage = torch.empty(int(stage_off[-1]), dtype=torch.uint8, device=dev)
        inner.emit(stage_off[:-1], stage)
        codec = snappy.DeviceJob(stage, stage_off[:-1], page_bytes[packed])
        stored[packed] = codec.plan()
        outer = DeviceJob(cols, enc, lay.pages[~packed], work) if not packed.all() else None
        if outer is not None:
            page_bytes[~packed] = _plan(outer, names)
        total, page_dst, spans, fills = lay.place(names, elements, enc, page_bytes, codecs, stored)
        d_out = torch.empty(total, dtype=torch.uint8, device=dev)
        codec.emit(page_dst[packed], d_out)
        if outer is not None:
            outer.emit(page_dst[~packed], d_out)
    return d_out, spans, fills


def encode_tables(columns, cuts, encodings=None, page_rows=PAGE_ROWS, row_group_rows=ROW_GROUP_ROWS, work=None, compression=None):
    """``columns``: ``{name: 1-d tensor}`` of one length on one ROCm device; ``cuts``: ascending row numbers, rows
    ``[cuts[i], cuts[i + 1])`` become file image i. ``encodings``: ``{name: 'plain' | 'delta'}`` (default plain; delta for
    integer columns whose values lie in the domain SPEC-PQWRITE states, else ``OttoError`` naming column and row).

    One plan and one emit for all segments, one device-to-host copy into a page-locked buffer with the gaps for headers
    and footers in place, which the host then fills. Returns one ``memoryview`` per file (views of that one buffer).
    ``work``: a uint8 scratch tensor to use instead of a fresh one.

    ``compression``: None (the default: the bytes are what they always were), ``'snappy'`` for every column, or
    ``{name: None | 'snappy'}``. The pages of a Snappy column are compressed on the device (SPEC-SNAPPY) after their
    value encoding; the column's metadata names the codec, and pyarrow, pandas and ``otto_amd.parquet`` read the file."""
    import torch
    from . import _lib
    names, enc = _normalise(columns, encodings)
    codecs = _codecs(names, compression)
    cols = [columns[n] for n in names]
    if not all(isinstance(c, torch.Tensor) and c.dim() == 1 for c in cols):
        raise ValueError('columns: expected 1-d tensors')
    if cols[0].device.type != 'cuda':
        raise _lib.OttoError('parquet_write.encode_tables needs tensors on a ROCm device (no CPU fallback)')
    elements = [element(c.dtype) for c in cols]
    lay = Layout(len(names), cuts, page_rows, row_group_rows)
    _check_columns(names, cols, elements, enc, lay.cuts)
    dev = cols[0].device
    if any(codecs):
        d_out, spans, fills = _encode_compressed(names, cols, elements, enc, codecs, lay, work)
        total = int(d_out.numel())
    else:
        job = DeviceJob(cols, enc, lay.pages, work)
        page_bytes = _plan(job, names)
        total, page_dst, spans, fills = lay.place(names, elements, enc, page_bytes)
        with torch.cuda.device(dev):
            d_out = torch.empty(total, dtype=torch.uint8, device=dev)
            job.emit(page_dst, d_out)
    with torch.cuda.device(dev):
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host.copy_(d_out, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    buf = memoryview(host.numpy())
    for at, b in fills:
        buf[at:at + len(b)] = b
    return [buf[a:b] for a, b in spans]


def write_tables(paths, columns, cuts, encodings=None, page_rows=PAGE_ROWS, row_group_rows=ROW_GROUP_ROWS, work=None, compression=None):
    """:func:`encode_tables`, image i written to ``paths[i]`` with one ``write``. Returns the bytes of each file."""
    paths = [os.fspath(p) for p in paths]
    if len(paths) != len(cuts) - 1:
        raise ValueError(f'{len(paths)} paths for {len(cuts) - 1} segments')
    images = encode_tables(columns, cuts, encodings, page_rows, row_group_rows, work, compression)
    for path, image in zip(paths, images):
        with open(path, 'wb', buffering=0) as f:
            f.write(image)
    return [len(i) for i in images]


def write_table(path, columns, encodings=None, page_rows=PAGE_ROWS, row_group_rows=ROW_GROUP_ROWS, work=None, compression=None):
    """One file of all rows of ``columns``."""
    n = len(columns[next(iter(columns))]) if columns else 0
    return write_tables([path], columns, [0, n], encodings, page_rows, row_group_rows, work, compression)[0]
