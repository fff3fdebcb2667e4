"""Device-side Snappy encoder (SPEC-SNAPPY, ``include/otto_snappy.h``): extents of a device uint8
tensor -> one Snappy raw-format stream each, compressed by HIP kernels (``csrc/otto_snappy.hip``). ``pyarrow.Codec('snappy')``,
python-snappy and :func:`otto_amd.parquet.snappy_decompress` read the streams; :mod:`otto_amd.parquet_write` uses them as the
page codec under ``compression='snappy'``.

Reference code replaced: the Snappy call inside pyarrow behind ``DataFrame.to_parquet`` of ``src/covisitation/covisitation.py``
and ``src/utilities/split_dataset_writer_parquet.py``.
"""
import ctypes as C

import numpy as np


def compressed_bound(n):
    """The most bytes a stream of ``n`` input bytes has: ``32 + n + n // 6``."""
    from . import _lib
    if n < 0:
        raise ValueError('n must not be negative')
    return int(_lib.lib().otto_snappy_bound(int(n)))


class DeviceJob:
    """One ``otto_snappy_job``: the extents ``src_off`` / ``src_len`` (int64 host arrays) of the 1-d uint8 device tensor
    ``d_bytes``, scratch, and the stream that is current when the job is made. :meth:`plan` and :meth:`emit` are the two
    entry points; everything they enqueue goes to that stream."""

    def __init__(self, d_bytes, src_off, src_len, work=None):
        import torch
        from . import _lib
        self.dev = dev = d_bytes.device
        self.d_bytes = d_bytes
        self.src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        self.src_len = np.ascontiguousarray(src_len, dtype=np.int64)
        n = len(self.src_off)
        self.job = _lib.SnappyJob(_lib.ptr(d_bytes, dev) if d_bytes.numel() else None, int(d_bytes.numel()),
                                  self.src_off.ctypes.data_as(C.c_void_p) if n else None, self.src_len.ctypes.data_as(C.c_void_p) if n else None,
                                  n, None, 0, _lib.stream(dev))
        need = int(_lib.lib().otto_snappy_workspace(C.byref(self.job)))
        if need < 0:
            _lib.check(need, 'otto_snappy_workspace')
        if work is None:
            with torch.cuda.device(dev):
                work = _lib.workspace(need, dev)
        elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
            raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
        self.work = work
        self.job.d_work, self.job.work_bytes = _lib.ptr(work, dev), int(work.numel())

    def plan(self):
        """The bytes of every stream (int64 array)."""
        from . import _lib
        sizes = np.zeros(max(len(self.src_off), 1), dtype=np.int64)
        _lib.call('otto_snappy_plan', self.dev, C.byref(self.job), sizes, stream=False)
        return sizes[:len(self.src_off)]

    def emit(self, dst_off, d_out):
        """Stream i to ``d_out[dst_off[i]:]`` (a uint8 device tensor), after :meth:`plan` on the same scratch."""
        import torch
        from . import _lib
        dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
        if len(dst_off) != len(self.src_off):
            raise ValueError(f'dst_off: {len(dst_off)} offsets for {len(self.src_off)} streams')
        _lib.need(d_out, 'd_out', torch.uint8, 1, device=self.dev)
        _lib.call('otto_snappy_emit', self.dev, C.byref(self.job), dst_off if len(dst_off) else None, d_out if d_out.numel() else None,
                  int(d_out.numel()), stream=False)


def compress_extents(d_bytes, src_off, src_len, out=None, dst_off=None, work=None):
    """Stream i is the Snappy raw-format stream of ``d_bytes[src_off[i] : src_off[i] + src_len[i]]``. Returns ``(out, sizes)``:
    ``out`` a device uint8 tensor that holds stream i at ``dst_off[i]`` (default: the streams back to back, in a fresh
    tensor), ``sizes`` an int64 NumPy array, the bytes of each stream. Nothing outside a stream's own extent of ``out`` is
    written; extents that overlap or leave ``out`` are an ``OttoError`` and nothing is written at all. ``work``: a uint8
    scratch tensor to use instead of a fresh one. The bytes are fully determined by the input bytes."""
    import torch
    from . import _lib
    if not isinstance(d_bytes, torch.Tensor) or d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1:
        raise ValueError('compress_extents: expected a 1-d uint8 tensor')
    if d_bytes.device.type != 'cuda':
        raise _lib.OttoError('compress_extents needs a ROCm device (no CPU fallback)')
    dev = d_bytes.device
    a = lambda v: np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.int64)))
    src_off, src_len = a(src_off), a(src_len)
    n = len(src_off)
    if len(src_len) != n:
        raise ValueError('compress_extents: src_off and src_len must have one entry per stream')
    if dst_off is not None and len(a(dst_off)) != n:
        raise ValueError('compress_extents: dst_off must have one entry per stream')
    if not d_bytes.is_contiguous():
        d_bytes = d_bytes.contiguous()
    job = DeviceJob(d_bytes, src_off, src_len, work)
    sizes = job.plan().copy()
    dst_off = a(np.r_[0, np.cumsum(sizes)[:-1]] if dst_off is None else dst_off)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.zeros(int((dst_off + sizes).max()) if n else 0, dtype=torch.uint8, device=dev)
        _lib.need(out, 'compress_extents: out', torch.uint8, dim=1, device=dev)
        job.emit(dst_off, out)
    return out, sizes


def compress(d_bytes):
    """The Snappy raw-format stream of all of ``d_bytes``, a 1-d uint8 tensor on a ROCm device."""
    import torch
    if not isinstance(d_bytes, torch.Tensor):
        raise ValueError('compress: expected a 1-d uint8 tensor')
    return compress_extents(d_bytes, [0], [int(d_bytes.numel())])[0]


def stored_stream(data):
    """A valid Snappy raw-format stream of ``data`` made of literal elements alone, on the host: what
    ``parquet_write.encode_tables_host`` compresses with when it is given no ``compress`` function (tests)."""
    data = bytes(data)
    out, n = bytearray(), len(data)
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    for i in range(0, len(data), 65536):
        piece = data[i:i + 65536]
        k = len(piece) - 1
        out += bytes([k << 2]) if k < 60 else bytes([60 << 2, k]) if k < 256 else bytes([61 << 2, k & 0xFF, k >> 8])
        out += piece
    return bytes(out)
