"""Device-side JSONL ingest: the dataset's ``train.jsonl`` / ``test.jsonl``
-> the event columns ``otto_events_sort`` takes, parsed and validated by HIP kernels (``include/otto_jsonl.h``, SPEC-JSONL).

Reference code replaced: ``create_dataframe`` of ``src/utilities/dataset_writer_pickle.py:11-65`` (``pd.read_json(lines=True)``
and a Python loop over every event). ``parse_bytes`` is the device call; ``cut_chunk`` and ``read_columns`` are the host side
that brings a file of any size across in chunks of whole lines.
"""
import numpy as np

from .parquet import _read_full

TILE_BYTES = 4096            # OTTO_JSONL_TILE
MAX_PIECE = 256              # OTTO_JSONL_MAX_PIECE
COLUMNS = ('session', 'aid', 'ts', 'type', 'sess_off', 'sess_id')


def _parse(d_bytes, line0=0):
    """``parse_bytes`` and the number of newlines in the buffer."""
    import ctypes as C
    import torch
    from . import _lib
    if not isinstance(d_bytes, torch.Tensor) or d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1:
        raise ValueError('parse_bytes: expected a 1-d uint8 tensor')
    if d_bytes.device.type != 'cuda':
        raise _lib.OttoError('parse_bytes needs a ROCm device (no CPU fallback)')
    dev = d_bytes.device
    n = int(d_bytes.numel())
    if not d_bytes.is_contiguous() or d_bytes.data_ptr() % 16:
        d_bytes = d_bytes.clone()                      # a fresh allocation is contiguous and aligned
    lib = _lib.lib()
    with torch.cuda.device(dev):
        work_bytes = int(lib.otto_jsonl_workspace(n))
        work = _lib.workspace(work_bytes, dev)
        counts = (C.c_int64 * 2)()
        _lib.call('otto_jsonl_count', dev, d_bytes, n, counts, work, work_bytes)
        S, E = int(counts[0]), int(counts[1])
        session = torch.empty(E, dtype=torch.int32, device=dev)
        aid = torch.empty(E, dtype=torch.int32, device=dev)
        ts = torch.empty(E, dtype=torch.int64, device=dev)
        typ = torch.empty(E, dtype=torch.uint8, device=dev)
        sess_off = torch.empty(S + 1, dtype=torch.int64, device=dev)
        sess_id = torch.empty(S, dtype=torch.int32, device=dev)
        _lib.call('otto_jsonl_parse', dev, d_bytes, n, int(line0), S, E, session, aid, ts, typ, sess_off, sess_id, counts, work,
                  work_bytes)
        newlines = C.c_int64()
        _lib.call('otto_jsonl_newlines', dev, work, work_bytes, n, C.byref(newlines))
    return (session, aid, ts, typ, sess_off, sess_id), int(newlines.value)


def parse_bytes(d_bytes, line0=0):
    """A device uint8 tensor holding whole lines of JSONL -> ``(session, aid, ts, type, sess_off, sess_id)`` on the same
    device, in file order: per event ``session`` and ``aid`` int32 (the bit patterns of uint32), ``ts`` int64 as written,
    ``type`` uint8 (0 clicks / 1 carts / 2 orders); per non-blank line ``sess_id`` int32 [S] and the CSR ``sess_off`` int64
    [S + 1]. Count, allocate, parse. A line that violates SPEC-JSONL raises ``OttoError`` naming its 1-based number,
    counted from ``line0`` (the lines that precede the buffer in its file)."""
    return _parse(d_bytes, line0)[0]


def cut_chunk(buf, n, eof=False):
    """The number of leading bytes of ``buf[:n]`` that are whole lines: up to and including the last newline; the rest is
    the carry that goes in front of the next read. At the end of the file (``eof``) the last line may lack its newline and
    everything is taken. Pure host code; ``buf``: bytes, bytearray or a uint8 array."""
    if eof:
        return n
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf
    hi, step = n, 1 << 16
    while hi > 0:                                      # backwards in growing windows: the last line is short
        lo = max(0, hi - step)
        hit = np.flatnonzero(a[lo:hi] == 10)
        if len(hit):
            return lo + int(hit[-1]) + 1
        hi, step = lo, step * 4
    raise ValueError(f'a line longer than chunk_bytes ({n} bytes without a newline)')


def read_columns(paths, device, chunk_bytes=256 << 20):
    """The files ``paths`` (one path or a list, read in order) -> ``(session, aid, ts, type)`` device tensors of all their
    events in file order, as :func:`parse_bytes` returns them.

    Binary reads of ``chunk_bytes`` go into two page-locked staging buffers that alternate; each chunk is cut after its
    last newline (:func:`cut_chunk`) and the cut-off tail is carried in front of the next read; chunk i + 1 is read and
    copied on a side stream while chunk i is parsed (as ``ingest.feed_host_events`` does). ``line0`` runs across the chunks
    of a file and restarts with every file, so an ``OttoError`` names the line of that file."""
    import os
    import torch
    dev = torch.device(device)
    on_gpu = dev.type == 'cuda'
    if on_gpu and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if chunk_bytes < 1 or chunk_bytes >= 1 << 31:
        raise ValueError('chunk_bytes must be in [1, 2^31)')
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
    chunk_bytes = min(chunk_bytes, max([os.path.getsize(p) for p in paths], default=0) + 1)     # no staging beyond the largest file
    host = [torch.empty(chunk_bytes, dtype=torch.uint8, pin_memory=on_gpu) for _ in range(2)]
    devb = [torch.empty(chunk_bytes, dtype=torch.uint8, device=dev) for _ in range(2)] if on_gpu else host
    if on_gpu:
        copy_stream = torch.cuda.Stream(device=dev)
        compute = torch.cuda.current_stream(dev)
        # the device sets come from the caller's stream's allocator: a block it freed may still be read by work queued there
        copy_stream.wait_stream(compute)
        sent = [torch.cuda.Event(), torch.cuda.Event()]      # H2D of the set finished
        used = [torch.cuda.Event(), torch.cuda.Event()]      # the parse no longer reads the set
    cols = [[], [], [], []]

    def chunks(f):
        """(staging set, bytes of whole lines) per chunk; the set is read and on its way to the device when it is yielded"""
        b, carry, i = 0, None, 0
        while True:
            if on_gpu and i >= 2:
                used[b].synchronize()                        # the set is free again, host and device side
            view = host[b].numpy()
            keep = 0
            if carry is not None:
                keep = len(carry)
                view[:keep] = carry
            fill = keep + _read_full(f, memoryview(view)[keep:])
            eof = fill < chunk_bytes
            if fill == 0:
                return
            n = cut_chunk(view, fill, eof)
            carry = view[n:fill] if n < fill else None       # stays valid until this set is filled again, two chunks on
            if on_gpu:
                with torch.cuda.stream(copy_stream):
                    devb[b][:n].copy_(host[b][:n], non_blocking=True)
                    sent[b].record(copy_stream)
            yield b, n
            if eof:
                return
            b, i = b ^ 1, i + 1

    for path in paths:
        line0 = 0
        with open(path, 'rb', buffering=0) as f:
            it = chunks(f)
            cur = next(it, None)
            while cur is not None:
                nxt = next(it, None)                         # read and send chunk i + 1 before chunk i is parsed
                b, n = cur
                if on_gpu:
                    compute.wait_event(sent[b])
                out, newlines = _parse(devb[b][:n], line0)
                if on_gpu:
                    used[b].record(compute)
                for c, t in zip(cols, out[:4]):
                    c.append(t)
                line0 += newlines
                cur = nxt
    if on_gpu:
        torch.cuda.synchronize(dev)
    dtypes = (torch.int32, torch.int32, torch.int64, torch.uint8)
    return tuple(torch.cat(c) if c else torch.empty(0, dtype=dt, device=dev) for c, dt in zip(cols, dtypes))
