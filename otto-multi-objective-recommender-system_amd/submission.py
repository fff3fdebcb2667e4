"""The submission file from the device (SPEC-SUBMIT): per-session top lists -> the bytes of the
``session_type,labels`` CSV, formatted by HIP kernels (``include/otto_submit.h``), then copied out in chunks and written
plain or as multi-member gzip: compressed by zlib on the host or, with ``compressor='device'``, by the DEFLATE kernels of
``otto_amd.deflate`` (SPEC-DEFLATE) before the copy.

Reference code replaced: the per-row ``' '.join(str(aid) ...)`` loops and ``DataFrame.to_csv`` of
``src/ranker/inference.py:403-408,566-572`` (``blend_submission.csv.gz``) and ``src/covisitation/inference.py:387-391,
437-447`` (``covisitation_submission.csv.gz``). :func:`format_rows` is the device call; :func:`write_csv` is the host side
and takes host parts too, so it runs without a GPU.

``python -m otto_amd.submission blend --out blend_submission.csv.gz --clicks 0.3:a.npz 0.7:b.npz --carts ... --orders ...``
(every ``.npz`` holds ``session``, ``aid``, ``score``) and ``python -m otto_amd.submission covisitation --out
covisitation_submission.csv.gz predictions.npz`` (``session_id`` [S], ``pred`` [3, S, k], ``n`` [3, S]). ``--device-gzip``
compresses on the device.
"""
import gzip
import time

import numpy as np

HEADER = b'session_type,labels\n'
TYPES = ('clicks', 'carts', 'orders')          # type code -> suffix
MAX_K = 64                                     # OTTO_SUBMIT_MAX_K
MAX_WORKERS = 16
COMPRESSORS = ('zlib', 'device')


def format_rows(session_id, tables, types, interleave=False, header=False):
    """``session_id`` int32 [S] and ``tables``, a list of 1 to 3 ``(top_aid int32 [S, k] (a row stride >= k is kept),
    n int32 [S])`` on one device, ``types`` their type codes (0 clicks / 1 carts / 2 orders) -> a device uint8 tensor
    holding the lines ``<session>_<suffix>,<aid> <aid> ...\\n``. ``interleave=False``: one block of S lines per table (the
    blend script's order); ``True``: the tables' lines of a session follow each other (the covisitation script's). A
    session with ``n < 0`` gets no line. ``header=True`` prepends ``session_type,labels\\n``. Raises ``OttoError`` for
    ``n > k``, a negative session id or a negative aid among the first ``n``."""
    import ctypes as C
    import torch
    from . import _lib
    session_id = _lib.need(session_id, 'session_id', torch.int32, 1)
    dev = session_id.device
    S = int(session_id.numel())
    tables, types = list(tables), [int(c) for c in types]
    T = len(tables)
    if not 1 <= T <= 3 or len(types) != T:
        raise ValueError('tables: expected 1 to 3 (top_aid, n) pairs and as many type codes')
    if any(c not in (0, 1, 2) for c in types):
        raise ValueError('types: expected codes 0 (clicks), 1 (carts), 2 (orders)')
    k = ld = None
    for t, (top, n) in enumerate(tables):
        _lib.need(n, f'n of table {t}', torch.int32, 1, device=dev, numel=S)
        if not isinstance(top, torch.Tensor) or top.dtype != torch.int32 or top.dim() != 2 or top.device != dev or top.shape[0] != S:
            raise ValueError(f'top_aid of table {t}: expected an int32 [S, k] tensor on {dev}')
        if top.stride(1) != 1 and top.numel():
            raise ValueError(f'top_aid of table {t}: rows must be contiguous')
        row = int(top.stride(0)) if S > 1 else int(top.shape[1])
        if (k, ld) != (None, None) and (k, ld) != (int(top.shape[1]), row):
            raise ValueError('tables: all top_aid tensors must have one k and one row stride')
        k, ld = int(top.shape[1]), row
    if not 1 <= k <= MAX_K or ld < k:
        raise ValueError(f'k must be in [1, {MAX_K}] and the row stride at least k (got k = {k}, stride {ld})')
    head = HEADER if header else b''
    arr = lambda i: (C.c_void_p * T)(*[_lib.ptr(tb[i]) if S else None for tb in tables])
    tops, ns, codes = arr(0), arr(1), (C.c_int32 * T)(*types)
    work_bytes = int(_lib.lib().otto_submit_workspace(S, T))
    work = _lib.workspace(work_bytes, dev)
    total = C.c_int64(0)
    _lib.call('otto_submit_measure', dev, T, tops, ns, codes, session_id, S, k, ld, int(bool(interleave)), C.byref(total), work,
              work_bytes)
    out = torch.empty(len(head) + int(total.value), dtype=torch.uint8, device=dev)
    if head:
        out[:len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
    if out.data_ptr() % 16:
        raise _lib.OttoError('format_rows: the allocator returned an unaligned buffer')
    _lib.call('otto_submit_format', dev, T, tops, ns, codes, session_id, S, k, ld, int(bool(interleave)), out, int(out.numel()),
              len(head), work, work_bytes)
    return out


def _member(data, level):
    return gzip.compress(data, compresslevel=level, mtime=0)


def _host_chunks(part, chunk_bytes):
    a = np.frombuffer(part, dtype=np.uint8) if isinstance(part, (bytes, bytearray, memoryview)) else np.ascontiguousarray(part, dtype=np.uint8).ravel()
    for lo in range(0, a.size, chunk_bytes):
        yield a[lo:lo + chunk_bytes].tobytes()


def _device_chunks(part, chunk_bytes, state, stats):
    """Chunks of a device uint8 tensor through one pair of pinned buffers on a side stream: chunk i + 1 is on its way while
    chunk i is handed on. A chunk is copied out of the pinned buffer (its slot is filled again two chunks later)."""
    import torch
    dev = part.device
    n = int(part.numel())
    size = min(chunk_bytes, n)
    if state.get('size', 0) < size or state.get('dev') != dev:
        state.update(size=size, dev=dev, host=[torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(2)],
                     stream=torch.cuda.Stream(device=dev), done=[torch.cuda.Event(), torch.cuda.Event()])
    host, side, done = state['host'], state['stream'], state['done']
    side.wait_stream(torch.cuda.current_stream(dev))         # the part is complete before the first copy reads it

    def send(i):
        lo = i * chunk_bytes
        m = min(chunk_bytes, n - lo)
        with torch.cuda.stream(side):
            host[i & 1][:m].copy_(part[lo:lo + m], non_blocking=True)
            done[i & 1].record(side)
        return m

    count = -(-n // chunk_bytes)
    m_next = send(0) if count else 0
    for i in range(count):
        m = m_next
        if i + 1 < count:
            m_next = send(i + 1)
        t0 = time.perf_counter()
        done[i & 1].synchronize()
        data = host[i & 1][:m].numpy().tobytes()
        stats['copy_s'] += time.perf_counter() - t0
        yield data
    part.record_stream(side)


class _Ready:
    """A chunk that is compressed already, in the place of a future of the zlib pool."""

    def __init__(self, data):
        self.data = data

    def result(self):
        return self.data, 0.0


def _device_members(part, chunk_bytes, state, stats):
    """Chunks of a device uint8 tensor, each compressed on the device (one call of ``deflate.gzip_members`` per chunk, so
    its scratch is bounded by ``chunk_bytes``) and brought across through the pinned buffer pair: (bytes, chunk length)."""
    import torch
    from . import deflate
    n = int(part.numel())
    size = min(chunk_bytes, n)
    if state.get('z_size', 0) < size or state.get('z_dev') != part.device:      # one workspace and one output for all chunks
        state.update(z_size=size, z_dev=part.device,
                     z_work=torch.empty(deflate.workspace_bytes(size), dtype=torch.uint8, device=part.device),
                     z_out=torch.empty(deflate.compressed_bound(size), dtype=torch.uint8, device=part.device))
    for lo in range(0, n, chunk_bytes):
        m = min(chunk_bytes, n - lo)
        t0 = time.perf_counter()
        z = deflate.gzip_members(part[lo:lo + m], work=state['z_work'], out=state['z_out'])
        torch.cuda.current_stream(part.device).synchronize()
        stats['device_s'] += time.perf_counter() - t0
        first = True
        for data in _device_chunks(z, chunk_bytes, state, stats):
            yield data, m if first else 0
            first = False


def write_csv(path, parts, level=6, chunk_bytes=32 << 20, threads=8, compressor='zlib'):
    """Write the concatenation of ``parts`` to ``path``. A part is a device uint8 tensor (:func:`format_rows`), host
    ``bytes`` or a NumPy uint8 array. Parts are cut into chunks of ``chunk_bytes``; device chunks come across through one
    pinned buffer pair on a side stream. A path that ends in ``.gz`` compresses every chunk as a gzip member of its own
    (``mtime=0``, so two runs give identical files; ``gzip`` and ``pandas.read_csv`` read the members as one stream) in a
    pool of ``min(threads, 16)`` workers and writes them in order; any other path is written plain. Returns a dict of
    ``bytes`` (uncompressed), ``file_bytes`` and the seconds spent waiting for copies (``copy_s``), inside zlib summed
    over the workers (``zlib_s``) and in file writes (``file_s``).

    ``compressor='device'`` compresses the chunks of device parts with the DEFLATE kernels (``otto_amd.deflate``: gzip
    members of 64 KiB, ``level`` does not apply) and copies the compressed bytes across; host parts still go through the
    zlib pool, and a file of mixed members is a valid gzip file. The seconds inside those calls are ``device_s``, an
    entry that exists only under ``'device'``. A plain path ignores the compressor. Any other name is a ``ValueError``."""
    import collections
    import concurrent.futures
    import os
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes must be at least 1')
    if threads < 1:
        raise ValueError('threads must be at least 1')
    if compressor not in COMPRESSORS:
        raise ValueError(f'compressor must be one of {COMPRESSORS} (got {compressor!r})')
    workers = min(int(threads), MAX_WORKERS)
    zipped = str(os.fspath(path)).endswith('.gz')
    stats = dict(bytes=0, file_bytes=0, copy_s=0.0, zlib_s=0.0, file_s=0.0)
    on_device = zipped and compressor == 'device'
    if compressor == 'device':
        stats['device_s'] = 0.0
    state = {}

    def chunks():
        """(bytes, uncompressed length, compressed already)"""
        raw = lambda it: ((data, len(data), False) for data in it)
        for part in parts:
            if isinstance(part, (bytes, bytearray, memoryview, np.ndarray)):
                yield from raw(_host_chunks(part, chunk_bytes))
            else:
                import torch
                from . import _lib
                if not isinstance(part, torch.Tensor) or part.dtype != torch.uint8 or part.dim() != 1:
                    raise ValueError('parts: expected 1-d uint8 device tensors, bytes or NumPy uint8 arrays')
                if part.device.type != 'cuda':
                    yield from raw(_host_chunks(part.numpy(), chunk_bytes))
                elif on_device:
                    for data, m in _device_members(part.contiguous(), chunk_bytes, state, stats):
                        yield data, m, True
                else:
                    yield from raw(_device_chunks(part.contiguous(), chunk_bytes, state, stats))

    def job(data):
        t0 = time.perf_counter()
        z = _member(data, level)
        return z, time.perf_counter() - t0

    def put(f, data):
        t0 = time.perf_counter()
        f.write(data)
        stats['file_s'] += time.perf_counter() - t0
        stats['file_bytes'] += len(data)

    with open(path, 'wb') as f:
        if not zipped:
            for data, _, _ in chunks():
                stats['bytes'] += len(data)
                put(f, data)
            return stats
        pending = collections.deque()

        def drain(keep):
            while len(pending) > keep:
                z, dt = pending.popleft().result()
                stats['zlib_s'] += dt
                put(f, z)

        with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
            for data, m, ready in chunks():
                stats['bytes'] += m
                pending.append(_Ready(data) if ready else pool.submit(job, data))
                drain(2 * workers)                           # bounds the chunks held in memory
            drain(0)
        if stats['bytes'] == 0:
            put(f, _member(b'', level))                      # an empty file is not a gzip stream
    return stats


def blend_submission(path, families_by_type, weights_by_type, k=20, left_of_base_by_type=None, **write_args):
    """``blend_submission.csv.gz`` of ``src/ranker/inference.py``: ``families_by_type`` and ``weights_by_type`` hold, for
    clicks, carts and orders in that order, the models ``(session, aid, score)`` and weights that ``blend.blend_topk``
    takes (``left_of_base_by_type``: its flags). Three blocks in the reference's order, every block with the session list
    of its own blend, under one header. Returns what :func:`write_csv` returns."""
    from .ranker import blend
    if len(families_by_type) != 3 or len(weights_by_type) != 3:
        raise ValueError('expected the families and weights of clicks, carts and orders')
    left = left_of_base_by_type or (None, None, None)
    parts = []
    for t in range(3):
        sid, top, n = blend.blend_topk(families_by_type[t], weights_by_type[t], left[t], k=k)
        parts.append(format_rows(sid.contiguous(), [(top, n)], [t], header=t == 0))
    return write_csv(path, parts, **write_args)


def covisitation_submission(path, session_id, pred, n, **write_args):
    """``covisitation_submission.csv.gz`` of ``src/covisitation/inference.py``: ``pred`` int32 [3, S, k] and ``n`` int32
    [3, S] as ``recency_predictions`` and the stacked ``predictions`` of clicks, carts and orders give them; the three lines
    of a session follow each other. Sessions with ``n < 0`` (the other branch's) get no line."""
    if pred.dim() != 3 or pred.shape[0] != 3 or n.dim() != 2 or n.shape[0] != 3:
        raise ValueError('expected pred [3, S, k] and n [3, S]')
    tables = [(pred[t], n[t].contiguous()) for t in range(3)]
    return write_csv(path, [format_rows(session_id, tables, [0, 1, 2], interleave=True, header=True)], **write_args)


def _main(argv=None):
    import argparse
    import torch
    parser = argparse.ArgumentParser(prog='python -m otto_amd.submission')
    sub = parser.add_subparsers(dest='mode', required=True)
    b = sub.add_parser('blend', help='robust-scale, join and weight score files, write the three blocks')
    b.add_argument('--out', required=True)
    for name in TYPES:
        b.add_argument(f'--{name}', nargs='+', required=True, metavar='WEIGHT:FILE.npz', help='session, aid, score per file')
    b.add_argument('--k', type=int, default=20)
    c = sub.add_parser('covisitation', help='write session_id [S], pred [3, S, k], n [3, S] of an .npz, interleaved')
    c.add_argument('--out', required=True)
    c.add_argument('predictions')
    for p in (b, c):
        p.add_argument('--device', default='cuda:0')
        p.add_argument('--level', type=int, default=6)
        p.add_argument('--threads', type=int, default=8)
        p.add_argument('--device-gzip', action='store_true', help='compress on the device (otto_amd.deflate) instead of zlib')
    args = parser.parse_args(argv)
    dev = torch.device(args.device)
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    write_args = dict(level=args.level, threads=args.threads, compressor='device' if args.device_gzip else 'zlib')
    if args.mode == 'blend':
        families, weights = [], []
        for name in TYPES:
            models, w = [], []
            for item in getattr(args, name):
                weight, _, file = item.partition(':')
                z = np.load(file)
                models.append((put(z['session'], np.int32), put(z['aid'], np.int32), put(z['score'], np.float64)))
                w.append(float(weight))
            families.append(models)
            weights.append(w)
        stats = blend_submission(args.out, families, weights, k=args.k, **write_args)
    else:
        z = np.load(args.predictions)
        stats = covisitation_submission(args.out, put(z['session_id'], np.int32), put(z['pred'], np.int32), put(z['n'], np.int32),
                                        **write_args)
    print(f"{args.out}: {stats['bytes']} bytes of text, {stats['file_bytes']} bytes written")


if __name__ == '__main__':
    _main()
