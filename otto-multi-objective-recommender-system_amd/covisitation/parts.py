"""The covisitation part files back on the device (SPEC-ROWS, ``include/otto_rows.h``): the
``top_15_<kind>_<i>.pqt`` / ``top_<kind>_<i>.pqt`` files a builder run left -- written by pyarrow or by ``--device-write`` --
-> the padded ``(aid_y [n_aids, k], wgt [n_aids, k], n [n_aids])`` arrays ``candidates.candidate_lookup`` takes. The pages are
decoded by ``parquet.read_columns`` (delta, PLAIN and dictionary pages, float columns as bit copies) and the rows regrouped
by ``otto_rows_topk``; no row is touched on the host.

Reference code replaced: the ``pd.read_parquet`` + ``groupby`` / ``dict.update`` chains of
``src/covisitation/inference.py:87-111``, ``src/ranker/covisitation_candidate_generation.py:49-73`` and
``src/ranker/regular_candidate_generation.py:75-101``.
"""
import ctypes as C
import os
import pathlib

import numpy as np

from .. import _lib
from .spec import REFERENCE_KINDS

COLUMNS = ('aid_x', 'aid_y', 'wgt')
MAX_K = 64                                   # OTTO_ROWS_MAX_K
REASONS = {1: 'aid_x outside [0, n_aids)', 2: 'aid_y outside [0, n_aids)', 3: "aid_x below the previous row's", 4: 'a run longer than k'}


def rows_to_topk(aid_x, aid_y, wgt, n_aids, k, work=None):
    """SPEC-ROWS: rows ``aid_x int32, aid_y int32, wgt float32`` with ``aid_x`` non-decreasing -> ``(y int32 [n_aids, k],
    w float32 [n_aids, k], n int32 [n_aids])``; unused slots are ``y = -1, w = 0``. ``OttoError`` naming the smallest
    offending row for an id outside ``[0, n_aids)``, a descending ``aid_x`` or a run longer than ``k``. ``work``: a uint8
    scratch tensor to use instead of a fresh one."""
    import torch
    dev = aid_x.device if isinstance(aid_x, torch.Tensor) else None
    if dev is None or dev.type != 'cuda':
        raise _lib.OttoError('parts.rows_to_topk needs tensors on a ROCm device (no CPU fallback)')
    n_rows = int(aid_x.numel())
    _lib.need(aid_x, 'aid_x', torch.int32, 1, device=dev)
    _lib.need(aid_y, 'aid_y', torch.int32, 1, device=dev, numel=n_rows)
    _lib.need(wgt, 'wgt', torch.float32, 1, device=dev, numel=n_rows)
    n_aids, k = int(n_aids), int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    if not 0 <= n_aids < 1 << 31:
        raise ValueError(f'n_aids must be in [0, 2^31) (got {n_aids})')
    with torch.cuda.device(dev):
        y = torch.empty((n_aids, k), dtype=torch.int32, device=dev)
        w = torch.empty((n_aids, k), dtype=torch.float32, device=dev)
        n = torch.empty(n_aids, dtype=torch.int32, device=dev)
        job = _lib.RowsJob(_lib.ptr(aid_x, dev), _lib.ptr(aid_y, dev), _lib.ptr(wgt, dev), n_rows, _lib.ptr(y, dev), _lib.ptr(w, dev),
                           _lib.ptr(n, dev), n_aids, k, 0, None, 0, _lib.stream(dev))
        need = int(_lib.lib().otto_rows_workspace(C.byref(job)))
        if need < 0:
            _lib.check(need, 'otto_rows_workspace')
        if work is None:
            work = _lib.workspace(need, dev)
        elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
            raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
        job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
        err = np.full(2, -1, dtype=np.int64)
        try:
            _lib.call('otto_rows_topk', dev, C.byref(job), err, stream=False)
        except _lib.OttoError:
            if err[0] < 0:
                raise
            raise _lib.OttoError(f'rows_to_topk: row {int(err[0])}: {REASONS.get(int(err[1]), "?")}') from None
    return y, w, n


def read_parts(paths, device):
    """``(aid_x int32, aid_y int32, wgt float32)`` of the part files ``paths``, in part order, decoded on the device."""
    import torch
    from .. import parquet
    paths = [os.fspath(p) for p in paths]
    return parquet.read_columns(paths, list(COLUMNS), device, floats=True,
                                dtypes={'aid_x': torch.int32, 'aid_y': torch.int32, 'wgt': torch.float32})


def part_paths(directory, prefix, kind, n_parts):
    return [pathlib.Path(directory) / f'{prefix}_{kind}_{i}.pqt' for i in range(n_parts)]


def load_matrix(directory, prefix, kind, n_parts, n_aids, k, device):
    """The ``n_parts`` files ``<prefix>_<kind>_<i>.pqt`` of ``directory`` -> ``(y, w, n)`` (:func:`rows_to_topk`). The parts
    partition aid_x into ascending ranges, so their rows in part order are sorted. ``n_aids=None``: one past the largest
    aid in the files."""
    import torch
    aid_x, aid_y, wgt = read_parts(part_paths(directory, prefix, kind, n_parts), device)
    if n_aids is None:
        n_aids = int(torch.maximum(aid_x.max(), aid_y.max())) + 1 if aid_x.numel() else 0
    return rows_to_topk(aid_x, aid_y, wgt, n_aids, k)


def load_matrices(directory, mode, which, n_aids, device, kinds=REFERENCE_KINDS):
    """``{kind: (y, w, n)}`` of one family of part files of a builder run, as ``candidate_lookup`` takes it. ``which``:
    ``'top_15'`` (top-15 per aid, the files of the candidate generators of ``mode``) or ``'top'`` (top-20, both modes).
    ``n_aids=None``: one past the largest aid in any of the files."""
    import torch
    from . import builder
    if mode not in ('validation', 'submission'):
        raise ValueError('Invalid mode')
    if which not in ('top_15', 'top'):
        raise ValueError(f"which must be 'top_15' or 'top' (got {which!r})")
    k = 15 if which == 'top_15' else 20
    rows = {}
    for kind in kinds:
        co = kind == 'cart_order'
        if which == 'top_15':
            n_parts = builder.TOP15_CART_ORDER_PARTS[mode] if co else builder.TOP15_PARTS[mode]
        else:
            n_parts = builder.TOP_CART_ORDER_PARTS if co else builder.TOP_PARTS
        rows[kind] = read_parts(part_paths(directory, which, kind, n_parts), device)
    if n_aids is None:
        n_aids = max([int(torch.maximum(x.max(), y.max())) + 1 for x, y, _ in rows.values() if x.numel()], default=0)
    return {kind: rows_to_topk(*r, n_aids, k) for kind, r in rows.items()}
