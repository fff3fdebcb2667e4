"""Device engine of the covisitation builder: thin Python over the C-ABI of
``include/otto_covis.h`` (hand-written gfx950 kernels in ``csrc/otto_covis.hip``).

torch is used only to own device buffers and the stream.  No CPU fallback.
"""
import ctypes as C
import numpy as np

from .. import _lib
from .spec import TYPE_WEIGHTS, FILTER_MASKS, TIME_KIND, ALL_KINDS, mask_bits


class CovisBuilder:
    """One context per device. ``feed`` session chunks, then ``finalize``.

    Parameters mirror SPEC-COVIS: ``window`` (tail window W), ``max_gap`` seconds,
    ``kinds`` (subset of ``spec.ALL_KINDS``), ``ts_min``/``ts_max`` = t0/t1 of the
    time weight (global over every chunk and rank).
    """

    def __init__(self, n_aids, kinds=ALL_KINDS, window=30, max_gap=86400, ts_min=0, ts_max=0, device='cuda:0'):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.OttoError('CovisBuilder needs a ROCm device (no CPU fallback)')
        unknown = [k for k in kinds if k not in ALL_KINDS]
        if unknown:
            raise ValueError(f'unknown covisitation kinds {unknown}')
        self.kinds = tuple(kinds)
        self.n_aids = int(n_aids)
        self.type_kinds = [k for k in self.kinds if k in TYPE_WEIGHTS]
        self.filter_kinds = [k for k in self.kinds if k in FILTER_MASKS]
        self.want_time = TIME_KIND in self.kinds
        p = _lib.CovisParams()
        p.window, p.max_gap, p.n_aids = int(window), int(max_gap), self.n_aids
        p.ts_min, p.ts_max, p.want_time = int(ts_min), int(ts_max), int(self.want_time)
        p.n_filters = len(self.filter_kinds)
        for i, k in enumerate(self.filter_kinds):
            p.filter_mask[i] = mask_bits(FILTER_MASKS[k])
        p.n_type_weights = len(self.type_kinds)
        for i, k in enumerate(self.type_kinds):
            for t in range(3):
                p.type_weight[i][t] = TYPE_WEIGHTS[k][t]
        self._lib = _lib.lib()                    # close() may run while the interpreter shuts down
        self._ctx = C.c_void_p()
        _lib.call('otto_covis_create', self.device, C.byref(self._ctx), C.byref(p), stream=False)

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx:
            self._lib.otto_covis_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _call(self, name, *args, **kw):
        _lib.call(name, self.device, self._ctx, *args, **kw)

    def reset(self):
        self._call('otto_covis_reset', stream=False)

    def feed(self, aid, ts, typ, sess_off):
        """K1 pair-expand over one session chunk (device tensors: aid int32, ts int32,
        type uint8, sess_off int64 CSR with n_sess+1 entries)."""
        t = self.torch
        for name, x, dt in (('aid', aid, t.int32), ('ts', ts, t.int32), ('type', typ, t.uint8), ('sess_off', sess_off, t.int64)):
            _lib.need(x, name, dt, device=self.device)
        if aid.numel() != ts.numel() or aid.numel() != typ.numel():
            raise ValueError('aid/ts/type length mismatch')
        self._call('otto_covis_feed', aid, ts, typ, sess_off, sess_off.numel() - 1)

    def _finalize_group(self, group, n_kinds, k, out=None):
        t = self.torch
        if out is None:
            out = (t.empty((n_kinds, self.n_aids, k), dtype=t.int32, device=self.device),
                   t.empty((n_kinds, self.n_aids, k), dtype=t.int64, device=self.device),
                   t.empty((n_kinds, self.n_aids), dtype=t.int32, device=self.device))
        y, w, n = out
        self._call('otto_covis_finalize', group, int(k), y, w, n)
        return y, w, n

    def finalize(self, k=20, out=None):
        """Reduce + top-k. Returns {kind: (aid_y int32 [n_aids,k], W int64 [n_aids,k], n int32 [n_aids])}.

        ``out`` optionally maps group id -> preallocated (y, w, n) tensors (bench reuse).
        """
        res = {}
        groups = ((_lib.GROUP_TYPE, self.type_kinds), (_lib.GROUP_FILTER, self.filter_kinds),
                  (_lib.GROUP_TIME, [TIME_KIND] if self.want_time else []))
        for group, names in groups:
            if not names:
                continue
            y, w, n = self._finalize_group(group, len(names), k, None if out is None else out.get(group))
            for i, name in enumerate(names):
                res[name] = (y[i], w[i], n[i])
        return res

    def set_option(self, name, value):
        self._call('otto_covis_set_option', name.encode(), int(value), stream=False)

    def stats(self):
        buf = (C.c_int64 * len(_lib.STAT_NAMES))()
        self._call('otto_covis_stats', buf, stream=False)
        return dict(zip(_lib.STAT_NAMES, [int(v) for v in buf]))

    def timings(self):
        """Per-kernel device milliseconds (hipEvents on the stream) of the last feed/finalize."""
        buf = (C.c_float * len(_lib.TIMING_NAMES))()
        self._lib.otto_covis_timings(self._ctx, buf)            # returns the slot count, not an error code
        return dict(zip(_lib.TIMING_NAMES, [float(v) for v in buf]))

    def kernel_names(self):
        """{timing slot: kernels launched under it since the last reset} as the library itself reports them."""
        out = {}
        for i, name in enumerate(_lib.TIMING_NAMES):
            buf = C.create_string_buffer(1024)
            self._call('otto_covis_kernel_names', i, buf, 1024, stream=False)
            out[name] = buf.value.decode()
        return out

    def copy_records(self):
        """Test hook: raw K1 output on the host (rec, tw or None, run_x, run_desc)."""
        st = self.stats()
        rec = np.empty(st['pair_slots'], dtype=np.uint32)
        tw = np.empty(st['pair_slots'], dtype=np.uint32) if self.want_time else None
        run_x = np.empty(st['tail_events'], dtype=np.uint32)
        run_desc = np.empty(st['tail_events'], dtype=np.uint64)
        self._call('otto_covis_copy_records', rec, tw, run_x, run_desc, stream=False)
        return rec, tw, run_x, run_desc

    # ---- multi-GPU exchange (SURVEY.md section 8 e) ------------------------------------------------
    def export_runs(self, x_lo, x_hi):
        """Runs with aid_x in [x_lo, x_hi) as device tensors (hdr int32 [n_runs,2], rec int32, tw int32|None)."""
        t = self.torch
        nr, nc = C.c_int64(), C.c_int64()
        self._call('otto_covis_export_count', int(x_lo), int(x_hi), C.byref(nr), C.byref(nc))
        hdr = t.empty((nr.value, 2), dtype=t.int32, device=self.device)
        rec = t.empty(nc.value, dtype=t.int32, device=self.device)
        tw = t.empty(nc.value, dtype=t.int32, device=self.device) if self.want_time else None
        self._call('otto_covis_export_runs', int(x_lo), int(x_hi), hdr, rec, tw)
        return hdr, rec, tw

    def export_all(self, bounds):
        """Every owner's piece in ONE owner-major buffer (owner o = aid_x in [bounds[o], bounds[o+1])): returns
        (hdr int32 [n_runs,2], rec int32 [n_recs], tw|None, runs_per_owner, recs_per_owner) -- the send buffers and
        split sizes of the all-to-all-v."""
        t = self.torch
        W = len(bounds) - 1
        hb = (C.c_uint32 * (W + 1))(*[int(b) for b in bounds])
        nr, nc = (C.c_int64 * W)(), (C.c_int64 * W)()
        self._call('otto_covis_export_plan', W, hb, nr, nc)
        runs, recs = [int(v) for v in nr], [int(v) for v in nc]
        hdr = t.empty((sum(runs), 2), dtype=t.int32, device=self.device)
        rec = t.empty(sum(recs), dtype=t.int32, device=self.device)
        tw = t.empty(sum(recs), dtype=t.int32, device=self.device) if self.want_time else None
        self._call('otto_covis_export_fill', W, hb, hdr, rec, tw)
        return hdr, rec, tw, runs, recs

    def export_plan_range(self, bounds, slot_lo, slot_hi):
        """(runs_per_owner, recs_per_owner) of the run slots [slot_lo, slot_hi) (chunked exchange; synchronises the stream)."""
        W = len(bounds) - 1
        hb = (C.c_uint32 * (W + 1))(*[int(b) for b in bounds])
        nr, nc = (C.c_int64 * W)(), (C.c_int64 * W)()
        self._call('otto_covis_export_plan_range', W, hb, int(slot_lo), int(slot_hi), nr, nc)
        return [int(v) for v in nr], [int(v) for v in nc]

    def export_fill_range(self, bounds, slot_lo, slot_hi, runs, recs, hdr, rec, tw=None):
        """Fills the owner-major send buffers of one slot range (``hdr`` int32 [sum(runs), 2], ``rec`` int32 [sum(recs)],
        ``tw`` like rec or None) on the current stream; no synchronisation."""
        W = len(bounds) - 1
        hb = (C.c_uint32 * (W + 1))(*[int(b) for b in bounds])
        nr, nc = (C.c_int64 * W)(*runs), (C.c_int64 * W)(*recs)
        self._call('otto_covis_export_fill_range', W, hb, int(slot_lo), int(slot_hi), nr, nc, hdr, rec, tw)

    def run_slots(self):
        return self.stats()['tail_events']

    def import_reserve(self, n_recs):
        """Zero-copy receive buffers: int32 tensors (rec, tw|None) that alias the end of the context's own record arrays.
        Fill them (e.g. as the output of the all-to-all-v) and hand them to ``import_runs``: no device copy is made."""
        t = self.torch
        pr, pt = C.c_void_p(), C.c_void_p()
        self._call('otto_covis_import_reserve', int(n_recs), C.byref(pr), C.byref(pt))

        def wrap(ptr):
            if not ptr or n_recs == 0:
                return None
            holder = type('_DevPtr', (), {'__cuda_array_interface__': {'shape': (int(n_recs),), 'typestr': '<i4',
                                                                       'data': (int(ptr), False), 'version': 2}})()
            return t.as_tensor(holder, device=self.device)
        return wrap(pr.value), wrap(pt.value)

    def import_runs(self, hdr, rec, tw=None):
        self._call('otto_covis_import_runs', hdr, hdr.shape[0], rec, tw, rec.numel())


def topk_to_rows(y, w, n):
    """Dense device top-k -> host rows (aid_x, aid_y, W) in (aid_x asc, rank asc) order (SPEC-COVIS 9)."""
    import torch
    k = y.shape[1]
    valid = torch.arange(k, device=y.device)[None, :] < n[:, None]
    aid_x = torch.arange(y.shape[0], device=y.device, dtype=torch.int32)[:, None].expand(-1, k)[valid]
    # (views, not astype: the values are non-negative, and a same-width astype is one more host pass over ~16 bytes per row --
    # 7 GB for the 14 row sets of a full-size build)
    def host(t, dt):
        a = t.cpu().numpy()
        return a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt)
    return host(aid_x, np.uint32), host(y[valid], np.uint32), host(w[valid], np.uint64)


def topk_to_device_rows(y, w, n):
    """The selection of :func:`topk_to_rows` with the three columns left on the device, as the part files store them:
    ``aid_x int32, aid_y int32, wgt float32``. ``wgt`` is bit-equal to the host chain ``(W.astype(float64) / Q16)
    .astype(float32)``: a division by a power of two, and both conversions round to nearest."""
    import torch
    from .spec import Q16
    k = y.shape[1]
    valid = torch.arange(k, device=y.device)[None, :] < n[:, None]
    aid_x = torch.arange(y.shape[0], device=y.device, dtype=torch.int32)[:, None].expand(-1, k)[valid]
    return aid_x, y[valid].to(torch.int32), (w[valid].double() / Q16).float()
