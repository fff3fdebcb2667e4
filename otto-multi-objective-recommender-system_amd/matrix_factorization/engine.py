"""Device engine of the MF path: thin Python over ``include/otto_mf.h``.
torch owns the embedding tables / optimizer state and the stream; every
arithmetic step runs in hand-written gfx950 kernels (``csrc/otto_mf.hip``)."""
import ctypes as C

from .. import _lib

LOSS_MSE, LOSS_BCE = 0, 1
BPR_HOGWILD, BPR_BATCH = 0, 1


class MFEngine:
    """Workspace (row-owner words, gradient slots) for one pair of embedding tables."""

    def __init__(self, n1, n2, d, max_batch, shared_table=False, device='cuda:0'):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.OttoError('MFEngine needs a ROCm device (no CPU fallback)')
        self.n1, self.n2, self.d = int(n1), int(n1 if shared_table else n2), int(d)
        self.max_batch, self.shared = int(max_batch), bool(shared_table)
        self._lib = _lib.lib()                    # close() may run while the interpreter shuts down
        self._ctx = C.c_void_p()
        _lib.call('otto_mf_create', self.device, C.byref(self._ctx), self.n1, self.n2, self.d, self.max_batch, int(self.shared),
                  stream=False)

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx:
            self._lib.otto_mf_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _call(self, name, *args):
        _lib.call(name, self.device, self._ctx, *args)

    def _tables(self, E1, E2):
        t = self.torch
        _lib.need(E1, 'E1', t.float32, device=self.device)
        _lib.need(E2, 'E2', t.float32, device=self.device)
        if E1.shape != (self.n1, self.d) or E2.shape != (self.n2, self.d):
            raise ValueError(f'table shapes {tuple(E1.shape)}, {tuple(E2.shape)} != ({self.n1},{self.d}), ({self.n2},{self.d})')

    def _idx(self, i1, i2, extra=()):
        t = self.torch
        for n, x in (('i1', i1), ('i2', i2)) + tuple(extra):
            _lib.need(x, n, t.int64, device=self.device)
        if i1.numel() != i2.numel() or any(x.numel() != i1.numel() for _, x in extra):
            raise ValueError('index / target length mismatch')
        return i1.numel()

    def forward(self, E1, E2, i1, i2, out=None):
        """out[b] = <E1[i1[b]], E2[i2[b]]>  (torch_modules.py:13-19, 32-38)."""
        t = self.torch
        self._tables(E1, E2)
        B = self._idx(i1, i2)
        if out is None:
            out = t.empty(B, dtype=t.float32, device=self.device)
        self._call('otto_mf_forward', E1, E2, i1, i2, B, out)
        return out

    def eval(self, E1, E2, i1, i2, target, loss_kind, loss_out, pred=None):
        """validate() batch body: mean loss into ``loss_out`` (1-element device view), optional predictions."""
        self._tables(E1, E2)
        B = self._idx(i1, i2, (('target', target),))
        self._call('otto_mf_eval', E1, E2, i1, i2, target, B, int(loss_kind), pred, loss_out)

    def eval_sums(self, E1, E2, i1, i2, target, loss_kind, loss_out, pred=None):
        """``eval`` + the context's running score sums (sum |p - t|, sum (p - t)^2, hits at 0.5, count) grow by this batch:
        validate() reads four doubles per epoch instead of every prediction (torch_trainer.py:144-158)."""
        self._tables(E1, E2)
        B = self._idx(i1, i2, (('target', target),))
        self._call('otto_mf_eval_sums', E1, E2, i1, i2, target, B, int(loss_kind), pred, loss_out)

    def read_sums(self, reset=True):
        """(sum |p - t|, sum (p - t)^2, hits, count) accumulated by ``eval_sums``; synchronises."""
        buf = (C.c_double * 4)()
        self._call('otto_mf_read_sums', buf, int(reset))
        return tuple(float(v) for v in buf)

    def check(self):
        """Raise ``OttoError`` if any kernel since the last call skipped a sample whose row id was outside its table
        (the kernels range-check instead of faulting; ``nn.Embedding`` would raise IndexError in the reference)."""
        self._call('otto_mf_check', None)

    def step_sparse_adam(self, E1, m1, v1, E2, m2, v2, i1, i2, target, loss_kind, lr, betas, eps, t_step, loss_out):
        """train() batch body with SparseAdam semantics; mean pre-update loss into ``loss_out``."""
        self._tables(E1, E2)
        B = self._idx(i1, i2, (('target', target),))
        self._call('otto_mf_step_sparse_adam', E1, m1, v1, E2, m2, v2, i1, i2, target, B, int(loss_kind), float(lr),
                   float(betas[0]), float(betas[1]), float(eps), int(t_step), loss_out)

    def dp_local(self, E1, m1, v1, E2, i1, i2, target, batch_global, priv_lo, priv_hi, loss_kind, lr, betas, eps, t_step,
                 ids, rows, count, loss_out):
        """Local half of the data-parallel SparseAdam step (``otto_mf_dp_local``): private rows of table 1 in
        ``[priv_lo, priv_hi)`` updated in place, the replicated rows' coalesced gradients written to the export list
        ``ids`` int32 [cap] / ``rows`` float32 [cap, d] with their number in ``count`` (int64 [1]); ``loss_out`` = local
        loss sum / ``batch_global``. A shared-table engine passes ``E1 is E2`` and no moments (``m1 = v1 = None``)."""
        t = self.torch
        self._tables(E1, E2)
        B = self._idx(i1, i2, (('target', target),))
        if not self.shared:
            _lib.need(m1, 'm1', t.float32, device=self.device)
            _lib.need(v1, 'v1', t.float32, device=self.device)
        _lib.need(ids, 'ids', t.int32, device=self.device)
        _lib.need(rows, 'rows', t.float32, device=self.device)
        _lib.need(count, 'count', t.int64, device=self.device)
        cap = ids.numel()
        if rows.shape != (cap, self.d) or count.numel() < 1 or loss_out.numel() < 1:
            raise ValueError(f'export buffers: ids [{cap}], rows {tuple(rows.shape)} != [{cap}, {self.d}]')
        self._call('otto_mf_dp_local', E1, m1, v1, E2, i1, i2, target, B, int(batch_global), int(priv_lo), int(priv_hi),
                   int(loss_kind), float(lr), float(betas[0]), float(betas[1]), float(eps), int(t_step), ids, rows, cap, count,
                   loss_out)

    def dp_apply(self, E2, m2, v2, ids, rows, counts, lr, betas, eps, t_step):
        """Apply half (``otto_mf_dp_apply``): the gathered export lists ``ids`` int32 [W, cap], ``rows`` float32
        [W, cap, d] (consumed), ``counts`` int64 [W] summed in rank order and applied with Adam to the replicated table."""
        t = self.torch
        _lib.need(E2, 'E2', t.float32, device=self.device)
        if E2.shape != (self.n2, self.d):
            raise ValueError(f'table shape {tuple(E2.shape)} != ({self.n2},{self.d})')
        for n, x, dt in (('m2', m2, t.float32), ('v2', v2, t.float32), ('ids', ids, t.int32), ('rows', rows, t.float32),
                         ('counts', counts, t.int64)):
            _lib.need(x, n, dt, device=self.device)
        if ids.dim() != 2 or rows.shape != (ids.shape[0], ids.shape[1], self.d) or counts.shape != (ids.shape[0],):
            raise ValueError(f'gathered buffers: ids {tuple(ids.shape)}, rows {tuple(rows.shape)}, counts {tuple(counts.shape)}')
        W, cap = ids.shape
        self._call('otto_mf_dp_apply', E2, m2, v2, ids, rows, counts, int(W), int(cap), float(lr), float(betas[0]),
                   float(betas[1]), float(eps), int(t_step))

    def bpr_step(self, U, V, u, i, seed, epoch, row0, lr, l2=0.0, mode=BPR_HOGWILD, loss_sum=None, neg_out=None):
        t = self.torch
        self._tables(U, V)
        B = self._idx(u, i)
        if loss_sum is None:
            loss_sum = t.empty(1, dtype=t.float32, device=self.device)
        self._call('otto_mf_bpr_step', U, V, u, i, B, int(seed), int(epoch), int(row0), float(lr), float(l2), int(mode),
                   loss_sum, neg_out)
        return loss_sum


def score_topk(U, V, k=20, pad_col=-1):
    """Full-sort scoring: top-k of U @ V.T per row without materialising it
    (recbole/inference.py:76-80). Returns (ids int32 [B,k], scores float32 [B,k])."""
    import torch
    if U.device.type != 'cuda':
        raise _lib.OttoError('score_topk needs a ROCm device (no CPU fallback)')
    for n, x in (('U', U), ('V', V)):
        _lib.need(x, n, torch.float32, device=U.device)
    B, d = U.shape
    N = V.shape[0]
    if V.shape[1] != d:
        raise ValueError('factor dimension mismatch')
    ws_bytes = _lib.lib().otto_mf_score_workspace(B, N, int(k))
    ws = _lib.workspace(ws_bytes, U.device)
    ids = torch.empty((B, k), dtype=torch.int32, device=U.device)
    scores = torch.empty((B, k), dtype=torch.float32, device=U.device)
    _lib.call('otto_mf_score_topk', U.device, U, V, B, N, int(d), int(k), int(pad_col), ids, scores, ws, ws_bytes)
    return ids, scores


def topk_merge(part_scores, part_ids, k):
    """Exact merge of W partial top-k lists per row: ``part_scores`` float32 / ``part_ids`` int32 [W, B, k] (id -1 = empty)
    -> (ids int32 [B, k], scores float32 [B, k]) ordered by (score desc, id asc). Used by the item-sharded scoring."""
    import torch
    if part_scores.device.type != 'cuda':
        raise _lib.OttoError('topk_merge needs a ROCm device (no CPU fallback)')
    _lib.need(part_scores, 'part_scores', torch.float32)
    _lib.need(part_ids, 'part_ids', torch.int32, device=part_scores.device)
    W, B, kk = part_scores.shape
    if part_ids.shape != part_scores.shape or kk != k:
        raise ValueError('partial lists must be [W, B, k]')
    ids = torch.empty((B, k), dtype=torch.int32, device=part_scores.device)
    scores = torch.empty((B, k), dtype=torch.float32, device=part_scores.device)
    _lib.call('otto_mf_topk_merge', part_scores.device, part_scores, part_ids, int(W), int(B), int(k), ids, scores)
    return ids, scores
