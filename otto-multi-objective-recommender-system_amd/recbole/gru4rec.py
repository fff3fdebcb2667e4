"""GRU4Rec, the sequential model of the reference's RecBole branch (``src/recbole/trainer.py:8-9,38``,
``src/recbole/inference.py:58-72``), trained and scored on the device (SPEC-GRU4REC, ``include/otto_gru.h``, DESIGN.md section
2k): prefix samples in a keyed epoch order, one BPR negative per sample, back-propagation through time, Adam on the weights
and on the item rows a batch touches, exact-f32 full-sort top-k through ``matrix_factorization.engine.score_topk``.

RecBole is not installed here and not vendored: the model follows RecBole 1.1.1's GRU4Rec as its published source reads, the
arithmetic is build-defined and parity with RecBole is not claimed. The parameter names (``item_embedding.weight``,
``gru_layers.weight_ih_l0``, ``gru_layers.weight_hh_l0``, ``dense.weight``, ``dense.bias``) are taken from RecBole's source as
recalled, so that a ``state_dict`` keeps its keys; they cannot be verified here. Not built, refused by name: ``loss_type: CE``,
``dropout_prob`` other than 0, ``num_layers`` above 1, several GPUs, loading a RecBole ``.pth``.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..matrix_factorization.engine import score_topk

MAX_LEN = 50                                 # OTTO_GRU_MAX_LEN, RecBole's MAX_ITEM_LIST_LENGTH
TILE = 16                                    # OTTO_GRU_TILE
CHUNK = 2048                                 # OTTO_GRU_CHUNK
MAX_BATCH = 1 << 20                          # OTTO_GRU_MAX_BATCH
EMBEDDING_SIZES = (32, 64)
HIDDEN_SIZES = (32, 64, 128)
DENSE = ('gru_layers.weight_ih_l0', 'gru_layers.weight_hh_l0', 'dense.weight', 'dense.bias')


@dataclass
class Plan:
    """The samples of one epoch in SPEC order, int32 [N] each on the device: event index ``p``, input sequence
    ``aid[seq_lo : seq_lo + seq_len]``, ``target`` and ``neg`` (aids, not rows)."""
    p: object
    seq_lo: object
    seq_len: object
    target: object
    neg: object

    def __len__(self):
        return int(self.p.numel())


@dataclass
class Grads:
    """What ``otto_gru_grad`` wrote: the dense gradients under ``DENSE``, the item gradient as ``ids`` int32 [cap] (rows of the
    item table, ascending) / ``rows`` float32 [cap, De] / ``count`` int64 [1] on the device, ``loss_sum`` float64 [1], ``o``."""
    dense: dict
    ids: object
    rows: object
    count: object
    loss_sum: object
    o: object = None


def check_sizes(embedding_size, hidden_size):
    if int(embedding_size) not in EMBEDDING_SIZES:
        raise ValueError(f'embedding_size = {embedding_size} is not built (only {EMBEDDING_SIZES})')
    if int(hidden_size) not in HIDDEN_SIZES:
        raise ValueError(f'hidden_size = {hidden_size} is not built (only {HIDDEN_SIZES})')


def check_max_len(max_len):
    if not 1 <= int(max_len) <= MAX_LEN:
        raise ValueError(f'max_len must be in [1, {MAX_LEN}] (got {max_len})')
    return int(max_len)


def _scratch(job, grad, dev, work):
    need = int(_lib.lib().otto_gru_workspace(C.byref(job), int(grad)))
    if need < 0:
        _lib.check(need, 'otto_gru_workspace')
    if work is None:
        work = _lib.workspace(need, dev)
    elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
        raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
    job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
    return work


class GRU4Rec(nn.Module):

    def __init__(self, n_aids, embedding_size=64, hidden_size=128, num_layers=1, dropout_prob=0.0, loss_type='BPR'):
        super().__init__()
        check_sizes(embedding_size, hidden_size)
        if int(num_layers) != 1:
            raise ValueError(f'num_layers = {num_layers} is not built (only 1)')
        if float(dropout_prob) != 0.0:
            raise ValueError(f'dropout_prob = {dropout_prob} is not built (only 0)')
        if loss_type != 'BPR':
            raise ValueError(f'loss_type = {loss_type!r} is not built (only BPR)')
        if not 1 <= int(n_aids) < (1 << 31) - 1:
            raise ValueError(f'n_aids must be in [1, 2^31 - 1) (got {n_aids})')
        self.n_aids, self.embedding_size, self.hidden_size = int(n_aids), int(embedding_size), int(hidden_size)
        self.item_embedding = nn.Embedding(self.n_aids + 1, self.embedding_size, padding_idx=0)
        self.gru_layers = nn.GRU(self.embedding_size, self.hidden_size, num_layers=1, bias=False, batch_first=True)
        self.dense = nn.Linear(self.hidden_size, self.embedding_size)
        # RecBole's _init_weights: xavier_normal_ on the table (PAD zeroed again), xavier_uniform_ on the GRU weights
        nn.init.xavier_normal_(self.item_embedding.weight)
        with torch.no_grad():
            self.item_embedding.weight[0].zero_()
        nn.init.xavier_uniform_(self.gru_layers.weight_ih_l0)
        nn.init.xavier_uniform_(self.gru_layers.weight_hh_l0)
        self.step_count = 0                  # Adam's global step
        self._moments = None

    @classmethod
    def from_recbole_checkpoint(cls, path):
        raise ValueError('loading a RecBole .pth is not built: RecBole is not installed and its checkpoint layout cannot be checked')

    # ---- tensors
    def tensors(self):
        """(E, W_ih, W_hh, W_d, b_d) as they live on the device"""
        t = (self.item_embedding.weight.data, self.gru_layers.weight_ih_l0.data, self.gru_layers.weight_hh_l0.data,
             self.dense.weight.data, self.dense.bias.data)
        dev = t[0].device
        if dev.type != 'cuda':
            raise _lib.OttoError('GRU4Rec needs its parameters on a ROCm device (no CPU fallback)')
        for x in t:
            _lib.need(x, 'parameter', torch.float32, device=dev)
        return t

    def moments(self):
        """Adam's (m, v) of the five tensors, zero at the first step"""
        t = self.tensors()
        if self._moments is None or self._moments[0][0].device != t[0].device:
            self._moments = ([torch.zeros_like(x) for x in t], [torch.zeros_like(x) for x in t])
        return self._moments

    def _job(self, aid, seq_lo, seq_len, max_len):
        E, W_ih, W_hh, W_d, b_d = self.tensors()
        dev = E.device
        B = int(seq_lo.numel())
        if B > MAX_BATCH:
            raise ValueError(f'a batch holds at most {MAX_BATCH} sequences (got {B})')
        _lib.need(aid, 'aid', torch.int32, 1, device=dev)
        _lib.need(seq_lo, 'seq_lo', torch.int32, 1, device=dev)
        _lib.need(seq_len, 'seq_len', torch.int32, 1, device=dev, numel=B)
        job = _lib.GruJob()
        job.d_E, job.d_W_ih, job.d_W_hh, job.d_W_d, job.d_b_d = (_lib.ptr(x, dev) for x in (E, W_ih, W_hh, W_d, b_d))
        job.n_aids, job.De, job.H = self.n_aids, self.embedding_size, self.hidden_size
        job.d_aid, job.n_events = _lib.ptr(aid, dev), int(aid.numel())
        job.d_seq_lo, job.d_seq_len, job.B, job.max_len = _lib.ptr(seq_lo, dev), _lib.ptr(seq_len, dev), B, check_max_len(max_len)
        job.stream = _lib.stream(dev)
        return job, dev, B

    # ---- the four calls
    def plan_epoch(self, events, seed, epoch, max_len=MAX_LEN, work=None):
        """SPEC SAMPLES + EPOCH ORDER + negatives of ``events`` (``aid`` int32 [E], ``sess_off`` int64 [S + 1] on the device).
        ``OttoError`` naming the first broken offset or the first event whose aid lies outside ``[0, n_aids)``."""
        aid, sess_off = events.aid, events.sess_off
        dev = self.tensors()[0].device
        _lib.need(aid, 'aid', torch.int32, 1, device=dev)
        _lib.need(sess_off, 'sess_off', torch.int64, 1, device=dev)
        if sess_off.numel() < 1:
            raise ValueError('sess_off: at least one offset')
        E, S = int(aid.numel()), int(sess_off.numel()) - 1
        with torch.cuda.device(dev):
            out = [torch.empty(E, dtype=torch.int32, device=dev) for _ in range(5)]
            job = _lib.GruPlanJob(_lib.ptr(aid, dev), _lib.ptr(sess_off, dev), E, S, self.n_aids, check_max_len(max_len), 0,
                                  int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), *(_lib.ptr(x, dev) for x in out), None, 0,
                                  _lib.stream(dev))
            need = int(_lib.lib().otto_gru_plan_workspace(C.byref(job)))
            if need < 0:
                _lib.check(need, 'otto_gru_plan_workspace')
            if work is None:
                work = _lib.workspace(need, dev)
            elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
                raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
            job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
            n, err = np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.int64)
            try:
                _lib.call('otto_gru_plan', dev, C.byref(job), n, err, stream=False)
            except _lib.OttoError as e:
                if err[0] < 0:
                    raise
                what = f'sess_off[{int(err[0])}] breaks the offsets' if err[1] == 1 else \
                    f'event {int(err[0])}: aid outside [0, {self.n_aids})'
                e = _lib.OttoError(f'gru4rec.plan_epoch: {what}')
                e.index, e.kind = int(err[0]), int(err[1])
                raise e from None
        return Plan(*(x[:int(n[0])] for x in out))

    def encode(self, aid, seq_lo, seq_len, max_len=MAX_LEN, out=None, work=None):
        """The forward pass: ``o`` float32 [B, De] = dense(h_T) of the sequences ``aid[seq_lo : seq_lo + seq_len]``."""
        job, dev, B = self._job(aid, seq_lo, seq_len, max_len)
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty((B, self.embedding_size), dtype=torch.float32, device=dev)
            _lib.need(out, 'out', torch.float32, 2, device=dev, numel=B * self.embedding_size)
            job.d_o = _lib.ptr(out, dev)
            work = _scratch(job, False, dev, work)
            _lib.call('otto_gru_encode', dev, C.byref(job), stream=False)
        return out

    def grad(self, aid, seq_lo, seq_len, target, neg, max_len=MAX_LEN, want_o=False, work=None, out=None):
        """Forward, BPR loss and back-propagation through time of one batch -> :class:`Grads` (gradients of the batch mean).
        ``out``: a :class:`Grads` of an earlier call with the same batch size, written again."""
        job, dev, B = self._job(aid, seq_lo, seq_len, max_len)
        _lib.need(target, 'target', torch.int32, 1, device=dev, numel=B)
        _lib.need(neg, 'neg', torch.int32, 1, device=dev, numel=B)
        De, H = self.embedding_size, self.hidden_size
        cap = max(1, min(B * (job.max_len + 2), self.n_aids))
        with torch.cuda.device(dev):
            if out is None:
                f32 = dict(dtype=torch.float32, device=dev)
                out = Grads({DENSE[0]: torch.empty((3 * H, De), **f32), DENSE[1]: torch.empty((3 * H, H), **f32),
                             DENSE[2]: torch.empty((De, H), **f32), DENSE[3]: torch.empty(De, **f32)},
                            torch.empty(cap, dtype=torch.int32, device=dev), torch.empty((cap, De), **f32),
                            torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev),
                            torch.empty((B, De), **f32) if want_o else None)
            elif out.ids.numel() < cap or (want_o and (out.o is None or out.o.shape[0] != B)):
                raise ValueError('out: made for another batch size')
            job.d_target, job.d_neg = _lib.ptr(target, dev), _lib.ptr(neg, dev)
            job.d_o = _lib.ptr(out.o if want_o else None, dev)
            job.d_gW_ih, job.d_gW_hh, job.d_gW_d, job.d_gb_d = (_lib.ptr(out.dense[k], dev) for k in DENSE)
            job.d_ids, job.d_rows, job.cap = _lib.ptr(out.ids, dev), _lib.ptr(out.rows, dev), int(out.ids.numel())
            job.d_count, job.d_loss_sum = _lib.ptr(out.count, dev), _lib.ptr(out.loss_sum, dev)
            work = _scratch(job, True, dev, work)
            _lib.call('otto_gru_grad', dev, C.byref(job), stream=False)
        return out

    def apply(self, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, t=None):
        """SPEC UPDATE with the gradients of :meth:`grad`; ``t``: the 1-based global step (default: the model's own count,
        which this call advances). No host synchronisation: the list's length is read on the device."""
        E, W_ih, W_hh, W_d, b_d = self.tensors()
        dev = E.device
        m, v = self.moments()
        if t is None:
            self.step_count += 1
            t = self.step_count
        if int(t) < 1:
            raise ValueError('t is the 1-based step')
        job = _lib.GruApplyJob()
        job.d_E, job.d_mE, job.d_vE = _lib.ptr(E, dev), _lib.ptr(m[0], dev), _lib.ptr(v[0], dev)
        job.n_aids, job.De, job.H = self.n_aids, self.embedding_size, self.hidden_size
        for q, (p, key) in enumerate(zip((W_ih, W_hh, W_d, b_d), DENSE)):
            g = _lib.need(grads.dense[key], key, torch.float32, device=dev, numel=p.numel())
            job.d_W[q], job.d_m[q], job.d_v[q], job.d_g[q] = (x.data_ptr() for x in (p, m[q + 1], v[q + 1], g))
        _lib.need(grads.ids, 'ids', torch.int32, 1, device=dev)
        _lib.need(grads.rows, 'rows', torch.float32, 2, device=dev, numel=grads.ids.numel() * self.embedding_size)
        _lib.need(grads.count, 'count', torch.int64, 1, device=dev, numel=1)
        job.d_ids, job.d_rows, job.cap, job.d_count = _lib.ptr(grads.ids, dev), _lib.ptr(grads.rows, dev), int(grads.ids.numel()), \
            _lib.ptr(grads.count, dev)
        job.lr, job.beta1, job.beta2, job.eps, job.t = float(lr), float(betas[0]), float(betas[1]), float(eps), int(t)
        job.stream = _lib.stream(dev)
        _lib.call('otto_gru_apply', dev, C.byref(job), stream=False)

    # ---- inference
    def encode_sessions(self, events, max_len=MAX_LEN, sessions_per_launch=1 << 16):
        """``o`` float32 [S, De] of the last ``max_len`` aids of every session (an empty session encodes to ``dense.bias``)."""
        max_len = check_max_len(max_len)
        off = events.sess_off
        lo = torch.maximum(off[:-1], off[1:] - max_len)
        seq_lo, seq_len = lo.to(torch.int32), (off[1:] - lo).to(torch.int32)
        S = int(seq_lo.numel())
        out = torch.empty((S, self.embedding_size), dtype=torch.float32, device=off.device)
        for a in range(0, S, int(sessions_per_launch)):
            b = min(S, a + int(sessions_per_launch))
            self.encode(events.aid, seq_lo[a:b].contiguous(), seq_len[a:b].contiguous(), max_len, out=out[a:b])
        return out

    def full_sort_topk(self, o, k=20):
        """Top-k rows of the item table by ``<o, E[row]>`` over ALL items, PAD excluded (``src/recbole/inference.py:76-80``):
        ``(rows int32 [B, k], scores float32 [B, k])``; aid = row - 1."""
        return score_topk(o, self.item_embedding.weight.data, k=k, pad_col=0)


def train_epoch(model, events, batch=2048, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=42, epoch=0, max_len=MAX_LEN, steps=None):
    """One pass over the prefix samples of ``events`` in SPEC's epoch order (or its first ``steps`` batches); returns the mean
    loss, read once at the end. A corpus without a sample trains nothing and returns 0."""
    batch = int(batch)
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError(f'batch must be in [1, {MAX_BATCH}] (got {batch})')
    plan = model.plan_epoch(events, seed, epoch, max_len)
    n = len(plan)
    n_batches = -(-n // batch)
    if steps is not None:
        n_batches = min(n_batches, int(steps))
    if n_batches == 0:
        return 0.0
    dev = plan.p.device
    losses = torch.zeros(n_batches, dtype=torch.float64, device=dev)
    seen = 0
    full = None
    for q in range(n_batches):
        a, b = q * batch, min(n, (q + 1) * batch)
        g = model.grad(events.aid, plan.seq_lo[a:b], plan.seq_len[a:b], plan.target[a:b], plan.neg[a:b], max_len,
                       out=full if b - a == batch else None)
        if b - a == batch:
            full = g                         # every full batch writes the same buffers
        model.apply(g, lr, betas, eps)
        losses[q] = g.loss_sum[0]
        seen += b - a
    return float(losses.sum().item()) / seen
