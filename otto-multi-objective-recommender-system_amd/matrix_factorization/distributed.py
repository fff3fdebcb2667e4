"""Exact data-parallel SparseAdam for the R-MF trainer (``torch_trainer.train()`` + ``SparseAdam`` + ``StepLR``).

One process per GPU. The result of every step equals one process running ``otto_mf_step_sparse_adam`` on the union of
the ranks' batches (to fp32 summation order):

* :class:`ShardedBatchLoader` gives rank ``r`` the rows of sessions ``[lo_r, hi_r)`` (``MatrixFactorization``: cuts
  contiguous in session id, balanced by row count) or the row range ``[r N / W, (r + 1) N / W)``
  (``CollaborativeFiltering``). Every rank runs ``n_steps = ceil(N / batch_size)`` steps per epoch; its batch ``k`` is
  rows ``[k n_r // n_steps, (k + 1) n_r // n_steps)`` of its own shuffled shard, possibly empty. ``B_global(k)``, the
  loss divisor, follows from the shard sizes, so no step needs a collective for it.
* :class:`DataParallelSparseAdam` runs per step the local half (``otto_mf_dp_local``: private session rows updated in
  place, the coalesced aid-gradient rows written to a padded export list), one all-gather of the export lists, and the
  apply half (``otto_mf_dp_apply``: rows summed in rank order, Adam once per row). Every rank keeps full-size tables; the
  session table is private (a rank reads and writes only its own rows), the aid table and its moments are replicated
  and stay bit-identical.
* :func:`full_state_dict` gathers every rank's session rows for a checkpoint with the reference's keys and shapes.

Collectives go through ``torch.distributed``; with a gloo group device tensors are staged through host buffers.
"""
import numpy as np
import torch
import torch.distributed as dist

from .data import _BatchLoader
from .torch_optim import SparseAdam, loss_kind


def _world(group):
    return (dist.get_rank(group), dist.get_world_size(group)) if dist.is_available() and dist.is_initialized() else (0, 1)


def _stage(group, stage_device):
    """'cpu' when collectives must be staged through host buffers (gloo, or asked for); None otherwise."""
    if stage_device not in (None, 'auto', 'cpu'):
        raise ValueError(f"stage_device must be None, 'auto' or 'cpu' (got {stage_device!r})")
    if stage_device == 'cpu':
        return 'cpu'
    if dist.is_available() and dist.is_initialized() and dist.get_backend(group) == 'gloo':
        return 'cpu'
    return None


def _coll_device(group):
    """Where a small host value travels for a collective: the current GPU for nccl, the host otherwise."""
    if dist.get_backend(group) == 'nccl':
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device('cpu')


def _all_reduce(t, op, group, stage):
    """In place; ``t`` may live on the device while the group only carries host tensors, or on the host while it only
    carries device tensors."""
    dev = torch.device('cpu') if stage else _coll_device(group)
    if t.device != dev:
        h = t.to(dev)
        dist.all_reduce(h, op=op, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op, group=group)
    return t


def _all_gather(out, t, group, stage):
    """``out`` [W, *t.shape] receives every rank's ``t`` (same shape on every rank)."""
    dev = torch.device('cpu') if stage else _coll_device(group)
    if t.device != dev or out.device != dev:
        h = torch.empty(out.shape, dtype=out.dtype, device=dev)
        _all_gather(h, t.to(dev), group, stage)
        out.copy_(h)
    elif dist.get_backend(group) == 'nccl':
        dist.all_gather_into_tensor(out.view(-1), t.reshape(-1), group=group)
    else:
        dist.all_gather(list(out.unbind(0)), t, group=group)
    return out


def _global_rank(group, r):
    return r if group is None else dist.get_global_rank(group, r)


# ---------------------------------------------------------------------------------------------------------------------
# shard and schedule arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def session_cuts(sessions, world, n_sessions=None):
    """Cuts ``c[0] = 0 <= c[1] <= ... <= c[W] = n_sessions``: rank ``r`` owns sessions ``[c[r], c[r + 1])``. Contiguous in
    session id; ``c[r]`` is the smallest session id with at least ``r N // W`` rows below it (rows balanced to within one
    session). Integer arithmetic only, so every rank computes the same cuts from the same column."""
    s = torch.as_tensor(sessions).reshape(-1)
    n = s.numel()
    top = int(s.max()) + 1 if n else 0
    n_sessions = top if n_sessions is None else int(n_sessions)
    if top > n_sessions or (n and int(s.min()) < 0):
        raise ValueError(f'session ids outside [0, {n_sessions})')
    prefix = torch.zeros(n_sessions + 1, dtype=torch.int64, device=s.device)
    if n:
        torch.cumsum(torch.bincount(s, minlength=n_sessions), 0, out=prefix[1:])
    targets = torch.tensor([(r * n) // world for r in range(world + 1)], dtype=torch.int64, device=s.device)
    cuts = torch.searchsorted(prefix, targets, side='left').cpu().tolist()
    cuts[0], cuts[world] = 0, n_sessions
    return cuts, [int(prefix[cuts[r + 1]]) - int(prefix[cuts[r]]) for r in range(world)]


def row_cuts(n, world):
    """Contiguous equal row ranges of the shared-table model: rank ``r`` owns rows ``[r n // W, (r + 1) n // W)``."""
    return [(r * n) // world for r in range(world + 1)]


def n_steps(n_total, batch_size):
    """Steps per epoch: the single-process loader's count, ``ceil(N / batch_size)``."""
    return (int(n_total) + int(batch_size) - 1) // int(batch_size)


def local_batch_bounds(k, n_local, steps):
    """Rows ``[lo, hi)`` of a rank's shuffled shard that form its batch ``k`` (possibly empty)."""
    return (k * n_local) // steps, ((k + 1) * n_local) // steps


def global_batch_sizes(sizes, steps):
    """``B_global(k) = sum_r |batch_r(k)|`` for k = 0 .. steps - 1 (int64 array, sums to ``sum(sizes)``)."""
    k = np.arange(steps + 1, dtype=np.int64)
    return sum(np.diff((k * int(n)) // steps) for n in sizes) if steps else np.zeros(0, np.int64)


class ShardedBatchLoader(_BatchLoader):
    """Rank ``rank``'s part of the data-parallel epoch: same ``(dict_of_int64_device_tensors, None)`` batches as
    :class:`~.data.DeviceBatchLoader`, ``len()`` = ``n_steps`` on every rank.

    ``columns`` are the FULL columns (every rank reads the same file); ``shard_key`` = ``'session'`` shards by session
    (``MatrixFactorization``; ``n_keys`` = the session table's row count, defaults to the largest id + 1), ``None`` by
    row range (``CollaborativeFiltering``). ``rank`` / ``world`` default to the process group's. With an initialised
    process group the shard sizes are all-gathered once, here, and checked against the local computation (ranks that
    read different data fail now instead of diverging)."""

    def __init__(self, columns, batch_size, shard_key='session', n_keys=None, shuffle=True, device='cuda:0', seed=None,
                 rank=None, world=None, group=None, stage_device=None):
        g_rank, g_world = _world(group)
        self.rank = g_rank if rank is None else int(rank)
        self.world = g_world if world is None else int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f'rank {self.rank} outside world {self.world}')
        self.group, self.stage = group, _stage(group, stage_device)
        super().__init__(columns, shuffle, device, None if seed is None else int(seed) * 1000003 + self.rank)
        self.n_total = self.n
        self.batch_size, self.shard_key = int(batch_size), shard_key
        if shard_key is None:
            self.cuts = row_cuts(self.n_total, self.world)
            self.sizes = [self.cuts[r + 1] - self.cuts[r] for r in range(self.world)]
            lo, hi = self.cuts[self.rank], self.cuts[self.rank + 1]
            self.columns = {k: v[lo:hi].contiguous() for k, v in self.columns.items()}
            self.private_rows = None
        else:
            self.cuts, self.sizes = session_cuts(self.columns[shard_key], self.world, n_keys)
            lo, hi = self.cuts[self.rank], self.cuts[self.rank + 1]
            key = self.columns[shard_key]
            keep = torch.nonzero((key >= lo) & (key < hi)).reshape(-1)
            self.columns = {k: v[keep].contiguous() for k, v in self.columns.items()}
            self.private_rows = (lo, hi)
        self.n = next(iter(self.columns.values())).numel()
        assert self.n == self.sizes[self.rank]
        if rank is None and world is None and self.world > 1:
            got = torch.zeros((self.world, 1), dtype=torch.int64)
            _all_gather(got, torch.tensor([self.n], dtype=torch.int64), group, self.stage)
            if got.reshape(-1).tolist() != self.sizes:
                raise ValueError(f'ranks disagree on the shard sizes: gathered {got.reshape(-1).tolist()}, '
                                 f'computed {self.sizes} (every rank must read the same data)')
        self.n_steps = n_steps(self.n_total, self.batch_size)
        self.global_sizes = global_batch_sizes(self.sizes, self.n_steps)
        self.max_local_batch = max(((n + self.n_steps - 1) // self.n_steps if self.n_steps else 0) for n in self.sizes)

    def batch_global(self, k):
        return int(self.global_sizes[k])

    def __len__(self):
        return self.n_steps

    def _batch_bounds(self):
        return (local_batch_bounds(k, self.n, self.n_steps) for k in range(self.n_steps))


# ---------------------------------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------------------------------
class DataParallelSparseAdam(SparseAdam):
    """:class:`~.torch_optim.SparseAdam` (same constructor, state layout and ``fused_step`` signature) whose step is the
    synchronous data-parallel step over ``group``. ``stage_device``: ``'cpu'`` stages the exchange through host buffers
    (automatic for a gloo group). The exchange buffers are allocated once (``cap`` = the largest local batch, twice that
    for a shared table) and reused; nothing table-sized is allocated."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False, group=None, stage_device=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, maximize=maximize)
        self.group = group
        self.rank, self.world = _world(group)
        self.stage = _stage(group, stage_device)
        self._buf = None

    def _agree(self, value, op):
        t = torch.tensor([int(value)], dtype=torch.int64)
        if self.world > 1:
            _all_reduce(t, op, self.group, self.stage)
        return int(t.item())

    def _buffers(self, cap, d, device):
        b = self._buf
        if b is None or b['cap'] < cap or b['d'] != d or b['device'] != device:
            cap = max(int(cap), 1)
            W = self.world
            b = dict(cap=cap, d=d, device=device,
                     ids=torch.zeros(cap, dtype=torch.int32, device=device),
                     rows=torch.zeros((cap, d), dtype=torch.float32, device=device),
                     count=torch.zeros(1, dtype=torch.int64, device=device),
                     g_ids=torch.empty((W, cap), dtype=torch.int32, device=device),
                     g_rows=torch.empty((W, cap, d), dtype=torch.float32, device=device),
                     g_count=torch.empty((W, 1), dtype=torch.int64, device=device))
            self._buf = b
        return b

    def exchange(self, b):
        """All-gather of the padded export lists (ids, rows, count) into the ``g_*`` buffers."""
        if self.world == 1 and not dist.is_initialized():
            b['g_ids'][0].copy_(b['ids'])
            b['g_rows'][0].copy_(b['rows'])
            b['g_count'][0].copy_(b['count'])
            return
        _all_gather(b['g_count'], b['count'], self.group, self.stage)
        _all_gather(b['g_ids'], b['ids'], self.group, self.stage)
        _all_gather(b['g_rows'], b['rows'], self.group, self.stage)

    def fused_step(self, model, i1, i2, targets, criterion, loss_out, batch_global=None, private_rows=None,
                   max_local_batch=None):
        """One global step. ``loss_out`` receives this rank's loss sum / ``batch_global``: the ranks' values add up to the
        global batch's mean loss. ``batch_global`` / ``max_local_batch`` come from :class:`ShardedBatchLoader`
        (``train()`` passes them); without them they are agreed by an all-reduce in this step. ``private_rows`` =
        the session rows ``[lo, hi)`` this rank owns (default: the whole table; ignored for a shared table)."""
        group = self.param_groups[0]
        E1, E2, shared, s1, s2 = self._begin_step(model)
        B = i1.numel()
        if batch_global is None:
            batch_global = self._agree(B, dist.ReduceOp.SUM) if self.world > 1 else B
        if max_local_batch is None:
            max_local_batch = self._agree(B, dist.ReduceOp.MAX) if self.world > 1 else B
        if B > max_local_batch or batch_global < B:
            raise ValueError(f'local batch {B} exceeds max_local_batch {max_local_batch} or batch_global {batch_global}')
        eng = model.engine(max(int(max_local_batch), 1))
        b = self._buffers(max(int(max_local_batch), 1) * (2 if shared else 1), E2.shape[1], E2.device)
        lo, hi = (0, E1.shape[0]) if private_rows is None else private_rows
        lr, betas, eps = group['lr'], group['betas'], group['eps']
        eng.dp_local(E1.data, None if shared else s1['exp_avg'], None if shared else s1['exp_avg_sq'], E2.data, i1, i2,
                     targets, max(int(batch_global), 1), lo, hi, loss_kind(criterion), lr, betas, eps, s1['step'],
                     b['ids'], b['rows'], b['count'], loss_out)
        self.exchange(b)
        eng.dp_apply(E2.data, s2['exp_avg'], s2['exp_avg_sq'], b['g_ids'], b['g_rows'], b['g_count'].reshape(-1),
                     lr, betas, eps, s2['step'])

    def all_reduce_sum(self, values):
        """Sum over ranks of a float64 host array (one collective): the per-epoch loss combination of ``train()``."""
        t = torch.as_tensor(np.asarray(values, dtype=np.float64))
        if self.world > 1:
            _all_reduce(t, dist.ReduceOp.SUM, self.group, self.stage)
        return t.numpy()


def full_state_dict(model, loader, group=None):
    """``model.state_dict()`` with every session row current: rank ``r`` broadcasts its rows ``[lo_r, hi_r)`` (one
    broadcast per rank, at checkpoint time only) into every rank's table, so rank 0 can ``torch.save`` a checkpoint with
    the reference's keys and shapes. Rows received here are copies: this rank never trains them. The shared-table model
    has no private rows and returns its ``state_dict()`` unchanged."""
    E1, _, shared = model._tables()
    rank, world = _world(group)
    if not shared and world > 1 and loader.private_rows is not None:
        stage = _stage(group, getattr(loader, 'stage', None))
        for r in range(world):
            lo, hi = loader.cuts[r], loader.cuts[r + 1]
            if hi <= lo:
                continue
            view = E1.data[lo:hi]
            dev = torch.device('cpu') if stage else _coll_device(group)
            if view.device != dev:
                h = view.to(dev)
                dist.broadcast(h, src=_global_rank(group, r), group=group)
                if r != rank:
                    view.copy_(h)
            else:
                dist.broadcast(view, src=_global_rank(group, r), group=group)
    return model.state_dict()
