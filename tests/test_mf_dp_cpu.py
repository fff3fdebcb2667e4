"""CPU tests of the exact data-parallel SparseAdam trainer (otto_amd/matrix_factorization/distributed.py): the shard and
schedule arithmetic, the optimizer's exchange protocol over gloo with a NumPy stand-in engine built from the oracle, and
the trainer's ``training.distributed`` configuration checks."""
import os
import queue
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

import mf_oracle as mo


# ---------------------------------------------------------------------------------------------------------------------
# shard / schedule arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [1, 2, 3, 5])
def test_session_cuts_contiguous_and_balanced(world):
    from otto_amd.matrix_factorization.distributed import session_cuts
    rng = np.random.default_rng(world)
    n_sessions = 400
    s = np.sort(rng.integers(0, n_sessions, 5000) * (rng.random(5000) < 0.9))   # session 0 heavy, some ids absent
    cuts, sizes = session_cuts(torch.from_numpy(s), world, n_sessions)
    assert cuts[0] == 0 and cuts[-1] == n_sessions and all(a <= b for a, b in zip(cuts, cuts[1:]))
    assert sizes == [int(((s >= cuts[r]) & (s < cuts[r + 1])).sum()) for r in range(world)]
    assert sum(sizes) == len(s)
    cnt = np.bincount(s, minlength=n_sessions)
    for r in range(1, world):
        below = int(cnt[:cuts[r]].sum())
        # the cut is the first session at or past the balanced row target r N / W
        assert below >= r * len(s) // world and below - int(cnt[cuts[r] - 1]) < r * len(s) // world


def test_session_cuts_empty_shards():
    from otto_amd.matrix_factorization.distributed import session_cuts
    cuts, sizes = session_cuts(torch.tensor([3, 3, 3, 3]), 3, 10)      # one session holds every row
    assert cuts[0] == 0 and cuts[-1] == 10 and sum(sizes) == 4 and sorted(sizes) == [0, 0, 4]
    cuts, sizes = session_cuts(torch.zeros(0, dtype=torch.int64), 2, 5)
    assert cuts == [0, 0, 5] and sizes == [0, 0]


@pytest.mark.parametrize('sizes,batch', [([10, 7, 3], 4), ([1, 50], 8), ([0, 9], 2), ([5, 5, 5], 100), ([2, 0, 31], 3)])
def test_schedule_every_rank_same_steps_and_global_sizes_sum(sizes, batch):
    from otto_amd.matrix_factorization.distributed import (ShardedBatchLoader, global_batch_sizes, local_batch_bounds,
                                                             n_steps, row_cuts)
    N = sum(sizes)
    S = n_steps(N, batch)
    assert S == -(-N // batch)
    bg = global_batch_sizes(sizes, S)
    assert len(bg) == S and int(bg.sum()) == N
    for n in sizes:
        bounds = [local_batch_bounds(k, n, S) for k in range(S)]
        assert bounds[0][0] == 0 and bounds[-1][1] == n and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    assert list(bg) == [sum(local_batch_bounds(k, n, S)[1] - local_batch_bounds(k, n, S)[0] for n in sizes)
                        for k in range(S)]
    # the loaders: same len on every rank, batches partition the shard, row ranges for the shared-table model
    W = len(sizes)
    sess = np.repeat(np.arange(W), sizes)
    cols = {'session': sess, 'aid': np.arange(N), 'target': np.zeros(N, dtype=np.int64)}
    seen = []
    for r in range(W):
        ld = ShardedBatchLoader(cols, batch, shard_key='session', n_keys=W, device='cpu', seed=1, rank=r, world=W)
        assert len(ld) == S and ld.private_rows == (ld.cuts[r], ld.cuts[r + 1])
        assert ld.max_local_batch == max(-(-n // S) for n in ld.sizes)
        got = [b for b, _ in ld]
        assert len(got) == S
        rows = torch.cat([b['aid'] for b in got]).tolist()
        assert sorted(rows) == sorted(np.nonzero((sess >= ld.cuts[r]) & (sess < ld.cuts[r + 1]))[0].tolist())
        seen += rows
        rl = ShardedBatchLoader(cols, batch, shard_key=None, device='cpu', seed=1, rank=r, world=W)
        lo, hi = row_cuts(N, W)[r], row_cuts(N, W)[r + 1]
        assert rl.private_rows is None and sorted(torch.cat([b['aid'] for b, _ in rl]).tolist()) == list(range(lo, hi))
    assert sorted(seen) == list(range(N))


# ---------------------------------------------------------------------------------------------------------------------
# the optimizer's protocol over gloo, NumPy stand-in engine
# ---------------------------------------------------------------------------------------------------------------------
class OracleDPEngine:
    """CPU stand-in with the dp_local / dp_apply / check surface of MFEngine (tests only)."""

    def __init__(self, shared, max_batch):
        self.shared, self.max_batch = shared, max_batch
        self.calls = []

    def check(self):
        pass

    def dp_local(self, E1, m1, v1, E2, i1, i2, target, batch_global, priv_lo, priv_hi, kind, lr, betas, eps, t_step,
                 ids, rows, count, loss_out):
        assert ids.dtype == torch.int32 and rows.shape == (ids.numel(), E2.shape[1])
        i1, i2, tg = i1.numpy(), i2.numpy(), target.numpy()
        if not self.shared:
            assert ((i1 >= priv_lo) & (i1 < priv_hi)).all()
        e1, e2 = E1.numpy(), E2.numpy()
        out = mo.forward(e1, e2, i1, i2)
        l, g = mo.loss_and_grad('MSELoss' if kind == 0 else 'BCEWithLogitsLoss', out, tg)
        c = (g / batch_global)[:, None]
        g1, g2 = c * e2[i2].astype(np.float64), c * e1[i1].astype(np.float64)
        if self.shared:
            touched, gr = mo._coalesced(e1.shape[0], e1.shape[1], np.concatenate([i1, i2]), np.concatenate([g1, g2]))
        else:
            t1, gr1 = mo._coalesced(e1.shape[0], e1.shape[1], i1, g1)
            touched, gr = mo._coalesced(e2.shape[0], e2.shape[1], i2, g2)
            mo._adam_rows(e1, m1.numpy(), v1.numpy(), t1, gr1, lr, betas, eps, t_step)
        n = len(touched)
        assert n <= ids.numel()
        rows.fill_(float('nan'))      # padding must never be read
        ids.fill_(-7)
        ids[:n] = torch.from_numpy(touched.astype(np.int32))
        rows[:n] = torch.from_numpy(gr)
        count[0] = n
        loss_out[0] = float(l.sum() / batch_global)
        self.calls.append(len(i1))

    def dp_apply(self, E2, m2, v2, ids, rows, counts, lr, betas, eps, t_step):
        W = ids.shape[0]
        sel = [(ids[r, :int(counts[r])].numpy().astype(np.int64), rows[r, :int(counts[r])].numpy()) for r in range(W)]
        for idx, _ in sel:
            assert len(np.unique(idx)) == len(idx)
        idx = np.concatenate([s[0] for s in sel])
        if len(idx) == 0:
            return
        e2 = E2.numpy()
        touched, gr = mo._coalesced(e2.shape[0], e2.shape[1], idx, np.concatenate([s[1] for s in sel]).astype(np.float64))
        mo._adam_rows(e2, m2.numpy(), v2.numpy(), touched, gr, lr, betas, eps, t_step)


def _standin_model(shared, n1, n2, d, seed):
    from otto_amd.matrix_factorization import torch_modules as tm

    base = tm.CollaborativeFiltering if shared else tm.MatrixFactorization

    class M(base):
        def engine(self, batch):
            if self._engine is None or self._engine.max_batch < batch:
                self._engine = OracleDPEngine(shared, batch)
            return self._engine

    m = tm.CollaborativeFiltering(n1, d) if shared else tm.MatrixFactorization(n1, n2, d)
    m.__class__ = M
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    return m


BATCH = 3


def _dataset(shared, seed=5):
    rng = np.random.default_rng(seed)
    if shared:
        n = 37
        x1, x2 = rng.integers(0, 25, n), np.minimum(rng.zipf(1.5, n) - 1, 24)
        return {'x1': x1, 'x2': x2, 'target': rng.integers(0, 2, n)}, 25, 25
    # unequal sessions, one heavy session so that a rank's shard is smaller than n_steps
    sess = np.concatenate([np.zeros(2, np.int64), np.full(30, 1), rng.integers(2, 12, 9)])
    aid = np.minimum(rng.zipf(1.4, len(sess)) - 1, 14)
    return {'session': sess, 'aid': aid, 'target': rng.integers(0, 3, len(sess))}, 12, 15


def _protocol_worker(rank, world, port, shared, q):
    import traceback
    from datetime import timedelta
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
    out = None
    try:
        import torch.distributed as dist
        from otto_amd.matrix_factorization import torch_trainer as tt
        from otto_amd.matrix_factorization.distributed import (DataParallelSparseAdam, ShardedBatchLoader,
                                                                 full_state_dict)
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=timedelta(seconds=60))
        cols, n1, n2 = _dataset(shared)
        d, batch, lr = 4, BATCH, 0.05
        key = dict(shard_key=None) if shared else dict(shard_key='session', n_keys=n1)
        loader = ShardedBatchLoader(cols, batch, device='cpu', seed=3, **key)
        model = _standin_model(shared, n1, n2, d, seed=9)
        ref = [p.detach().numpy().copy() for p in model.parameters()]
        opt = DataParallelSparseAdam(model.parameters(), lr=lr)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
        crit = torch.nn.BCEWithLogitsLoss() if shared else torch.nn.MSELoss()
        # the single-process reference on the same global batches (every rank rebuilds every rank's loader)
        others = [ShardedBatchLoader(cols, batch, device='cpu', seed=3, rank=r, world=world, **key) for r in range(world)]
        E1 = ref[0]
        E2 = E1 if shared else ref[1]
        st = [np.zeros_like(E1), np.zeros_like(E1)]
        st += st if shared else [np.zeros_like(E2), np.zeros_like(E2)]
        k1, k2 = ('x1', 'x2') if shared else ('session', 'aid')
        epochs, t, epoch_losses, ref_losses = 2, 0, [], []
        empty_steps = 0
        for e in range(epochs):
            got = tt.train(loader, model, crit, opt, 'cpu', scheduler=sched)
            epoch_losses.append(got)
            batches = [list(ld) for ld in others]
            step_losses = []
            for k in range(len(loader)):
                parts = [batches[r][k][0] for r in range(world)]
                empty_steps += sum(p[k1].numel() == 0 for p in parts)
                i1 = torch.cat([p[k1] for p in parts]).numpy()
                i2 = torch.cat([p[k2] for p in parts]).numpy()
                tg = torch.cat([p['target'] for p in parts]).numpy()
                assert len(i1) == loader.batch_global(k)
                t += 1
                step_losses.append(mo.sparse_adam_step(E1, st[0], st[1], E2, st[2], st[3], i1, i2, tg,
                                                       crit.__class__.__name__, lr * 0.5 ** ((t - 1) // 3), step=t,
                                                       shared=shared)[0])
            ref_losses.append(float(np.mean(step_losses)))
        sd = full_state_dict(model, loader)
        assert opt._buf['cap'] == loader.max_local_batch * (2 if shared else 1)
        out = dict(epoch=epoch_losses, ref_epoch=ref_losses, empty=empty_steps, sizes=loader.sizes,
                   sd={k: v.numpy().copy() for k, v in sd.items()}, ref=[E1, E2] + st,
                   st=[v.numpy().copy() for s in opt.state.values() for v in (s['exp_avg'], s['exp_avg_sq'])])
        q.put((rank, out, None))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, out, traceback.format_exc()))
        raise


def _collect(q, procs, deadline_s):
    res, errors = {}, {}
    deadline = time.monotonic() + deadline_s
    try:
        while len(res) < len(procs) and time.monotonic() < deadline:
            try:
                r, out, err = q.get(timeout=1)
            except queue.Empty:
                if not any(p.is_alive() for p in procs):
                    break
                continue
            res[r] = out
            if err is not None:
                errors[r] = err
    finally:
        for p in procs:
            p.join(max(1.0, deadline - time.monotonic()) if not errors else 10)
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
    for r, p in enumerate(procs):
        if r not in res:
            errors[r] = f'rank {r} reported nothing (exit code {p.exitcode})'
        elif p.exitcode != 0 and r not in errors:
            errors[r] = f'rank {r} exit code {p.exitcode}'
    return res, errors


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('shared', [False, True])
def test_dp_sparse_adam_protocol_matches_union_batch_oracle(world, shared):
    """gloo, CPU tensors: padded export lists, counts, empty local batches, StepLR, the per-epoch loss all-reduce and
    full_state_dict against the oracle's single-process step on the union batches."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_protocol_worker, args=(r, world, port, shared, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, errors = _collect(q, procs, 180)
    assert not errors, '\n'.join(f'rank {r}:\n{e}' for r, e in sorted(errors.items()))
    if not shared:
        assert min(res[0]['sizes']) < -(-sum(res[0]['sizes']) // BATCH)     # a shard smaller than n_steps
        assert res[0]['empty'] > 0                                         # so some local batches are empty
    for r in range(world):
        o = res[r]
        np.testing.assert_allclose(o['epoch'], o['ref_epoch'], rtol=1e-5)
        assert o['epoch'] == res[0]['epoch']
        ref = o['ref']
        names = ['embeddings.weight'] if shared else ['session_embeddings.weight', 'aid_embeddings.weight']
        for name, want in zip(names, ref[:2]):
            np.testing.assert_allclose(o['sd'][name], want, rtol=1e-4, atol=1e-6)
        # replicated table and moments: identical on every rank
        rep = names[-1]
        assert np.array_equal(o['sd'][rep], res[0]['sd'][rep])
        assert all(np.array_equal(a, b) for a, b in zip(o['st'][-2:], res[0]['st'][-2:]))


# ---------------------------------------------------------------------------------------------------------------------
# run(): the training.distributed section
# ---------------------------------------------------------------------------------------------------------------------
def _config(**dist_section):
    cfg = {'training': {'optimizer': 'SparseAdam', 'device': 'cpu'}}
    if dist_section:
        cfg['training']['distributed'] = dist_section
    return cfg


@pytest.mark.parametrize('section,message', [
    ({'backend': 'mpi'}, "backend must be 'nccl' or 'gloo'"),
    ({'backend': 'nccl', 'overlap': True}, 'unsupported key'),
    ({'backend': 'nccl', 'device': 'cuda:3'}, "device must be 'local_rank' or 'configured'"),
])
def test_run_rejects_unsupported_distributed_settings(section, message):
    from otto_amd.matrix_factorization import torch_trainer as tt
    with pytest.raises(ValueError, match=message):
        tt._distributed_setup(_config(**section))


def test_run_distributed_needs_launcher_environment(monkeypatch):
    from otto_amd.matrix_factorization import torch_trainer as tt
    for k in ('RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match='torchrun-style launcher'):
        tt._distributed_setup(_config(backend='gloo'))
    cfg = _config(backend='gloo')
    cfg['training']['optimizer'] = 'Adam'
    with pytest.raises(ValueError, match='SparseAdam only'):
        tt._distributed_setup(cfg)


def test_run_without_section_takes_todays_path(monkeypatch):
    """No training.distributed: no process group, DeviceBatchLoader + SparseAdam, model.state_dict() checkpoints."""
    import torch.distributed as dist
    from otto_amd.matrix_factorization import torch_trainer as tt
    assert tt._distributed_setup(_config()) is None
    called = []
    monkeypatch.setattr(dist, 'init_process_group', lambda *a, **k: called.append(a))
    assert tt._distributed_setup({'training': {'optimizer': 'SparseAdam', 'device': 'cpu', 'other': 1}}) is None
    assert not called
    with pytest.raises(ValueError, match='DataParallelSparseAdam and ShardedBatchLoader'):
        from otto_amd.matrix_factorization.distributed import ShardedBatchLoader
        ld = ShardedBatchLoader({'session': [0, 1], 'aid': [0, 1], 'target': [0, 1]}, 2, device='cpu', rank=0, world=1)
        m = _standin_model(False, 2, 2, 4, 0)
        opt = tt.torch_optim.SparseAdam(m.parameters(), lr=0.1)
        tt.train(ld, m, torch.nn.MSELoss(), opt, 'cpu')
