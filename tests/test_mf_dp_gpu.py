"""GPU tests of the exact data-parallel SparseAdam step (otto_mf_dp_local / otto_mf_dp_apply) and its trainer
(otto_amd/matrix_factorization/distributed.py): W ranks emulated in one process against the oracle on the union batch
and the reference golden run, then 1-3 real processes over gloo and RCCL through the public API."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import mf_oracle as mo
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
RTOL = 1e-4
BETAS, EPS = (0.9, 0.999), 1e-8


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Ranks:
    """W emulated ranks in one process: one engine and one replica of every table per rank."""

    def __init__(self, W, E1, E2, d, max_batch, dev, shared=False, state=None):
        from otto_amd.matrix_factorization.engine import MFEngine
        self.W, self.d, self.dev, self.shared = W, d, dev, shared
        n1, n2 = E1.shape[0], E2.shape[0]
        self.engs = [MFEngine(n1, n2, d, max_batch, shared_table=shared, device=dev) for _ in range(W)]
        st = state or [np.zeros_like(E1), np.zeros_like(E1), np.zeros_like(E2), np.zeros_like(E2)]
        self.E1 = [_t(E1, dev) for _ in range(W)]
        self.m1 = [_t(st[0], dev) for _ in range(W)]
        self.v1 = [_t(st[1], dev) for _ in range(W)]
        if shared:
            self.E2, self.m2, self.v2 = self.E1, self.m1, self.v1
        else:
            self.E2 = [_t(E2, dev) for _ in range(W)]
            self.m2 = [_t(st[2], dev) for _ in range(W)]
            self.v2 = [_t(st[3], dev) for _ in range(W)]
        self.cap = max_batch * (2 if shared else 1)
        self.ids = torch.zeros((W, self.cap), dtype=torch.int32, device=dev)
        self.rows = torch.full((W, self.cap, d), float('nan'), device=dev)     # padding is never read
        self.count = torch.zeros((W, 1), dtype=torch.int64, device=dev)
        self.loss = torch.zeros(W, device=dev)

    def step(self, parts, cuts, kind, lr, t, batch_global=None):
        """parts[r] = (i1, i2, target) device int64; cuts[r], cuts[r + 1] = rank r's private rows. Returns the summed loss."""
        Bg = batch_global or sum(p[0].numel() for p in parts)
        self.rows.fill_(float('nan'))
        for r, (i1, i2, tg) in enumerate(parts):
            self.engs[r].dp_local(self.E1[r], None if self.shared else self.m1[r], None if self.shared else self.v1[r],
                                  self.E2[r], i1, i2, tg, Bg, cuts[r], cuts[r + 1], kind, lr, BETAS, EPS, t,
                                  self.ids[r], self.rows[r], self.count[r], self.loss[r:r + 1])
        for r in range(self.W):     # every replica gets its own copy of the gathered lists (the apply half consumes rows)
            self.engs[r].dp_apply(self.E2[r], self.m2[r], self.v2[r], self.ids.clone(), self.rows.clone(),
                                  self.count.reshape(-1).clone(), lr, BETAS, EPS, t)
        return float(self.loss.sum())

    def assert_replicas_identical(self):
        for r in range(1, self.W):
            for a in (self.E2, self.m2, self.v2):
                assert torch.equal(a[r], a[0]), f'replica {r} differs from replica 0'

    def private(self, cuts, which):
        """The private table as rank r's own rows [cuts[r], cuts[r + 1]) assembled (numpy)."""
        src = {'E1': self.E1, 'm1': self.m1, 'v1': self.v1}[which]
        out = src[0].cpu().numpy().copy()
        for r in range(self.W):
            out[cuts[r]:cuts[r + 1]] = src[r][cuts[r]:cuts[r + 1]].cpu().numpy()
        return out


def _split_by_session(i1, i2, tg, cuts):
    parts, order = [], []
    for r in range(len(cuts) - 1):
        sel = np.nonzero((i1 >= cuts[r]) & (i1 < cuts[r + 1]))[0]
        parts.append(sel)
        order.append(sel)
    return parts, np.concatenate(order)


def _close(got, ref, atol=2e-5):
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=atol)
    assert np.linalg.norm(got - ref) <= RTOL * max(np.linalg.norm(ref), 1e-30)


@pytest.mark.parametrize('W', [1, 2, 3])
@pytest.mark.parametrize('d,B', [(32, 262144), (16, 4096), (64, 4096), (128, 2048)])
def test_dp_halves_match_union_batch_oracle_heavy_duplicates(gpu_device, W, d, B):
    from otto_amd.matrix_factorization.distributed import session_cuts
    rng = np.random.default_rng(d * 7 + W)
    n1, n2 = (200000, 20000) if B > 100000 else (3000, 200)
    E1 = (rng.standard_normal((n1, d)) * 0.3).astype(np.float32)
    E2 = (rng.standard_normal((n2, d)) * 0.3).astype(np.float32)
    st = [np.zeros_like(E1), np.zeros_like(E1), np.zeros_like(E2), np.zeros_like(E2)]
    E1_0 = E1.copy()
    i1_all = rng.integers(0, n1, 3 * B)
    cuts, _ = session_cuts(torch.from_numpy(i1_all), W, n1)
    ranks = Ranks(W, E1, E2, d, B, gpu_device)
    for step in range(1, 4):
        i1 = i1_all[(step - 1) * B:step * B]
        i2 = np.minimum(rng.zipf(1.3, B) - 1, n2 - 1)      # one aid holds a large share of the batch
        tg = rng.integers(0, 3, B)
        sel, order = _split_by_session(i1, i2, tg, cuts)
        parts = [(_t(i1[s], gpu_device), _t(i2[s], gpu_device), _t(tg[s], gpu_device)) for s in sel]
        loss = ranks.step(parts, cuts, 0, 0.05, step)
        want, _ = mo.sparse_adam_step(E1, st[0], st[1], E2, st[2], st[3], i1[order], i2[order], tg[order], 'MSELoss', 0.05,
                                      step=step)
        np.testing.assert_allclose(loss, want, rtol=RTOL)
        ranks.assert_replicas_identical()
    for r in range(W):      # private rows outside a rank's shard are never written
        outside = np.ones(n1, bool)
        outside[cuts[r]:cuts[r + 1]] = False
        assert np.array_equal(ranks.E1[r].cpu().numpy()[outside], E1_0[outside])
        assert not ranks.m1[r].cpu().numpy()[outside].any()
    _close(ranks.private(cuts, 'E1'), E1)
    _close(ranks.private(cuts, 'm1'), st[0])
    _close(ranks.E2[0].cpu().numpy(), E2)
    _close(ranks.m2[0].cpu().numpy(), st[2])
    _close(ranks.v2[0].cpu().numpy(), st[3], atol=1e-9)
    for e in ranks.engs:
        e.check()


@pytest.mark.parametrize('W', [2, 3])
def test_dp_shared_table_matches_union_batch_oracle(gpu_device, W):
    rng = np.random.default_rng(W)
    n, d, B = 500, 16, 3000
    E = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    st = [np.zeros_like(E), np.zeros_like(E)]
    ranks = Ranks(W, E, E, d, B // W + 1, gpu_device, shared=True, state=st + st)
    for step in range(1, 4):
        x1, x2 = rng.integers(0, n, B), np.minimum(rng.zipf(1.4, B) - 1, n - 1)
        tg = rng.integers(0, 2, B)
        cut = [(r * B) // W for r in range(W + 1)]
        parts = [(_t(x1[cut[r]:cut[r + 1]], gpu_device), _t(x2[cut[r]:cut[r + 1]], gpu_device),
                  _t(tg[cut[r]:cut[r + 1]], gpu_device)) for r in range(W)]
        loss = ranks.step(parts, [0] * (W + 1), 1, 0.05, step)
        want, _ = mo.sparse_adam_step(E, st[0], st[1], E, st[0], st[1], x1, x2, tg, 'BCEWithLogitsLoss', 0.05, step=step,
                                      shared=True)
        np.testing.assert_allclose(loss, want, rtol=RTOL)
        ranks.assert_replicas_identical()
    _close(ranks.E1[0].cpu().numpy(), E)
    _close(ranks.m1[0].cpu().numpy(), st[0])


def test_dp_empty_local_batch_and_zero_gradient_row(gpu_device):
    """W = 3, rank 1 has an empty local batch; aid 7 is touched only by a sample whose session row is all zeros, so its
    summed gradient is exactly 0, and its moments must still decay (torch's sparse_adam updates every touched row)."""
    rng = np.random.default_rng(3)
    n1, n2, d, B = 90, 40, 8, 60
    E1 = (rng.standard_normal((n1, d)) * 0.3).astype(np.float32)
    E2 = (rng.standard_normal((n2, d)) * 0.3).astype(np.float32)
    E1[5] = 0.0
    st = [np.zeros_like(E1), np.zeros_like(E1), (rng.random((n2, d)) * 0.1).astype(np.float32),
          (rng.random((n2, d)) * 0.01).astype(np.float32)]
    m2_before = st[2][7].copy()
    cuts = [0, 30, 60, 90]
    ranks = Ranks(3, E1, E2, d, B, gpu_device, state=[s.copy() for s in st])
    i1 = np.concatenate([[5], rng.integers(0, 30, 20), rng.integers(60, 90, 15)])
    i2 = np.concatenate([[7], rng.integers(8, n2, 35)])
    tg = rng.integers(0, 3, len(i1))
    sel = [np.arange(0, 21), np.zeros(0, np.int64), np.arange(21, 36)]
    parts = [(_t(i1[s], gpu_device), _t(i2[s], gpu_device), _t(tg[s], gpu_device)) for s in sel]
    loss = ranks.step(parts, cuts, 0, 0.01, 1)
    assert int(ranks.count[1]) == 0 and float(ranks.loss[1]) == 0.0
    want, _ = mo.sparse_adam_step(E1, st[0], st[1], E2, st[2], st[3], i1, i2, tg, 'MSELoss', 0.01, step=1)
    np.testing.assert_allclose(loss, want, rtol=RTOL)
    ranks.assert_replicas_identical()
    m2 = ranks.m2[0].cpu().numpy()
    np.testing.assert_allclose(m2[7], m2_before * np.float32(0.9), rtol=1e-6)
    np.testing.assert_allclose(m2[7], st[2][7], rtol=1e-6)
    _close(ranks.E2[0].cpu().numpy(), E2)
    _close(ranks.private(cuts, 'E1'), E1)


def test_dp_out_of_shard_and_out_of_table_ids_are_skipped_and_reported(gpu_device):
    from otto_amd import _lib
    rng = np.random.default_rng(11)
    n1, n2, d, B = 100, 50, 8, 40
    E1 = (rng.standard_normal((n1, d)) * 0.3).astype(np.float32)
    E2 = (rng.standard_normal((n2, d)) * 0.3).astype(np.float32)
    E1_0 = E1.copy()
    cuts = [0, 50, 100]
    ranks = Ranks(2, E1, E2, d, B, gpu_device)
    i1 = np.concatenate([rng.integers(0, 50, 20), rng.integers(50, 100, 20)])
    i2 = rng.integers(0, n2, B)
    tg = rng.integers(0, 3, B)
    bad1 = i1.copy()
    bad1[3] = 77          # rank 0 does not own session 77
    bad2 = i2.copy()
    bad2[25] = n2 + 3     # outside the aid table
    sel = [np.arange(0, 20), np.arange(20, 40)]
    parts = [(_t(bad1[s], gpu_device), _t(bad2[s], gpu_device), _t(tg[s], gpu_device)) for s in sel]
    ranks.step(parts, cuts, 0, 0.01, 1)
    with pytest.raises(_lib.OttoError, match='1 sample'):
        ranks.engs[0].check()
    with pytest.raises(_lib.OttoError, match='1 sample'):
        ranks.engs[1].check()
    ranks.engs[0].check()
    keep = np.array([b not in (3, 25) for b in range(B)])
    mo.sparse_adam_step(E1, np.zeros_like(E1), np.zeros_like(E1), E2, np.zeros_like(E2), np.zeros_like(E2), i1[keep],
                        i2[keep], tg[keep], 'MSELoss', 0.01, step=1, batch_size=B)
    assert np.array_equal(ranks.E1[0].cpu().numpy()[77], E1_0[77])      # rank 0 does not own session 77
    _close(ranks.private(cuts, 'E1'), E1)
    _close(ranks.E2[0].cpu().numpy(), E2)
    ranks.assert_replicas_identical()


@pytest.mark.parametrize('d', [8, 32, 128])
def test_dp_world_one_without_duplicate_aids_is_bit_identical_to_single_step(gpu_device, d):
    from otto_amd.matrix_factorization.engine import MFEngine
    rng = np.random.default_rng(d)
    n1, n2, B = 5000, 3000, 2000
    E1 = (rng.standard_normal((n1, d)) * 0.3).astype(np.float32)
    E2 = (rng.standard_normal((n2, d)) * 0.3).astype(np.float32)
    ranks = Ranks(1, E1, E2, d, B, gpu_device)
    eng = MFEngine(n1, n2, d, B, device=gpu_device)
    ref = [_t(x, gpu_device) for x in (E1, np.zeros_like(E1), np.zeros_like(E1), E2, np.zeros_like(E2), np.zeros_like(E2))]
    loss = torch.zeros(1, device=gpu_device)
    for step in range(1, 4):
        i1 = rng.permutation(n1)[:B]          # no row twice: a float atomic sum of 3+ terms has no fixed order
        i2 = rng.permutation(n2)[:B]          # no aid twice
        tg = rng.integers(0, 3, B)
        di = [_t(x, gpu_device) for x in (i1, i2, tg)]
        ranks.step([tuple(di)], [0, n1], 0, 0.05, step)
        eng.step_sparse_adam(*ref, *di, 0, 0.05, BETAS, EPS, step, loss)
        assert torch.equal(ranks.loss[0:1], loss)
        for got, want in zip((ranks.E1[0], ranks.m1[0], ranks.v1[0], ranks.E2[0], ranks.m2[0], ranks.v2[0]), ref):
            assert torch.equal(got, want)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'mf_golden.npz'))


@pytest.mark.parametrize('W', [2, 3])
@pytest.mark.parametrize('p,loss_kind,shared', [('mf_', 0, False), ('cf_', 1, True)])
def test_dp_training_matches_reference_golden(gold, gpu_device, p, loss_kind, shared, W):
    """The golden run (3 epochs, StepLR per batch) with each batch split over W emulated ranks: by session chunk (mf_)
    or by row range (cf_); same tolerances as test_sparse_adam_training_matches_reference_golden."""
    from otto_amd.matrix_factorization.distributed import session_cuts
    g = gold
    n1, n2, d, B, nb, ne, step_size = g[p + 'hyper'].tolist()
    lr0 = float(g[p + 'lr'])
    w1 = g[p + 'w1_0']
    w2 = w1 if shared else g[p + 'w2_0']
    ranks = Ranks(W, w1, w2, d, B, gpu_device, shared=shared)
    i1, i2, tg = g[p + 'i1'], g[p + 'i2'], g[p + 'target']
    cuts = session_cuts(torch.from_numpy(i1.reshape(-1)), W, n1)[0] if not shared else [0] * (W + 1)
    losses, t = [], 0
    for e in range(ne):
        for b in range(nb):
            lr = lr0 * 0.5 ** (t // step_size)
            t += 1
            if shared:
                rc = [(r * B) // W for r in range(W + 1)]
                sel = [np.arange(rc[r], rc[r + 1]) for r in range(W)]
            else:
                sel, _ = _split_by_session(i1[b], i2[b], tg[b], cuts)
            parts = [(_t(i1[b][s], gpu_device), _t(i2[b][s], gpu_device), _t(tg[b][s], gpu_device)) for s in sel]
            losses.append(ranks.step(parts, cuts, loss_kind, lr, t))
            ranks.assert_replicas_identical()
            if t == 1:
                full = (lambda k: ranks.private(cuts, k)) if not shared else (lambda k: getattr(ranks, k)[0].cpu().numpy())
                np.testing.assert_allclose(full('E1'), g[p + 'step_w1'], rtol=RTOL, atol=1e-6)
                np.testing.assert_allclose(full('m1'), g[p + 'step_m1'], rtol=RTOL, atol=1e-7)
                np.testing.assert_allclose(full('v1'), g[p + 'step_v1'], rtol=RTOL, atol=1e-9)
                if not shared:
                    np.testing.assert_allclose(ranks.E2[0].cpu().numpy(), g[p + 'step_w2'], rtol=RTOL, atol=1e-6)
                    np.testing.assert_allclose(ranks.v2[0].cpu().numpy(), g[p + 'step_v2'], rtol=RTOL, atol=1e-9)
    losses = np.asarray(losses, dtype=np.float64)
    np.testing.assert_allclose(losses, g[p + 'step_loss'], rtol=RTOL)
    np.testing.assert_allclose(losses.reshape(ne, nb).mean(1), g[p + 'epoch_train_loss'], rtol=RTOL)
    for key, which in (('w1_T', 'E1'), ('m1_T', 'm1')):
        a = ranks.private(cuts, which) if not shared else getattr(ranks, which)[0].cpu().numpy()
        np.testing.assert_allclose(a, g[p + key], rtol=1e-3, atol=2e-5 if key == 'w1_T' else 1e-6)
        assert np.linalg.norm(a - g[p + key]) <= RTOL * np.linalg.norm(g[p + key])


# ---------------------------------------------------------------------------------------------------------------------
# real processes through the public API
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _data(shared, seed=21):
    rng = np.random.default_rng(seed)
    if shared:
        n = 3000
        return {'x1': rng.integers(0, 400, n), 'x2': np.minimum(rng.zipf(1.4, n) - 1, 399),
                'target': rng.integers(0, 2, n)}, 400, 400
    # unequal shards: session 10 holds most rows, so the balanced cuts leave the last rank fewer rows than n_steps (and,
    # with 3 ranks, the middle rank none at all)
    sess = np.concatenate([rng.integers(0, 10, 20), np.full(3000, 10), rng.integers(11, 600, 30)])
    aid = np.minimum(rng.zipf(1.3, len(sess)) - 1, 299)
    return {'session': sess, 'aid': aid, 'target': rng.integers(0, 3, len(sess))}, 600, 300


BATCH, EPOCHS, LR = 64, 2, 0.02


def _model(shared, n1, n2, dev):
    from otto_amd.matrix_factorization import torch_modules as tm
    torch.manual_seed(5)
    m = tm.CollaborativeFiltering(n1, 16) if shared else tm.MatrixFactorization(n1, n2, 16)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.3)
    return m.to(dev)


def _dp_worker(rank, world, port, shared, backend, q):
    import traceback
    from datetime import timedelta
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
    out = None
    try:
        import torch.distributed as dist
        from otto_amd.matrix_factorization import torch_trainer as tt
        from otto_amd.matrix_factorization.distributed import DataParallelSparseAdam, ShardedBatchLoader, full_state_dict
        dev = torch.device('cuda:0')
        torch.cuda.set_device(dev)
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=120))
        cols, n1, n2 = _data(shared)
        key = dict(shard_key=None) if shared else dict(shard_key='session', n_keys=n1)
        tl = ShardedBatchLoader(cols, BATCH, device=dev, seed=1, **key)
        vl = ShardedBatchLoader(cols, BATCH * 2, device=dev, seed=2, **key)
        model = _model(shared, n1, n2, dev)
        opt = DataParallelSparseAdam(model.parameters(), lr=LR)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
        crit = torch.nn.BCEWithLogitsLoss() if shared else torch.nn.MSELoss()
        out = dict(train=[], val=[], scores=[], rep=[], sizes=tl.sizes, n_steps=len(tl))
        for _ in range(EPOCHS):
            out['train'].append(tt.train(tl, model, crit, opt, dev, scheduler=sched))
            vloss, sc = tt.validate(vl, model, crit, dev, scores=True)
            out['val'].append(vloss)
            out['scores'].append(sc)
            E2 = model._tables()[1]
            s2 = opt.state[E2]
            out['rep'].append([E2.detach().cpu().numpy().copy(), s2['exp_avg'].cpu().numpy().copy(),
                               s2['exp_avg_sq'].cpu().numpy().copy()])
        out['sd'] = {k: v.cpu().numpy().copy() for k, v in full_state_dict(model, tl).items()}
        q.put((rank, out, None))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, out, traceback.format_exc()))
        raise


def _single_process_reference(shared, world, dev):
    """One process, plain SparseAdam.fused_step, fed the concatenation of the ranks' batches."""
    from otto_amd.matrix_factorization import torch_optim
    from otto_amd.matrix_factorization.distributed import ShardedBatchLoader
    from otto_amd.matrix_factorization.torch_optim import loss_kind
    from otto_amd.matrix_factorization import metrics
    cols, n1, n2 = _data(shared)
    key = dict(shard_key=None) if shared else dict(shard_key='session', n_keys=n1)
    tls = [ShardedBatchLoader(cols, BATCH, device=dev, seed=1, rank=r, world=world, **key) for r in range(world)]
    vls = [ShardedBatchLoader(cols, BATCH * 2, device=dev, seed=2, rank=r, world=world, **key) for r in range(world)]
    model = _model(shared, n1, n2, dev)
    opt = torch_optim.SparseAdam(model.parameters(), lr=LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    crit = torch.nn.BCEWithLogitsLoss() if shared else torch.nn.MSELoss()
    k1, k2 = ('x1', 'x2') if shared else ('session', 'aid')
    train, val, scores = [], [], []
    E1, E2, _ = model._tables()
    for _ in range(EPOCHS):
        losses = torch.zeros(len(tls[0]), device=dev)
        for k, parts in enumerate(zip(*tls)):
            cat = {c: torch.cat([p[0][c] for p in parts]) for c in (k1, k2, 'target')}
            opt.fused_step(model, cat[k1], cat[k2], cat['target'], crit, losses[k:k + 1])
            sched.step()
        train.append(float(losses.double().mean()))
        vl, preds, tgs = [], [], []
        eng = model.engine(max(v.max_local_batch for v in vls) * world)
        eng.read_sums(reset=True)
        for parts in zip(*vls):
            cat = {c: torch.cat([p[0][c] for p in parts]) for c in (k1, k2, 'target')}
            lo = torch.zeros(1, device=dev)
            pr = torch.empty(cat[k1].numel(), device=dev)
            eng.eval_sums(E1.data, E2.data, cat[k1], cat[k2], cat['target'], loss_kind(crit), lo, pr)
            vl.append(float(lo))
            preds.append(pr)
            tgs.append(cat['target'])
        val.append(float(np.mean(vl)))
        auc = metrics.roc_auc(torch.cat(tgs), torch.sigmoid(torch.cat(preds))) if shared else None
        scores.append(metrics.scores_from_sums(eng.read_sums(reset=True), shared, auc))
    return train, val, scores, {k: v.cpu().numpy() for k, v in model.state_dict().items()}


def _launch(world, shared, backend):
    from test_mf_dp_cpu import _collect
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, shared, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, errors = _collect(q, procs, 300)
    assert not errors, '\n'.join(f'rank {r}:\n{e}' for r, e in sorted(errors.items()))
    return res


def _compare(res, world, shared, dev):
    train, val, scores, sd = _single_process_reference(shared, world, dev)
    for r in range(world):
        o = res[r]
        assert o['train'] == res[0]['train'] and o['val'] == res[0]['val'] and o['scores'] == res[0]['scores']
        for e in range(EPOCHS):
            assert all(np.array_equal(a, b) for a, b in zip(o['rep'][e], res[0]['rep'][e])), f'rank {r} epoch {e}'
        np.testing.assert_allclose(o['train'], train, rtol=RTOL)
        np.testing.assert_allclose(o['val'], val, rtol=RTOL)
        n_val = sum(o['sizes'])
        for got, want in zip(o['scores'], scores):
            assert got.keys() == want.keys()
            for k in want:      # accuracy: a probability within the tables' 1e-4 of 0.5 may land on the other side
                np.testing.assert_allclose(got[k], want[k], rtol=RTOL, atol=1.01 / n_val if k == 'accuracy' else 0)
        assert o['sd'].keys() == sd.keys()
        for k in sd:
            np.testing.assert_allclose(o['sd'][k], sd[k], rtol=1e-3, atol=2e-5)
            assert np.linalg.norm(o['sd'][k] - sd[k]) <= RTOL * np.linalg.norm(sd[k])


@pytest.mark.parametrize('world,shared', [(2, False), (3, False), (2, True)])
def test_dp_trainer_gloo_processes_match_single_process(gpu_device, world, shared):
    res = _launch(world, shared, 'gloo')
    if not shared:
        sizes, steps = res[0]['sizes'], res[0]['n_steps']
        assert len(set(sizes)) == world and min(sizes) < steps     # unequal shards, one smaller than n_steps
    _compare(res, world, shared, gpu_device)


def test_dp_trainer_rccl_world_of_one_matches_plain_trainer(gpu_device):
    res = _launch(1, False, 'nccl')
    _compare(res, 1, False, gpu_device)


def _run_worker(rank, world, port, tmp, q):
    import traceback
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0', OTTO_DATA=os.path.join(tmp, 'data'), OTTO_MODELS=os.path.join(tmp, 'models'),
                      OTTO_LOGS=os.path.join(tmp, 'logs'))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
    try:
        from otto_amd.matrix_factorization import torch_trainer as tt
        cols, n1, n2 = _data(False)
        cfg = {
            'model': {'model_class': 'MatrixFactorization', 'n_sessions': n1, 'n_aids': n2, 'n_factors': 16, 'sparse': True,
                      'dropout_probability': 0.0, 'model_checkpoint_path': None},
            'dataset': {'load_dataset': True},
            'training': {'device': 'cuda:0', 'random_state': 42, 'deterministic_cudnn': False, 'training_batch_size': BATCH,
                         'validation_batch_size': BATCH, 'loss_function': 'MSELoss', 'loss_args': {},
                         'optimizer': 'SparseAdam', 'optimizer_args': {'lr': LR}, 'lr_scheduler': 'StepLR',
                         'lr_scheduler_args': {'step_size': 10, 'gamma': 0.5}, 'epochs': 2, 'scores': True,
                         'early_stopping_patience': 0, 'distributed': {'backend': 'gloo', 'device': 'configured'}},
            'persistence': {'model_directory': f'mf_dp_rank{rank}', 'save_epoch_model': [], 'save_best_model': True,
                            'visualize_learning_curve': False},
        }
        _, summary, scores = tt.run(cfg)
        q.put((rank, (summary, scores), None))
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise


def test_run_with_distributed_section_two_processes(gpu_device, tmp_path):
    import pandas as pd
    from test_mf_dp_cpu import _collect
    from otto_amd.matrix_factorization import torch_modules as tm
    cols, n1, n2 = _data(False)
    (tmp_path / 'data' / 'matrix_factorization').mkdir(parents=True)
    pd.DataFrame(cols).to_parquet(tmp_path / 'data' / 'matrix_factorization' / 'sessions_aids.parquet')
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res, errors = _collect(q, procs, 300)
    assert not errors, '\n'.join(f'rank {r}:\n{e}' for r, e in sorted(errors.items()))
    assert res[0] == res[1]
    assert (tmp_path / 'models' / 'mf_dp_rank0' / 'model_best.pt').exists()
    assert not (tmp_path / 'models' / 'mf_dp_rank1' / 'model_best.pt').exists()
    sd = torch.load(tmp_path / 'models' / 'mf_dp_rank0' / 'model_best.pt', weights_only=True)
    assert set(sd) == {'session_embeddings.weight', 'aid_embeddings.weight'}
    assert sd['session_embeddings.weight'].shape == (n1, 16) and sd['aid_embeddings.weight'].shape == (n2, 16)
    fresh = tm.MatrixFactorization(n1, n2, 16)
    fresh.load_state_dict(sd)
