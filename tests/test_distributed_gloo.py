"""world_size-2 gloo (CPU) test of the multi-GPU covisitation exchange
(otto_amd/covisitation/distributed.py): the real exchange code routes runs produced by a
CPU stand-in engine built on the oracle's per-window expansion; owners reduce with the
oracle; the union must equal the single-process result."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

import covis_oracle as co


class OracleEngine:
    """CPU stand-in with the export_runs/import_runs surface of CovisBuilder (tests only)."""
    FK = ('click_cart', 'click_order', 'cart_order', 'click_click')

    def __init__(self):
        self.runs = []   # (x, [rec...], [tw...])

    def feed(self, aid, ts, typ, off, t0, t1):
        sp = co.CovisSpec()
        for s in range(len(off) - 1):
            rows = co.expand_window_python(aid, ts, typ, int(off[s]), int(off[s + 1]), sp, self.FK, t0, t1)
            cur = None
            for x, y, ty, fb, ex in rows:
                if cur is None or cur[0] != x:
                    cur = (x, [], [])
                    self.runs.append(cur)
                cur[1].append(y | ty << 26 | fb << 28)
                cur[2].append(ex)

    def export_runs(self, lo, hi):
        sel = [r for r in self.runs if lo <= r[0] < hi]
        hdr = torch.tensor([[r[0], len(r[1])] for r in sel], dtype=torch.int32).reshape(-1, 2)
        rec = torch.tensor([v for r in sel for v in r[1]], dtype=torch.int64).to(torch.int32)
        tw = torch.tensor([v for r in sel for v in r[2]], dtype=torch.int32)
        return hdr, rec, tw

    # the run-slot range surface of the chunked exchange (exchange_runs_chunked): slot i = self.runs[i]
    device = torch.device('cpu')

    def run_slots(self):
        return len(self.runs)

    def _owned(self, bounds, lo, hi):
        return [[r for r in self.runs[lo:hi] if bounds[o] <= r[0] < bounds[o + 1]] for o in range(len(bounds) - 1)]

    def export_plan_range(self, bounds, lo, hi):
        assert 0 <= lo <= hi <= len(self.runs)
        own = self._owned(bounds, lo, hi)
        return [len(rs) for rs in own], [sum(len(r[1]) for r in rs) for rs in own]

    def export_fill_range(self, bounds, lo, hi, runs, recs, hdr, rec, tw=None):
        sel = [r for rs in self._owned(bounds, lo, hi) for r in rs]
        assert hdr.shape == (sum(runs), 2) and rec.numel() == sum(recs) == sum(len(r[1]) for r in sel)
        p = 0
        for i, (x, rc, tws) in enumerate(sel):
            hdr[i, 0], hdr[i, 1] = x, len(rc)
            rec[p:p + len(rc)] = torch.tensor(rc, dtype=torch.int64).to(torch.int32)
            if tw is not None:
                tw[p:p + len(rc)] = torch.tensor(tws, dtype=torch.int32)
            p += len(rc)

    def import_reserve(self, n):
        return torch.empty(n, dtype=torch.int32), torch.empty(n, dtype=torch.int32)

    def import_runs(self, hdr, rec, tw):
        p = 0
        for x, n in hdr.tolist():
            self.runs.append((x, (rec[p:p + n].to(torch.int64) & 0xFFFFFFFF).tolist(), tw[p:p + n].tolist()))
            p += n

    def reduce(self):
        """{(x, y): (c0, c1, c2, cnt_fbits[4], time W)}"""
        acc = {}
        for x, recs, tws in self.runs:
            for rc, ex in zip(recs, tws):
                y, ty, fb = rc & 0x3FFFFFF, (rc >> 26) & 3, rc >> 28
                a = acc.setdefault((x, y), [0, 0, 0, 0, 0, 0, 0, 0])
                a[ty] += 1
                for f in range(4):
                    a[3 + f] += (fb >> f) & 1
                a[7] += co.Q16 + ex
        return acc


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
    import torch.distributed as dist
    from otto_amd.synth import generate_sessions
    from otto_amd.covisitation.distributed import exchange_runs, owner_bounds, global_ts_range
    dist.init_process_group('gloo', rank=rank, world_size=world)
    ev = generate_sessions(160, n_aids=90, seed=77)
    half = ev.n_sessions // world
    lo, hi = rank * half, (rank + 1) * half if rank < world - 1 else ev.n_sessions
    e0, e1 = int(ev.sess_off[lo]), int(ev.sess_off[hi])
    t0, t1 = global_ts_range(torch.from_numpy(ev.ts[e0:e1]))
    assert (t0, t1) == (int(ev.ts.min()), int(ev.ts.max()))
    local, owner = OracleEngine(), OracleEngine()
    local.feed(ev.aid[e0:e1], ev.ts[e0:e1], ev.type[e0:e1], ev.sess_off[lo:hi + 1] - e0, t0, t1)
    bounds = owner_bounds(ev.n_aids, world)
    sent = exchange_runs(local.export_runs, owner.import_runs, bounds, want_time=True)
    assert sent[1] == sum(len(r[1]) for r in local.runs)
    acc = owner.reduce()
    assert all(bounds[rank] <= x < bounds[rank + 1] for x, _ in acc)
    q.put((rank, acc))
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_world2_matches_single_process():
    from otto_amd.synth import generate_sessions
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    parts = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    merged = {}
    for acc in parts.values():
        assert not (set(acc) & set(merged))
        merged.update(acc)
    ev = generate_sessions(160, n_aids=90, seed=77)
    want = co.covis_pairs_python(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec())
    for kind, tw in co.TYPE_WEIGHTS.items():
        got = {p: co.Q16 * (a[0] * tw[0] + a[1] * tw[1] + a[2] * tw[2]) for p, a in merged.items()}
        assert got == want[kind], kind
    for f, kind in enumerate(OracleEngine.FK):
        got = {p: co.Q16 * a[3 + f] for p, a in merged.items() if a[3 + f]}
        assert got == want[kind], kind
    assert {p: a[7] for p, a in merged.items()} == want['time_weighted']


def _chunked_events(world):
    """Unequal shards for the chunked exchange: one rank holds the 160 generated sessions, one a single 2-event session
    (2 run slots), with 3 ranks rank 0 none; the aids leave owner 1's range empty (it receives nothing)."""
    from otto_amd.synth import Events, generate_sessions
    from otto_amd.covisitation.distributed import owner_bounds
    n_aids = 90
    b = owner_bounds(n_aids, world)
    gen = generate_sessions(160, n_aids=n_aids - (b[2] - b[1]), seed=78)
    gen_aid = np.where(gen.aid >= b[1], gen.aid + (b[2] - b[1]), gen.aid).astype(np.uint32)
    t = int(gen.ts.min()) + 500
    tiny = (np.array([3, 5], np.uint32), np.array([t, t + 40], np.int32), np.array([0, 1], np.uint8))
    big = (gen_aid, gen.ts, gen.type)
    if world == 2:
        parts, shards, lens = [tiny, big], [(0, 1), (1, 161)], np.concatenate([[2], np.diff(gen.sess_off)])
    else:
        parts, shards, lens = [big, tiny], [(0, 0), (0, 160), (160, 161)], np.concatenate([np.diff(gen.sess_off), [2]])
    ev = Events(aid=np.concatenate([p[0] for p in parts]), ts=np.concatenate([p[1] for p in parts]),
                type=np.concatenate([p[2] for p in parts]), sess_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                n_aids=n_aids)
    return ev, shards


def collect_workers(q, procs, deadline_s):
    """Reads one ``(rank, result, error | None)`` per worker from ``q`` for at most ``deadline_s`` seconds, stops early once
    every worker has exited, then terminates and joins whatever is still alive. A worker that reported nothing becomes an
    error. Returns ({rank: result}, {rank: (where, message)})."""
    import queue
    import time
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
            errors[r] = (None, f'rank {r} reported nothing (exit code {p.exitcode})')
    return res, errors


CHUNKS = (1, 2, 4, 7)


def _chunked_worker(rank, world, port, q):
    import traceback
    from datetime import timedelta
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]
    import torch.distributed as dist
    from otto_amd.covisitation.distributed import exchange_runs_chunked, owner_bounds, global_ts_range
    out, n = {}, None
    try:
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=timedelta(seconds=60))
        ev, shards = _chunked_events(world)
        lo, hi = shards[rank]
        e0, e1 = int(ev.sess_off[lo]), int(ev.sess_off[hi])
        t0, t1 = global_ts_range(torch.from_numpy(ev.ts[e0:e1]))
        bounds = owner_bounds(ev.n_aids, world)
        for n in CHUNKS:
            for stage in (None, 'cpu'):
                local, owner = OracleEngine(), OracleEngine()
                local.feed(ev.aid[e0:e1], ev.ts[e0:e1], ev.type[e0:e1], ev.sess_off[lo:hi + 1] - e0, t0, t1)
                ex = exchange_runs_chunked(local, owner, bounds, want_time=True, n_chunks=n, stage_device=stage)
                out[(n, stage)] = (local.run_slots(), ex, owner.reduce())
        q.put((rank, out, None))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, out, (n, traceback.format_exc())))
        raise


@pytest.mark.parametrize('world', [2, 3])
def test_chunked_exchange_unequal_shards_and_an_owner_receiving_nothing(world):
    """exchange_runs_chunked over gloo with 1, 2, 4 and 7 run-slot ranges, on device and staged: a rank with 2 run slots
    (fewer than the ranges: it still issues every range's collectives, empty), with 3 ranks a rank without sessions, and
    an owner that receives zero runs and zero records while the time channel is on. Union of the owners == the oracle."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_chunked_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, errors = collect_workers(q, procs, 150)
    assert not errors, '\n'.join(f'rank {r} (n_chunks {e[0]}):\n{e[1]}' for r, e in sorted(errors.items()))
    from otto_amd.covisitation.distributed import owner_bounds
    ev, _ = _chunked_events(world)
    bounds = owner_bounds(ev.n_aids, world)
    want = co.covis_pairs_python(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec())
    for key in res[0]:
        slots = [res[r][key][0] for r in range(world)]
        ex = [res[r][key][1] for r in range(world)]
        assert sorted(slots)[:world - 1] == ([0, 2] if world == 3 else [2])      # the shards this test is about
        assert ex[1][2:] == (0, 0)                                               # owner 1 receives nothing
        assert sum(e[0] for e in ex) == sum(e[2] for e in ex) == sum(slots)
        assert sum(e[1] for e in ex) == sum(e[3] for e in ex)
        merged = {}
        for r in range(world):
            assert all(bounds[r] <= x < bounds[r + 1] for x, _ in res[r][key][2])
            assert not (set(res[r][key][2]) & set(merged))
            merged.update(res[r][key][2])
        for kind, tw in co.TYPE_WEIGHTS.items():
            got = {p: co.Q16 * (a[0] * tw[0] + a[1] * tw[1] + a[2] * tw[2]) for p, a in merged.items()}
            assert got == want[kind], (key, kind)
        for f, kind in enumerate(OracleEngine.FK):
            assert {p: co.Q16 * a[3 + f] for p, a in merged.items() if a[3 + f]} == want[kind], (key, kind)
        assert {p: a[7] for p, a in merged.items()} == want['time_weighted'], key


def test_owner_bounds_partition():
    from otto_amd.covisitation.distributed import owner_bounds
    for n, w in ((1855603, 8), (10, 3), (7, 8)):
        b = owner_bounds(n, w)
        assert b[0] == 0 and b[-1] == n and all(b[i] <= b[i + 1] for i in range(w))


# ---- data-parallel BPR: ItemTableSync over gloo with the oracle's batch step standing in for the HIP kernel -------------
def _planted_small(seed=0):
    rng = np.random.default_rng(seed)
    n_users, n_items, groups = 1200, 601, 12
    grp = rng.integers(0, groups, n_users)
    item_grp = np.r_[-1, rng.integers(0, groups, n_items - 1)]
    by = [np.flatnonzero(item_grp == g_) for g_ in range(groups)]
    u = np.repeat(np.arange(n_users), 10)
    i = np.array([rng.choice(by[grp[x]]) for x in u])
    return u, i, n_users, n_items


class _CpuBpr:
    """Stand-in for BPR + MFEngine on CPU tensors: `train_epoch` drives it exactly as it drives the HIP engine
    (tests only; the arithmetic is oracle/mf_oracle.bpr_step_batch)."""

    class _Emb:
        def __init__(self, w):
            self.weight = type('P', (), {'data': w})()

    def __init__(self, n_users, n_items, d, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.user_embedding = self._Emb(torch.randn(n_users, d, generator=g) * 0.1)
        self.item_embedding = self._Emb(torch.randn(n_items, d, generator=g) * 0.1)
        self.rng = np.random.default_rng(5)

    def engine(self, batch):
        return self

    def bpr_step(self, U, V, users, items, seed, epoch, row0, lr, l2, mode, loss_sum=None, neg_out=None):
        import mf_oracle as mo
        j = self.rng.integers(0, V.shape[0], users.numel())
        Un, Vn = U.numpy(), V.numpy()                      # views: updated in place
        loss = mo.bpr_step_batch(Un, Vn, users.numpy(), items.numpy(), j, lr, l2)
        if loss_sum is not None:
            loss_sum += loss
        if neg_out is not None:
            neg_out[:users.numel()] = torch.from_numpy(j)


def _bpr_worker(rank, world, port, q, reduce, rows_per_launch, uneven, epochs, script):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')]
    import torch.distributed as dist
    from otto_amd.matrix_factorization.bpr import ItemTableSync, train_epoch
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    u, i, n_users, n_items = _planted_small()
    cut = [n_users * r // world for r in range(world + 1)]
    if uneven:                                              # session-chunk shards of different sizes
        cut = [0] + [min(n_users, c + 37 * (r + 1)) for r, c in enumerate(cut[1:-1])] + [n_users]
    mine = (u >= cut[rank]) & (u < cut[rank + 1])
    model = _CpuBpr(n_users, n_items, 16)
    du, di = torch.from_numpy(u[mine]), torch.from_numpy(i[mine])
    V = model.item_embedding.weight.data
    sync = ItemTableSync(V, reduce=reduce)
    losses = []
    if script == 'epochs':
        for e in range(epochs):
            losses.append(train_epoch(model, du, di, lr=0.2, seed=1, epoch=e, rows_per_launch=rows_per_launch,
                                      row0=int(np.flatnonzero(mine)[0]), sync=sync, sync_every=2))
    else:
        # one period with a launch that is NOT reported and one that is: the exchange must not drop the first one's rows
        sync.tracking = True
        eng, U = model, model.user_embedding.weight.data
        neg = torch.empty(len(du), dtype=torch.int64)
        eng.bpr_step(U, V, du[:3000], di[:3000], 1, 0, 0, 0.2, 0.0, 0, neg_out=neg)
        sync.untracked()
        eng.bpr_step(U, V, du[3000:3040], di[3000:3040], 1, 0, 0, 0.2, 0.0, 0, neg_out=neg)
        sync.touched(di[3000:3040], neg[:40])
        sync.finish()
    q.put((rank, V.numpy().copy(), losses, int(mine.sum()), dict(sync.stats)))
    dist.barrier()
    dist.destroy_process_group()


def _run_bpr(world, reduce='sum', rows_per_launch=1024, uneven=False, epochs=20, script='epochs'):
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_bpr_worker, args=(r, world, port, q, reduce, rows_per_launch, uneven, epochs, script))
             for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in procs))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def _single_rank_losses(rows_per_launch, epochs):
    sys.path[:0] = [os.path.join(ROOT, 'oracle')]
    from otto_amd.matrix_factorization.bpr import train_epoch
    u, i, n_users, n_items = _planted_small()
    model = _CpuBpr(n_users, n_items, 16)
    du, di = torch.from_numpy(u), torch.from_numpy(i)
    return [train_epoch(model, du, di, lr=0.2, seed=1, epoch=e, rows_per_launch=rows_per_launch) for e in range(epochs)]


def test_data_parallel_bpr_world4_loss_band_two_sided():
    """W = 4 ranks, session-chunk shards, the item table exchanged by ItemTableSync over gloo (dense, asynchronous: launches
    of 1024 rows > n_items / 4): the row-weighted mean loss of the last epoch is within +-10 % of the single-process run
    with reduce='sum' (every triplet's step applied once, as the single process applies it) and replicas are identical.
    reduce='mean' (model averaging) is the conservative variant: it must converge too, but more slowly -- its final
    loss lies ABOVE the single-process loss."""
    ref = _single_rank_losses(1024, 20)
    for reduce in ('sum', 'mean'):
        res = _run_bpr(4, reduce=reduce)
        for r in range(1, 4):
            assert np.array_equal(res[0][0], res[r][0]), 'item-table replicas differ after the drain'
        n = np.array([res[r][2] for r in range(4)], dtype=np.float64)
        loss = sum(np.array(res[r][1]) * n[r] for r in range(4)) / n.sum()
        assert loss[-1] < 0.2 * loss[0]
        if reduce == 'sum':
            assert 0.9 * ref[-1] <= loss[-1] <= 1.1 * ref[-1], (loss[-1], ref[-1])
        else:
            assert ref[-1] < loss[-1] <= 2.0 * ref[-1], (loss[-1], ref[-1])
        assert res[0][3]['dense'] > 0 and res[0][3]['sparse'] == 0


def test_data_parallel_bpr_unequal_shards_issue_the_same_collectives():
    """Shards of 300 + 37 r users: the ranks' launch counts differ (tracked launches of 128 rows: sparse exchanges, with a
    vote all-reduce each) -- a rank that runs out of rows must keep taking part in the exchange schedule. A mismatch hangs
    (the workers are joined with a timeout) or leaves different replicas."""
    res = _run_bpr(3, rows_per_launch=128, uneven=True, epochs=2)
    rows = [res[r][2] for r in range(3)]
    assert len({(n + 127) // 128 for n in rows}) > 1, rows          # the launch counts do differ
    for r in range(1, 3):
        assert np.array_equal(res[0][0], res[r][0])
    assert res[0][3]['dense'] + res[0][3]['sparse'] >= 2 * ((max(rows) + 127) // 128 // 2)   # every slot pair was exchanged


def test_item_table_sync_untracked_launch_makes_the_period_dense():
    """A period with one launch that was not reported to touched() and one that was: a sparse exchange would ship only
    the second launch's rows and the drain would then overwrite the first launch's updates with the common table. Every
    rank's replica must contain BOTH launches' deltas of every rank = the sum the dense path forms."""
    res = _run_bpr(2, script='period')
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][3] == {'dense': 1, 'sparse': 0}
    # reference: both ranks' deltas on the common start table, computed without any exchange machinery
    import mf_oracle as mo
    u, i, n_users, n_items = _planted_small()
    total = None
    for rank in range(2):
        lo, hi = n_users * rank // 2, n_users * (rank + 1) // 2
        mine = (u >= lo) & (u < hi)
        m = _CpuBpr(n_users, n_items, 16)
        V0 = m.item_embedding.weight.data.clone()
        du, di = torch.from_numpy(u[mine]), torch.from_numpy(i[mine])
        U, V = m.user_embedding.weight.data, m.item_embedding.weight.data
        m.bpr_step(U, V, du[:3000], di[:3000], 1, 0, 0, 0.2, 0.0, 0)
        m.bpr_step(U, V, du[3000:3040], di[3000:3040], 1, 0, 0, 0.2, 0.0, 0)
        total = (V - V0) if total is None else total + (V - V0)
    want = (V0 + total).numpy()
    assert np.allclose(res[0][0], want, rtol=0, atol=1e-6)
