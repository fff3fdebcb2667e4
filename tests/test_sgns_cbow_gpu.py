"""SPEC-CBOW and SPEC-DOC2VEC on the device (otto_sgns_cbow_step, include/otto_sgns.h) against tests/sgns_cbow_restatement.py:
the batch step at every row width, negative count, arch and variant, with and without the tree and cut into launches; the edge
input; the hogwild step one centre (DBOW: one session) per launch; a race-free whole-epoch launch past the grid; refusals; the
stream and scratch guarantees of the job record; the driver; and what hogwild learns on the planted sessions."""
import ctypes as C
import os

import numpy as np
import pytest

import sgns_cbow_inputs as ci
import sgns_cbow_restatement as cr
import sgns_hogwild_inputs as hi
import sgns_hs_restatement as hr
import sgns_inputs as si
import sgns_restatement as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6             # test_sgns_gpu.py's band
N_STEP_AIDS = 400
IDS = [a[0] for a in ci.ARCHS]
TABLES = ('In', 'Out', 'Syn1', 'Doc')


def _sg():
    from otto_amd.gensim_fasttext import skipgram
    return skipgram


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Tables:
    """the restatement's tree in the shape SkipGramEngine(hs=...) takes"""

    def __init__(self, h):
        self.V, self.n_inner, self.max_len = h['V'], h['n_inner'], h['max_len']
        self.path_off, self.path_node = h['path_off'], h['path_node']
        self.code = np.array(h['code'], dtype=np.uint64)


class _Band:
    """asserts the band and keeps the largest ratio seen"""

    def __init__(self):
        self.worst = 0.0

    def rows(self, got, want, what):
        r = hi.band_ratio(got.cpu().numpy() if hasattr(got, 'cpu') else got, want)
        self.worst = max(self.worst, r)
        assert r <= 1.0, f'{what}: {r:.4g} x the band'

    def loss(self, got, want, what):
        r = abs(got - want) / (RTOL * abs(want) + ATOL)
        self.worst = max(self.worst, r)
        assert r <= 1.0, f'loss {what}: {got!r} against {want!r}, {r:.4g} x the band'


def _host_tables(n_aids, n_inner, S, d, seed=1):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-0.5, 0.5, (rows, d)).astype(np.float32) for k, rows in zip(TABLES, (n_aids, n_aids, n_inner, S))}


def _used(arch, hs):
    return [k for k in TABLES if not (k == 'In' and arch == cr.DBOW) and not (k == 'Doc' and arch == cr.CBOW) and not (k == 'Syn1' and not hs)]


class _Case:
    """an engine over `data` (aid, sess_off, keep_q, weight, cum, n_aids, seed, ws), the four tables on the host and on the
    device, and launches that are compared with the restatement one by one"""

    def __init__(self, dev, data, d, neg, hs, n_aids=None, table_seed=1):
        sg = _sg()
        self.dev, self.data, self.d, self.neg, self.hs = dev, data, d, neg, hs
        self.n = data['n_aids'] if n_aids is None else n_aids
        self.eng = sg.SkipGramEngine(self.n, d, data['ws'], neg, data['keep_q'], data['weight'], seed=data['seed'], device=dev,
                                     hs=None if hs is None else _Tables(hs))
        self.S = len(data['sess_off']) - 1
        self.d_aid, self.d_off = _dev(data['aid'], dev), _dev(data['sess_off'], dev)
        self.host = _host_tables(self.n, 1 if hs is None else hs['n_inner'], self.S, d, table_seed)
        self.devt = {k: _dev(v, dev) for k, v in self.host.items()}
        self.band = _Band()
        self.skipped = 0

    def plan(self, ep, p):
        plan = self.eng.plan(self.d_aid, self.d_off, ep)
        for k in ('tok_aid', 'tok_src', 'tok_off', 'tok_left', 'pair_off'):
            assert np.array_equal(getattr(plan, k).cpu().numpy(), p[k]), k
        return plan

    def launch(self, plan, p, ep, t0, t1, lr, mode, arch, variant, what=''):
        import torch
        sg = _sg()
        neg, hs, dt = self.neg, self.hs, self.devt
        used = _used(arch, hs is not None)
        ngo = torch.full((t1 - t0, max(neg, 1)), -7, dtype=torch.int32, device=self.dev)
        loss = self.eng.step_cbow(plan, t0, t1, dt['In'] if 'In' in used else None, dt['Out'], lr, arch, variant, mode,
                                  Syn1=dt['Syn1'] if hs is not None else None, Doc=dt['Doc'] if 'Doc' in used else None,
                                  neg_out=ngo if neg else None).item()
        sub = {k: self.host[k] for k in used}
        fn = cr.step_batch if mode == sg.BATCH else cr.step_sequential
        want = fn(p, self.data['cum'], sub, hs, self.data['seed'], ep, neg, lr, t0, t1, arch, variant)
        if neg:
            wn = cr.negatives(p, self.data['cum'], self.data['seed'], ep, neg, t0, t1, self.n)
            got = ngo.cpu().numpy()
            trained = np.array([arch != cr.CBOW or cr.n_inputs(p, c, arch) > 0 for c in range(t0, t1)])
            self.skipped += int((~trained).sum())
            assert np.array_equal(got[trained, :neg], wn[trained]), (what, t0, t1)      # bit for bit: the same draws, the same keys
            assert (got[~trained] == -7).all()                                          # a skipped centre writes nothing
        self.band.loss(loss, want, f'{what} [{t0}, {t1})')
        for k in TABLES:
            if k in used:
                self.band.rows(dt[k], self.host[k], f'{k} {what} [{t0}, {t1})')
            else:
                assert np.array_equal(dt[k].cpu().numpy(), self.host[k]), f'{k} is not a table of this arch and was written'
        return loss

    def workspaces_are_zero(self):
        e = self.eng
        for g in (*(e._grads or ()), e._gsyn1, e._gdoc):
            assert g is None or not bool(g.any())


# ---------------------------------------------------------------------------
# 1. batch step
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def step_data():
    # the sessions of test_sgns_gpu.py's step_data: 16 sessions, 400 aids, rows repeat heavily, some events subsampled
    rng = np.random.default_rng(8)
    lens = [9, 1, 2, 9, 5, 9, 3, 9, 9, 9, 4, 9, 9, 6, 9, 9]
    sess_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    aid = np.minimum(rng.zipf(1.2, sess_off[-1]) - 1, N_STEP_AIDS - 1).astype(np.int32)
    count, keep_q, weight = _sg().vocab_tables(aid, N_STEP_AIDS, 1, 0.05, 0.5)
    plans = [sr.plan(aid, sess_off, keep_q, 6, ep, 3) for ep in (0, 1)]
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight), plans=plans, n_aids=N_STEP_AIDS,
                seed=6, ws=3, hs=hr.huffman(count, 1))


def _run_batch(gpu_device, sd, d, neg, hs, arch, variant, cut=None):
    sg = _sg()
    case = _Case(gpu_device, sd, d, neg, sd['hs'] if hs else None)
    inside = False
    for ep, p in enumerate(sd['plans']):
        plan = case.plan(ep, p)
        step = plan.T if cut is None else cut
        for t0 in range(0, plan.T, step):
            t1 = min(t0 + step, plan.T)
            inside |= t1 < plan.T and t1 not in set(p['tok_off'].tolist())
            case.launch(plan, p, ep, t0, t1, 0.05 * (1 - 0.1 * ep), sg.BATCH, arch, variant, f'epoch {ep}')
    case.workspaces_are_zero()
    print(f'batch d {d} neg {neg} hs {hs} arch {arch} variant {variant} cut {cut}: largest band ratio {case.band.worst:.3f}')
    return case, inside


@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=IDS)
@pytest.mark.parametrize('d', [4, 32, 64, 128])
def test_batch_step_at_every_row_width(gpu_device, step_data, d, name, arch, variant):
    case, _ = _run_batch(gpu_device, step_data, d, 5, False, arch, variant)
    assert arch != cr.CBOW or case.skipped > 0                   # a one-token session: the centre CBOW skips


@pytest.mark.parametrize('name,arch,variant', [ci.ARCHS[1], ci.ARCHS[4]], ids=[IDS[1], IDS[4]])
@pytest.mark.parametrize('neg', [0, 1, 5, 40, 64])
def test_batch_step_at_every_negative_count(gpu_device, step_data, neg, name, arch, variant):
    _run_batch(gpu_device, step_data, 32, neg, neg == 0, arch, variant)        # neg = 0: the tree is the only objective beside the centre


@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=IDS)
def test_batch_step_with_the_tree(gpu_device, step_data, name, arch, variant):
    hs = step_data['hs']
    assert hs['V'] > 20 and hs['lens'].max() > 4 and (hs['lens'] == 0).any()     # out-of-vocabulary aids keep empty rows
    _run_batch(gpu_device, step_data, 32, 5, True, arch, variant)


@pytest.mark.parametrize('name,arch,variant', [ci.ARCHS[1], ci.ARCHS[4], ci.ARCHS[6]], ids=[IDS[1], IDS[4], IDS[6]])
@pytest.mark.parametrize('cut', [1, 7])
def test_batch_step_cut_into_launches(gpu_device, step_data, cut, name, arch, variant):
    _, inside = _run_batch(gpu_device, step_data, 32, 5, True, arch, variant, cut)
    assert inside                       # a launch boundary fell inside a session


# ---------------------------------------------------------------------------
# 2. the edge input
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def edge():
    return ci.edge_input()


@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=IDS)
def test_edge_input_batch(gpu_device, edge, name, arch, variant):
    sg = _sg()
    case = _Case(gpu_device, edge, 16, 3, edge['hs'])
    for ep, p in enumerate(edge['plans']):
        plan = case.plan(ep, p)
        case.launch(plan, p, ep, 0, plan.T, 0.05, sg.BATCH, arch, variant, f'edge epoch {ep}')
    case.workspaces_are_zero()
    assert arch != cr.CBOW or case.skipped == 2                  # the one-token session, once per epoch


def _units(p, arch):
    """the launches in which hogwild is the sequential loop: one centre, for DBOW one session"""
    if arch == cr.DBOW:
        return [(int(a), int(b)) for a, b in zip(p['tok_off'][:-1], p['tok_off'][1:]) if b > a]
    return [(c, c + 1) for c in range(len(p['tok_aid']))]


@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=IDS)
def test_edge_input_hogwild(gpu_device, edge, name, arch, variant):
    sg = _sg()
    case = _Case(gpu_device, edge, 16, 3, edge['hs'])
    p = edge['plans'][0]
    plan = case.plan(0, p)
    for t0, t1 in _units(p, arch):
        case.launch(plan, p, 0, t0, t1, 0.05, sg.HOGWILD, arch, variant, 'edge hogwild')
    print(f'edge hogwild {name}: largest band ratio {case.band.worst:.3f}')


# ---------------------------------------------------------------------------
# 3. hogwild, one centre (one session) per launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('hs', [False, True])
@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=IDS)
def test_hogwild_one_centre_per_launch(gpu_device, name, arch, variant, hs):
    _one_per_launch(gpu_device, 32, 5, hs, arch, variant)


@pytest.mark.parametrize('name,arch,variant', [ci.ARCHS[4], ci.ARCHS[6]], ids=[IDS[4], IDS[6]])
@pytest.mark.parametrize('d,neg', [(4, 40), (128, 3), (64, 0)])
def test_hogwild_one_centre_per_launch_at_other_shapes(gpu_device, d, neg, name, arch, variant):
    _one_per_launch(gpu_device, d, neg, neg == 0, arch, variant)


def _one_per_launch(gpu_device, d, neg, hs, arch, variant):
    sg = _sg()
    tv = hi.tiny_vocab()
    case = _Case(gpu_device, tv, d, neg, hr.huffman(tv['count'], 1) if hs else None)
    doubled = False
    for ep, p in enumerate(tv['plans']):
        plan = case.plan(ep, p)
        for c in range(plan.T):
            ctx = cr.context_aids(p, c)
            doubled |= len(set(ctx)) < len(ctx)
        for t0, t1 in _units(p, arch):
            case.launch(plan, p, ep, t0, t1, 0.25 * (1 - 0.1 * ep), sg.HOGWILD, arch, variant, f'epoch {ep}')
    assert doubled                      # tokens 1 and 2 are both aid 3: a context row that is read and written twice
    print(f'one per launch d {d} neg {neg} hs {hs} arch {arch} variant {variant}: largest band ratio {case.band.worst:.3f}')


# ---------------------------------------------------------------------------
# 4. a race-free whole-epoch launch past the grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('d', [4, 128])
def test_grid_stride_hogwild_and_batch(gpu_device, d):
    sg = _sg()
    pm = hi.permutation(d)
    T = pm['T']
    assert T > hi.SG_GRID * hi.gpb(d)                            # lane groups take a second centre
    eng = sg.SkipGramEngine(T, d, 1, 0, pm['keep_q'], pm['weight'], seed=pm['seed'], device=gpu_device)
    plan = eng.plan(_dev(pm['aid'], gpu_device), _dev(pm['sess_off'], gpu_device), 0)
    assert plan.T == T and np.array_equal(plan.pair_off.cpu().numpy(), hi.permutation_plan(pm)['pair_off'])
    start = ci.permutation_tables(pm, d)
    want = {k: v.copy() for k, v in start.items()}
    wl = ci.permutation_cbow_step(pm, want, hi.PERM_LR)
    assert all((want[k] != start[k]).any(axis=1).sum() == T - 1 for k in want)   # every centre but the lone last token
    band = _Band()
    for mode, name in ((sg.HOGWILD, 'hogwild'), (sg.BATCH, 'batch')):
        for variant in (sg.CBOW_SUM, sg.CBOW_MEAN):             # n = 1: the mean is the sum
            In, Out = _dev(start['In'], gpu_device), _dev(start['Out'], gpu_device)
            loss = eng.step_cbow(plan, 0, T, In, Out, hi.PERM_LR, sg.ARCH_CBOW, variant, mode)
            band.loss(loss.item(), wl, name)
            band.rows(In, want['In'], f'In, {name}')
            band.rows(Out, want['Out'], f'Out, {name}')
    print(f'grid stride d {d}: {T} centres in one launch; largest band ratio {band.worst:.3f}')


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_tables_unwritten(gpu_device, step_data):
    import torch
    from otto_amd import _lib
    sg = _sg()
    sd, hs, d, neg = step_data, step_data['hs'], 32, 5
    case = _Case(gpu_device, sd, d, neg, hs)
    eng, dt = case.eng, case.devt
    plan = case.plan(0, sd['plans'][0])
    grads = tuple(torch.zeros(dt[k].shape, dtype=torch.float64, device=gpu_device) for k in TABLES)
    grads = (grads[0], grads[1], grads[2], grads[3])            # gin, gout, gsyn1, gdoc
    loss = torch.full((1,), -3.0, dtype=torch.float64, device=gpu_device)
    ngo = torch.full((plan.T, neg), -7, dtype=torch.int32, device=gpu_device)

    def job(arch=sg.ARCH_PVDM, mode=sg.BATCH, **edit):
        j = eng._cbow_job(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, arch, sg.CBOW_MEAN, mode, dt['Syn1'], dt['Doc'], ngo, loss, grads)
        for k, v in edit.items():
            if k == 'total':
                j.table.total = v
            else:
                setattr(j, k, v)
        return j

    bad = [job(arch=3), job(arch=-1), job(variant=3), job(arch=sg.ARCH_CBOW, variant=-1), job(mode=2),
           job(d=12), job(d=0), job(d=6), job(d=256), job(neg=-1), job(neg=65),
           job(total=0), job(n_aids=1),
           job(d_Doc=None), job(arch=sg.ARCH_DBOW, d_Doc=None), job(arch=sg.ARCH_DBOW, d_tok_off=None), job(d_In=None),
           job(arch=sg.ARCH_CBOW, d_gin=None), job(d_gout=None), job(d_gdoc=None), job(arch=sg.ARCH_DBOW, d_gdoc=None), job(d_gsyn1=None),
           job(t0=5, t1=4), job(t1=plan.T + 1), job(t0=-1), job(T=plan.T - 1),
           job(d_code=None), job(d_path_off=None), job(d_Syn1=None), job(n_inner=0), job(d_loss_sum=None)]
    for j in bad:
        with pytest.raises(_lib.OttoError, match=r'code -22'):
            _lib.call('otto_sgns_cbow_step', gpu_device, C.byref(j), stream=False)
    for wrapper_bad in (lambda: eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, 5, Syn1=dt['Syn1']),
                        lambda: eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, sg.ARCH_CBOW, 7, Syn1=dt['Syn1']),
                        lambda: eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, sg.ARCH_PVDM, Syn1=dt['Syn1']),       # no Doc
                        lambda: eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, sg.ARCH_CBOW),                        # no Syn1
                        lambda: eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, sg.ARCH_DBOW, Syn1=dt['Syn1'],
                                              Doc=dt['Doc'][:-1].contiguous())):
        with pytest.raises(ValueError):
            wrapper_bad()
    for k in TABLES:
        assert np.array_equal(dt[k].cpu().numpy(), case.host[k]), k
    assert all(not bool(g.any()) for g in grads) and loss.item() == -3.0 and bool((ngo == -7).all())
    # the same records with everything in place run
    _lib.call('otto_sgns_cbow_step', gpu_device, C.byref(job()), stream=False)
    assert all(not np.array_equal(dt[k].cpu().numpy(), case.host[k]) for k in TABLES) and loss.item() > 0
    assert all(not bool(g.any()) for g in grads)
    before = dt['In'].clone()
    _lib.call('otto_sgns_cbow_step', gpu_device, C.byref(job(arch=sg.ARCH_DBOW, variant=99, d_In=None, d_gin=None)), stream=False)
    assert torch.equal(dt['In'], before) and all(not bool(g.any()) for g in grads)
    # an empty range writes the loss 0 and nothing else
    snap = {k: dt[k].clone() for k in TABLES}
    _lib.call('otto_sgns_cbow_step', gpu_device, C.byref(job(t0=4, t1=4)), stream=False)
    assert loss.item() == 0.0 and all(torch.equal(dt[k], snap[k]) for k in TABLES)


# ---------------------------------------------------------------------------
# 6. stream and scratch: the contract of tests/contract_cases.py for the job record
# ---------------------------------------------------------------------------
def _contract_want(sd, d, neg, seed, t0, t1):
    host = _host_tables(N_STEP_AIDS, sd['hs']['n_inner'], len(sd['sess_off']) - 1, d, seed)
    want = {k: v.copy() for k, v in host.items()}
    loss = cr.step_batch(sd['plans'][0], sd['cum'], want, sd['hs'], sd['seed'], 0, neg, 0.05, t0, t1, cr.PVDM, cr.MEAN)
    return host, want, loss


def test_reused_scratch_and_repetition(gpu_device, step_data):
    sg = _sg()
    sd, d, neg = step_data, 32, 5
    case = _Case(gpu_device, sd, d, neg, sd['hs'])
    plan = case.plan(0, sd['plans'][0])
    T = plan.T
    band = _Band()

    def run(seed, t0, t1):
        host, want, wl = _contract_want(sd, d, neg, seed, t0, t1)
        dt = {k: _dev(v, gpu_device) for k, v in host.items()}
        loss = case.eng.step_cbow(plan, t0, t1, dt['In'], dt['Out'], 0.05, sg.ARCH_PVDM, sg.CBOW_MEAN, sg.BATCH, Syn1=dt['Syn1'], Doc=dt['Doc'])
        band.loss(loss.item(), wl, f'seed {seed} [{t0}, {t1})')
        for k in TABLES:
            band.rows(dt[k], want[k], f'{k}, seed {seed} [{t0}, {t1})')
        case.workspaces_are_zero()

    run(1, 0, T // 2)
    run(1, 0, T // 2)                   # twice in a row
    run(2, 0, T // 2)                   # a decoy of the same size
    run(1, 0, T // 2)
    run(2, 0, T)                        # one of twice the size
    run(1, 0, T // 2)
    # and the skip-gram entry, which shares the loss partials and the apply kernel, in between
    In, Out, Syn1 = (_dev(case.host[k], gpu_device) for k in ('In', 'Out', 'Syn1'))
    case.eng.step(plan, 0, T, In, Out, 0.05, sg.BATCH, Syn1=Syn1)
    run(1, 0, T // 2)


def test_side_stream_with_late_inputs(gpu_device, step_data):
    """The tables hold a decoy; on a side stream a delay is followed by the copy of the real tables and by the step. An entry
    point that launched on another stream than the job's would read the decoy."""
    import torch
    sg = _sg()
    sd, d, neg = step_data, 32, 5
    case = _Case(gpu_device, sd, d, neg, sd['hs'])
    plan = case.plan(0, sd['plans'][0])
    host, want, wl = _contract_want(sd, d, neg, 1, 0, plan.T)
    decoy = _host_tables(N_STEP_AIDS, sd['hs']['n_inner'], case.S, d, 2)
    torch.cuda._sleep(1_000_000)                             # the first launch of the delay kernel is not the measured one
    torch.cuda.synchronize(gpu_device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                               # about 30 ms
    dt = {k: _dev(v, gpu_device) for k, v in decoy.items()}
    pinned = {k: torch.from_numpy(v.copy()).pin_memory() for k, v in host.items()}
    loss = torch.zeros(1, dtype=torch.float64, device=gpu_device)
    case.eng.step_cbow(plan, 0, 0, dt['In'], dt['Out'], 0.05, sg.ARCH_PVDM, sg.CBOW_MEAN, sg.BATCH, Syn1=dt['Syn1'], Doc=dt['Doc'])   # workspaces exist
    torch.cuda.synchronize(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        for k in TABLES:
            dt[k].copy_(pinned[k], non_blocking=True)
        case.eng.step_cbow(plan, 0, plan.T, dt['In'], dt['Out'], 0.05, sg.ARCH_PVDM, sg.CBOW_MEAN, sg.BATCH, Syn1=dt['Syn1'], Doc=dt['Doc'],
                           loss=loss)
    side.synchronize()
    print(f'sgns cbow: the delay in front of the late inputs took {e0.elapsed_time(e1):.1f} ms')
    assert e0.elapsed_time(e1) >= 10.0
    band = _Band()
    band.loss(loss.item(), wl, 'side stream')
    for k in TABLES:
        band.rows(dt[k], want[k], f'{k}, side stream')
        assert hi.band_ratio(want[k], decoy[k]) > 1
    case.workspaces_are_zero()


# ---------------------------------------------------------------------------
# 7. the driver
# ---------------------------------------------------------------------------
def test_driver_writes_its_files_for_cbow_and_doc2vec(gpu_device, tmp_path, monkeypatch):
    import pandas as pd
    from otto_amd import settings
    from otto_amd.gensim_fasttext import trainer
    sg = _sg()
    aid, sess_off, _ = si.planted_sessions()
    S = len(sess_off) - 1
    session = np.repeat(np.arange(S) * 3 + 11, np.diff(sess_off))
    df = pd.DataFrame({'session': session.astype(np.int32), 'aid': aid, 'ts': np.arange(len(aid), dtype=np.int64) + 1_600_000_000,
                       'type': np.zeros(len(aid), dtype=np.uint8)})
    monkeypatch.setattr(settings, 'MODELS', tmp_path / 'models')
    gensim = dict(vector_size=32, alpha=0.025, window=3, min_count=1, sample=0.003, seed=42, workers=32, min_alpha=0.0001, negative=5,
                  ns_exponent=0.75, epochs=1)
    configs = {'fasttext_cbow': ('FastText', dict(model='cbow', lr=0.05, dim=32, ws=3, epoch=1, minCount=1, minn=0, maxn=0, neg=5, loss='ns',
                                                  t=0.003)),
               'word2vec_cbow': ('Word2Vec', {**gensim, 'sg': 0, 'cbow_mean': 0, 'hs': 1}),
               'doc2vec_dm': ('Doc2Vec', {**gensim, 'dm': 1, 'dm_mean': None}),
               'doc2vec_dbow': ('Doc2Vec', {**gensim, 'dm': 0, 'hs': 1, 'negative': 0})}
    aid_tables = {}
    for name, (model, args) in configs.items():
        config = {'model': {'model_name': model, 'model_args': args}, 'persistence': {'model_directory': name}}
        first, losses, root = trainer.run(config, df=df, device=str(gpu_device), n_aids=si.N_AIDS, tokens_per_launch=1000)
        assert root == tmp_path / 'models' / name and len(losses) == 1 and np.isfinite(losses[0]) and losses[0] > 0
        files = sorted(f.name for f in root.iterdir())
        if model == 'Doc2Vec':
            doc = np.load(root / 'doc_embeddings.npy')
            assert doc.dtype == np.float32 and doc.shape == (S, 32) and np.array_equal(doc, first) and np.isfinite(doc).all()
            assert not np.array_equal(doc, sg.init_doc(S, 32, 42))                  # trained
            assert np.array_equal(np.load(root / 'doc_sessions.npy'), np.arange(S) * 3 + 11)
        if name == 'doc2vec_dbow':
            assert files == ['doc_embeddings.npy', 'doc_sessions.npy']              # DBOW writes no aid files
            continue
        assert files == sorted(['aid_embeddings.npy', 'aid_embeddings.vec'] + (['doc_embeddings.npy', 'doc_sessions.npy'] if model == 'Doc2Vec' else []))
        saved = np.load(root / 'aid_embeddings.npy')
        assert saved.dtype == np.float32 and saved.shape == (si.N_AIDS, 32) and np.isfinite(saved).all()
        if model != 'Doc2Vec':
            assert np.array_equal(saved, first)
        aids, vec = sg.load_vec(root / 'aid_embeddings.vec')
        assert len(aids) == si.N_AIDS
        np.testing.assert_allclose(vec, saved[aids], rtol=5e-6, atol=0)
        aid_tables[name] = saved
    assert not np.array_equal(aid_tables['word2vec_cbow'], aid_tables['doc2vec_dm'])


# ---------------------------------------------------------------------------
# 8. hogwild learns the planted clusters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name,arch,variant,epochs', ci.LEARN, ids=[a[0] for a in ci.LEARN])
def test_hogwild_learns_the_planted_clusters(gpu_device, name, arch, variant, epochs):
    """The rule of test_sgns_hs_gpu.py's test: purity >= min - (max - min) of the purities the sequential restatement
    reaches over GOLDEN_SEEDS (tests/golden/make_sgns_cbow_golden.py), in hogwild launches of 16 tokens.

    Measured on an MI355X: cbow_mean In 0.8720 against a bound of 0.8127; pvdm_mean In 0.9992 against 0.9987 and Doc 0.9973
    against 0.9926; dbow Doc 1.0000 against 1.0000. CBOW-mean is on the steep part of its curve after three epochs and is
    the case that shows a lost update: with plain stores for the input rows it reached 0.21, with plain stores for the
    target rows alone 0.797 (0.757 - 0.821 over the five seeds), and with the float32 atomic adds of SPEC-CBOW's HOGWILD mode
    what a batch step of 16 tokens reaches (0.871)."""
    import torch
    from otto_amd.matrix_factorization.neighbours import neighbour_table
    sg = _sg()
    g = np.load(os.path.join(GOLDEN, 'sgns_cbow_golden.npz'))
    aid, sess_off, cluster = si.planted_sessions()
    kw = dict(dim=si.DIM, ws=si.WS, neg=si.NEG, epochs=epochs, lr=si.LR, t=si.T, min_count=si.MIN_COUNT, ns_exponent=si.NS_EXPONENT,
              seed=int(si.GOLDEN_SEEDS[0]), mode=sg.HOGWILD, tokens_per_launch=si.TOKENS_PER_LAUNCH)
    d_aid, d_off = _dev(aid, gpu_device), _dev(sess_off, gpu_device)
    if arch == cr.CBOW:
        In, Out, losses = sg.train_cbow(d_aid, d_off, si.N_AIDS, variant=variant, **kw)
        Doc = None
    else:
        Doc, In, Out, losses = sg.train_doc2vec(d_aid, d_off, si.N_AIDS, dm=int(arch == cr.PVDM), dm_mean=1, **kw)
    assert losses[0] > losses[-1] and all(np.isfinite(losses)), losses
    assert all(bool(torch.isfinite(M).all()) for M in (In, Out) + (() if Doc is None else (Doc,)))
    if arch == cr.DBOW:
        assert np.array_equal(In.cpu().numpy(), sg.init_tables(si.N_AIDS, si.DIM, kw['seed'])[0])      # never touched
    for kind, M, clusters in (('aid', In, cluster), ('doc', Doc, ci.doc_clusters(aid, sess_off, cluster))):
        key = f'{name}_{kind}_purity'
        if key not in g.files:
            continue
        recorded = g[key]
        assert len(recorded) == 5 and recorded.min() >= 0.5      # chance is 1/12
        ids, _, _ = neighbour_table(M, k=10, metric='euclidean')
        purity = si.purity_from_ids(ids.cpu().numpy(), clusters)
        bound = recorded.min() - (recorded.max() - recorded.min())
        print(f'{name} {kind} purity {purity:.4f}, recorded {recorded}, bound {bound:.4f}, losses {losses}, '
              f'restatement losses {g[name + "_losses"][0]}')
        assert purity >= bound, (name, kind, purity, recorded)
