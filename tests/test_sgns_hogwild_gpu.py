"""k_sgns_step<false, *> (csrc/otto_sgns.hip), the HOGWILD skip-gram step, against the sequential loop of
tests/sgns_restatement.py / tests/sgns_hs_restatement.py wherever hogwild is deterministic (tests/sgns_hogwild_inputs.py):
one centre per launch at every lane-group size and target-list shape, the longest pair chain, maximal race-free launches
over several workgroups, and the grid-stride loop on a permutation. tests/test_sgns_hogwild_cpu.py shows that a float32 run
of the restatement uses at most 0.11 of the band these tests allow and that the bugs they are aimed at leave it by 100 x."""
import numpy as np
import pytest

import sgns_hogwild_inputs as hi
import sgns_hs_restatement as hr
import sgns_restatement as sr

pytestmark = pytest.mark.gpu
RTOL, ATOL = hi.RTOL, hi.ATOL       # test_sgns_gpu.py's band
LR = 0.05
PLAN_KEYS = ('tok_aid', 'tok_src', 'tok_off', 'radius', 'tok_left', 'pair_off')


def _sg():
    from otto_amd.gensim_fasttext import skipgram
    return skipgram


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_plan(plan, want):
    for k in PLAN_KEYS:
        got = getattr(plan, k).cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    assert plan.T == len(want['tok_aid']) and plan.P == int(want['pair_off'][-1])


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


def _launch(eng, plan, p, t0, t1, In, Out, lr, cum, neg, n_aids, seed, epoch, Syn1=None, mode=None):
    """one launch over [t0, t1); its contexts and negatives bit for bit against the restatement's sampler"""
    import torch
    sg = _sg()
    npair = int(p['pair_off'][t1] - p['pair_off'][t0])
    ctx = torch.full((max(npair, 1),), -7, dtype=torch.int32, device=In.device)
    ngo = torch.full((max(npair, 1), max(neg, 1)), -7, dtype=torch.int32, device=In.device)
    loss = eng.step(plan, t0, t1, In, Out, lr, sg.HOGWILD if mode is None else mode, ctx_out=ctx, neg_out=ngo if neg else None,
                    Syn1=Syn1)
    wc, wn = sr.negatives(p, cum, seed, epoch, neg, t0, t1, n_aids)
    assert np.array_equal(ctx.cpu().numpy()[:npair], wc), (t0, t1)
    if neg:
        assert np.array_equal(ngo.cpu().numpy()[:npair, :neg], wn), (t0, t1)
    return loss.item(), wc, wn


@pytest.fixture(scope='module')
def tiny():
    return hi.tiny_vocab()


@pytest.fixture(scope='module')
def chain():
    return hi.long_chain()


# ---------------------------------------------------------------------------
# shape A: one centre per launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('hs', [False, True])
@pytest.mark.parametrize('neg', hi.NEGS)
@pytest.mark.parametrize('d', hi.DIMS)
def test_one_centre_per_launch(gpu_device, tiny, d, neg, hs):
    sg = _sg()
    tv, n = tiny, tiny['n_aids']
    tree = hr.huffman(tv['count'], 1) if hs else None
    eng = sg.SkipGramEngine(n, d, tv['ws'], neg, tv['keep_q'], tv['weight'], seed=tv['seed'], device=gpu_device,
                            hs=_Tables(tree) if hs else None)
    In_h, Out_h = hi.tables(n, d, 1), hi.tables(n, d, 2)
    Syn_h = hi.tables(tree['n_inner'], d, 3) if hs else None
    In, Out = _dev(In_h, gpu_device), _dev(Out_h, gpu_device)
    Syn1 = _dev(Syn_h, gpu_device) if hs else None
    d_aid, d_off = _dev(tv['aid'], gpu_device), _dev(tv['sess_off'], gpu_device)
    band = _Band()
    for ep, p in enumerate(tv['plans']):
        plan = eng.plan(d_aid, d_off, ep)
        _check_plan(plan, p)
        lr = LR * (1 - 0.1 * ep)
        for c in range(plan.T):
            loss, _, _ = _launch(eng, plan, p, c, c + 1, In, Out, lr, tv['cum'], neg, n, tv['seed'], ep, Syn1=Syn1)
            if hs:
                want = hr.step_sequential_hs(p, tv['cum'], In_h, Out_h, Syn_h, tree, tv['seed'], ep, neg, lr, c, c + 1)
                band.rows(Syn1, Syn_h, f'Syn1 after epoch {ep} centre {c}')
            else:
                want = sr.step_sequential(p, tv['cum'], In_h, Out_h, tv['seed'], ep, neg, lr, c, c + 1)
            band.loss(loss, want, f'epoch {ep} centre {c}')
            band.rows(In, In_h, f'In after epoch {ep} centre {c}')
            band.rows(Out, Out_h, f'Out after epoch {ep} centre {c}')
    print(f'one centre per launch d {d} neg {neg} hs {hs}: largest band ratio {band.worst:.3f}')


@pytest.mark.parametrize('d', [4, 32, 128])
def test_longest_chain(gpu_device, chain, d):
    sg = _sg()
    lc, n, p = chain, chain['n_aids'], chain['plan']
    eng = sg.SkipGramEngine(n, d, lc['ws'], lc['neg'], lc['keep_q'], lc['weight'], seed=lc['seed'], device=gpu_device)
    plan = eng.plan(_dev(lc['aid'], gpu_device), _dev(lc['sess_off'], gpu_device), 0)
    _check_plan(plan, p)
    In_h, Out_h = hi.tables(n, d, 1), hi.tables(n, d, 2)
    In, Out = _dev(In_h, gpu_device), _dev(Out_h, gpu_device)
    band = _Band()
    assert int(p['pair_off'][lc['centres'][2] + 1] - p['pair_off'][lc['centres'][2]]) == 64
    for c in lc['centres']:
        loss, _, _ = _launch(eng, plan, p, c, c + 1, In, Out, LR, lc['cum'], lc['neg'], n, lc['seed'], 0)
        want = sr.step_sequential(p, lc['cum'], In_h, Out_h, lc['seed'], 0, lc['neg'], LR, c, c + 1)
        band.loss(loss, want, f'centre {c}')
        band.rows(In, In_h, f'In after centre {c}')
        band.rows(Out, Out_h, f'Out after centre {c}')
    print(f'longest chain d {d}: largest band ratio {band.worst:.3f}')


# ---------------------------------------------------------------------------
# shape B: maximal race-free launches
# ---------------------------------------------------------------------------
def _wide_setup(gpu_device, d, neg):
    sg = _sg()
    w = hi.wide_vocab(d, neg)
    eng = sg.SkipGramEngine(w['n_aids'], d, w['ws'], neg, w['keep_q'], w['weight'], seed=w['seed'], device=gpu_device)
    plan = eng.plan(_dev(w['aid'], gpu_device), _dev(w['sess_off'], gpu_device), 0)
    _check_plan(plan, w['plan'])
    sp = w['sparse']
    # the plan that is launched: one centre per session keeps its pairs (sgns_hogwild_inputs.wide_vocab)
    sparse = sg.Plan(tok_aid=plan.tok_aid, tok_src=plan.tok_src, tok_off=plan.tok_off, radius=plan.radius,
                     tok_left=_dev(sp['tok_left'], gpu_device), pair_off=_dev(sp['pair_off'], gpu_device), T=plan.T,
                     P=int(sp['pair_off'][-1]), epoch=0)
    return w, eng, sparse


@pytest.mark.parametrize('neg', hi.WIDE_NEGS)
@pytest.mark.parametrize('d', hi.DIMS)
def test_race_free_launches(gpu_device, d, neg):
    import torch
    w, eng, sparse = _wide_setup(gpu_device, d, neg)
    sp, n = w['sparse'], w['n_aids']
    In_h, Out_h = hi.tables(n, d, 1), hi.tables(n, d, 2)
    In0, Out0 = _dev(In_h, gpu_device), _dev(Out_h, gpu_device)
    In, Out = In0.clone(), Out0.clone()
    band = _Band()
    seen_in, seen_out = [], []
    for t0, t1 in w['cut']:
        loss, wc, wn = _launch(eng, sparse, sp, t0, t1, In, Out, LR, w['cum'], neg, n, w['seed'], 0)
        want = sr.step_sequential(sp, w['cum'], In_h, Out_h, w['seed'], 0, neg, LR, t0, t1)
        has_pairs = np.diff(sp['pair_off'][t0:t1 + 1]) > 0
        rows_in = np.unique(sp['tok_aid'][t0:t1][has_pairs]).astype(np.int64)
        rows_out = np.unique(np.concatenate((wc, wn.ravel()))).astype(np.int64)
        band.loss(loss, want, f'launch [{t0}, {t1})')
        band.rows(In[_dev(rows_in, gpu_device)], In_h[rows_in], f'In after launch [{t0}, {t1})')
        band.rows(Out[_dev(rows_out, gpu_device)], Out_h[rows_out], f'Out after launch [{t0}, {t1})')
        seen_in.append(rows_in)
        seen_out.append(rows_out)
    for M, M0, M_h, seen, name in ((In, In0, In_h, seen_in, 'In'), (Out, Out0, Out_h, seen_out, 'Out')):
        rows = np.unique(np.concatenate(seen))
        band.rows(M[_dev(rows, gpu_device)], M_h[rows], f'{name} at the end')
        untouched = torch.ones(n, dtype=torch.bool, device=gpu_device)
        untouched[_dev(rows, gpu_device)] = False
        assert int(untouched.sum()) == n - len(rows) > 0
        assert torch.equal(M[untouched], M0[untouched]), f'{name}: a row no centre names was written'
    longest = max(hi.active_in(sp, t0, t1) for t0, t1 in w['cut'])
    assert longest >= 2 * hi.gpb(d) + 1
    print(f'race-free launches d {d} neg {neg}: {len(w["cut"])} launches, longest {longest} centres with pairs of '
          f'{max(t1 - t0 for t0, t1 in w["cut"])} tokens; largest band ratio {band.worst:.3f}')


# ---------------------------------------------------------------------------
# shape C: the grid-stride loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('d', hi.PERM_DIMS)
def test_grid_stride_hogwild_and_batch(gpu_device, d):
    import torch
    sg = _sg()
    pm = hi.permutation(d)
    T = pm['T']
    assert T > hi.SG_GRID * hi.gpb(d)
    eng = sg.SkipGramEngine(T, d, 1, 0, pm['keep_q'], pm['weight'], seed=pm['seed'], device=gpu_device)
    plan = eng.plan(_dev(pm['aid'], gpu_device), _dev(pm['sess_off'], gpu_device), 0)
    _check_plan(plan, hi.permutation_plan(pm))
    In_0, Out_0 = hi.tables(T, d, 1), hi.tables(T, d, 2)
    In_h, Out_h = In_0.copy(), Out_0.copy()
    want, want_ctx = hi.permutation_step(pm, In_h, Out_h, hi.PERM_LR)
    # every centre but the lone last token moves its In row and its context's Out row
    assert (In_h != In_0).any(axis=1).sum() == T - 1 == (Out_h != Out_0).any(axis=1).sum()
    band = _Band()
    for mode, name in ((sg.HOGWILD, 'hogwild'), (sg.BATCH, 'batch')):
        In, Out = _dev(In_0, gpu_device), _dev(Out_0, gpu_device)
        ctx = torch.full((plan.P,), -7, dtype=torch.int32, device=gpu_device)
        loss = eng.step(plan, 0, T, In, Out, hi.PERM_LR, mode, ctx_out=ctx)
        assert np.array_equal(ctx.cpu().numpy(), want_ctx)
        band.loss(loss.item(), want, name)
        band.rows(In, In_h, f'In, {name}')
        band.rows(Out, Out_h, f'Out, {name}')
    print(f'grid stride d {d}: {T} centres in one launch; largest band ratio {band.worst:.3f}')


# ---------------------------------------------------------------------------
# nothing races, so nothing varies
# ---------------------------------------------------------------------------
def test_second_run_is_identical(gpu_device, tiny):
    import torch
    sg = _sg()
    # shape A: the centre of tiny_vocab with the most pairs, neg = 40
    tv, n, d, neg = tiny, tiny['n_aids'], 32, 40
    p = tv['plans'][0]
    c = int(np.argmax(np.diff(p['pair_off'])))
    eng = sg.SkipGramEngine(n, d, tv['ws'], neg, tv['keep_q'], tv['weight'], seed=tv['seed'], device=gpu_device)
    plan = eng.plan(_dev(tv['aid'], gpu_device), _dev(tv['sess_off'], gpu_device), 0)
    runs = []
    for _ in range(2):
        In, Out = _dev(hi.tables(n, d, 1), gpu_device), _dev(hi.tables(n, d, 2), gpu_device)
        loss = eng.step(plan, c, c + 1, In, Out, LR, sg.HOGWILD).item()
        runs.append((In, Out, loss))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert not torch.equal(runs[0][1], _dev(hi.tables(n, d, 2), gpu_device))
    # shape B: the longest race-free launch of wide_vocab(32, 5)
    w, eng, sparse = _wide_setup(gpu_device, 32, 5)
    t0, t1 = max(w['cut'], key=lambda ab: hi.active_in(w['sparse'], *ab))
    In_h, Out_h = hi.tables(w['n_aids'], 32, 1), hi.tables(w['n_aids'], 32, 2)
    runs = []
    for _ in range(2):
        In, Out = _dev(In_h, gpu_device), _dev(Out_h, gpu_device)
        loss = eng.step(sparse, t0, t1, In, Out, LR, sg.HOGWILD).item()
        runs.append((In, Out, loss))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert not torch.equal(runs[0][0], _dev(In_h, gpu_device))
