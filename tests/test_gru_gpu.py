"""GRU4Rec on the device (SPEC-GRU4REC, include/otto_gru.h; otto_amd/recbole) against the NumPy restatement
(tests/gru_restatement.py): plans and negatives exactly; o and every gradient within the bands of tests/golden/gru_bounds.json
(4 x the float32-to-float64 distance of the restatement itself, measured on the CPU) of the float64 restatement; the Adam
updates within the project's fp32 band of the float32 restatement fed the device's own gradients, with every untouched row
bit for bit; determinism, the calling contract, the refusals, a training run, the learning fixture and the routing."""
import json
import os

import numpy as np
import pytest
import torch

import conftest
import gru_inputs as I
import gru_restatement as R
import gru_routing

pytestmark = pytest.mark.gpu
CANARY, PAD = 0x5A, 256
RTOL, ATOL = 1e-4, 1e-6                      # the project's fp32 band (tests/test_sgns_gpu.py)

with open(os.path.join(conftest.GOLDEN, 'gru_bounds.json')) as fh:
    BOUNDS = json.load(fh)
CASES = I.cases()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def distance(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return 0.0
    d, m = float(np.abs(a - b).max()), float(np.abs(b).max())
    return d / m if m > 0 else d


class Events:
    def __init__(self, dev, aid, sess_off, n_aids, typ=None):
        self.aid, self.sess_off, self.n_aids = _dev(aid, dev), _dev(sess_off, dev), n_aids
        self.type = _dev(np.zeros(len(aid), dtype=np.uint8) if typ is None else typ, dev)


def _model(dev, c, P=None):
    from otto_amd.recbole.gru4rec import GRU4Rec
    m = GRU4Rec(c['n_aids'], c['De'], c['H'])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in (c['P'] if P is None else P).items()})
    return m.to(dev)


class Canaried:
    """tensors cut out of canary-filled buffers; ``intact`` looks at what lies around them"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.uint8, device=self.dev)
        self.bufs.append((buf, n))
        return buf[PAD:PAD + n].view(dtype).reshape(shape)

    def intact(self):
        return all(bool((b[:PAD] == CANARY).all()) and bool((b[PAD + n:] == CANARY).all()) for b, n in self.bufs)


def _grads(dev, c, can, want_o=True):
    from otto_amd.recbole.gru4rec import DENSE, Grads
    De, H, B = c['De'], c['H'], len(c['seq_lo'])
    cap = max(1, min(B * (c['L'] + 2), c['n_aids']))
    f = torch.float32
    return Grads({DENSE[0]: can.new((3 * H, De), f), DENSE[1]: can.new((3 * H, H), f), DENSE[2]: can.new((De, H), f), DENSE[3]: can.new((De,), f)},
                 can.new((cap,), torch.int32), can.new((cap, De), f), can.new((1,), torch.int64), can.new((1,), torch.float64),
                 can.new((B, De), f) if want_o else None)


def _batch(dev, c):
    return [_dev(c[k], dev) for k in ('seq_lo', 'seq_len', 'target', 'neg')]


def _host(g):
    cnt = int(g.count[0])
    return ({k: v.cpu().numpy() for k, v in g.dense.items()}, g.ids[:cnt].cpu().numpy(), g.rows[:cnt].cpu().numpy(),
            float(g.loss_sum[0]), None if g.o is None else g.o.cpu().numpy())


def _check_case(dev, name):
    c, band = CASES[name], BOUNDS['cases'][name]
    ev = Events(dev, c['aid'], c['sess_off'], c['n_aids'])
    model = _model(dev, c)
    # the plan of the case's corpus: exact
    plan = model.plan_epoch(ev, I.SEED, I.EPOCH, c['L'])
    want = R.plan(c['aid'], c['sess_off'], c['n_aids'], I.SEED, I.EPOCH, c['L'])
    for got, w, what in zip((plan.p, plan.seq_lo, plan.seq_len, plan.target, plan.neg), want, ('p', 'seq_lo', 'seq_len', 'target', 'neg')):
        assert np.array_equal(got.cpu().numpy(), w), what
    # forward and gradients against the float64 restatement
    args = _batch(dev, c)
    can = Canaried(dev)
    G, loss, o64 = R.grad(c['P'], c['aid'], c['seq_lo'], c['seq_len'], c['target'], c['neg'])
    o = model.encode(ev.aid, args[0], args[1], c['L'], out=can.new(o64.shape, torch.float32)).cpu().numpy()
    g = model.grad(ev.aid, *args, c['L'], want_o=True, out=_grads(dev, c, can))
    dense, ids, rows, loss_sum, o_grad = _host(g)
    figures = {'o': distance(o, o64), 'o (grad)': distance(o_grad, o64)}
    figures.update({k: distance(dense[k], G[k]) for k in R.DENSE})
    want_ids, _ = R.export_list(G[R.KEYS[0]], c['aid'], c['seq_lo'], c['seq_len'], c['target'], c['neg'])
    assert np.array_equal(ids, want_ids) and (np.diff(ids) > 0).all() and (ids > 0).all()
    gE = np.zeros(G[R.KEYS[0]].shape, dtype=np.float32)
    gE[ids] = rows
    figures[R.KEYS[0]] = distance(gE, G[R.KEYS[0]])
    print(name, {k: f'{v:.2e}' for k, v in figures.items()}, 'loss', loss_sum, float(loss))
    for q, d in figures.items():
        assert d <= band[q.split(' ')[0]]['band'], (name, q, d, band[q.split(' ')[0]])
    assert abs(loss_sum - float(loss)) <= RTOL * abs(float(loss)) + ATOL
    # determinism: the same bytes again
    g2 = model.grad(ev.aid, *args, c['L'], want_o=True, out=_grads(dev, c, can))
    dense2, ids2, rows2, _, o2 = _host(g2)
    for a, b in zip([ids, rows, o_grad] + [dense[k] for k in R.DENSE], [ids2, rows2, o2] + [dense2[k] for k in R.DENSE]):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert float(g2.loss_sum[0]) == loss_sum
    # apply, fed the device's own gradients, against the float32 restatement fed the same
    state = R.new_state(c['P'], np.float32)
    before = {k: v.copy() for k, v in state['p'].items()}
    for t in (1, 2):
        model.apply(g, t=t, **I.ADAM)
        R.apply(state, dense, ids, rows, t=t, dtype=np.float32, **I.ADAM)
    got = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    m, v = model.moments()
    for k in R.KEYS:
        assert np.allclose(got[k], state['p'][k], rtol=RTOL, atol=ATOL), k
    assert np.allclose(m[0].cpu().numpy(), state['m'][R.KEYS[0]], rtol=RTOL, atol=ATOL)
    assert np.allclose(v[0].cpu().numpy(), state['v'][R.KEYS[0]], rtol=RTOL, atol=1e-12)
    untouched = np.setdiff1d(np.arange(c['n_aids'] + 1), ids)
    assert 0 in untouched
    assert np.array_equal(got[R.KEYS[0]][untouched].view(np.uint32), before[R.KEYS[0]][untouched].view(np.uint32))
    assert not m[0].cpu().numpy()[untouched].any() and not v[0].cpu().numpy()[untouched].any()
    assert can.intact()


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_step_on_the_edge_shapes(gpu_device, name):
    _check_case(gpu_device, name)


def test_truncation_forgets_the_first_events(gpu_device):
    dev = gpu_device
    c = I.length_case(3)
    first = int(c['sess_off'][-2])
    sel = (c['seq_len'] == 3) & (c['seq_lo'] > first)
    assert sel.any()
    other = c['aid'].copy()
    other[first:int(c['seq_lo'][sel].min())] = (other[first:int(c['seq_lo'][sel].min())] + 1) % c['n_aids']
    model = _model(dev, c)
    lo, n = _dev(c['seq_lo'][sel], dev), _dev(c['seq_len'][sel], dev)
    a, b = model.encode(_dev(c['aid'], dev), lo, n, 3), model.encode(_dev(other, dev), lo, n, 3)
    assert torch.equal(a, b)


def test_a_corpus_without_a_sample_is_a_no_op(gpu_device):
    from otto_amd.recbole import gru4rec
    dev = gpu_device
    c = I.no_samples()
    ev = Events(dev, c['aid'], c['sess_off'], c['n_aids'])
    model = _model(dev, c)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    plan = model.plan_epoch(ev, I.SEED, I.EPOCH, c['L'])
    assert len(plan) == 0
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    assert model.encode(ev.aid, empty, empty, c['L']).shape == (0, c['De'])
    g = model.grad(ev.aid, empty, empty, empty, empty, c['L'])
    assert int(g.count[0]) == 0 and float(g.loss_sum[0]) == 0.0 and all(not v.any() for v in g.dense.values())
    assert gru4rec.train_epoch(model, ev, batch=8, seed=I.SEED, epoch=I.EPOCH, max_len=c['L'], **I.ADAM) == 0.0
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and model.step_count == 0
    # an empty session and a session of one event encode to the bias and to one step
    o = model.encode_sessions(ev, c['L']).cpu().numpy()
    lens = np.diff(c['sess_off'])
    want = R.encode(c['P'], c['aid'], c['sess_off'][:-1], lens)
    assert np.array_equal(o[lens == 0], np.broadcast_to(c['P'][R.KEYS[4]], o[lens == 0].shape))
    assert distance(o, want) <= 1e-6


def test_refusals_leave_the_outputs_alone(gpu_device):
    import ctypes as C
    from otto_amd import _lib
    dev = gpu_device
    c = I.batch_case(4)
    model = _model(dev, c)
    E = len(c['aid'])
    bad_aid = c['aid'].copy()
    bad_aid[[7, 20]] = [c['n_aids'], -1]
    bad_off = c['sess_off'].copy()
    bad_off[3] = bad_off[2] - 1
    short_off = c['sess_off'].copy()
    short_off[-1] -= 1
    for aid, off, index, kind in ((bad_aid, c['sess_off'], 7, 2), (c['aid'], bad_off, 2, 1), (bad_aid, bad_off, 2, 1),
                                  (c['aid'], short_off, len(short_off) - 1, 1), (c['aid'], c['sess_off'] + 1, 0, 1)):
        assert R.check(aid, off, c['n_aids']) == (index, kind)
        with pytest.raises(_lib.OttoError) as e:
            model.plan_epoch(Events(dev, aid, off, c['n_aids']), 1, 0, c['L'])
        assert (e.value.index, e.value.kind) == (index, kind)
        # the C call itself, on canary-padded outputs
        can = Canaried(dev)
        outs = [can.new((E,), torch.int32) for _ in range(5)]
        for t in outs:
            t.fill_(-7)
        d_aid, d_off = _dev(aid, dev), _dev(off, dev)
        job = _lib.GruPlanJob(_lib.ptr(d_aid, dev), _lib.ptr(d_off, dev), E, len(off) - 1, c['n_aids'], c['L'], 0, 1, 0,
                              *(_lib.ptr(t, dev) for t in outs), None, 0, _lib.stream(dev))
        work = _lib.workspace(_lib.lib().otto_gru_plan_workspace(C.byref(job)), dev)
        job.d_work, job.work_bytes = _lib.ptr(work, dev), work.numel()
        n, err = np.full(1, 99, dtype=np.int64), np.zeros(2, dtype=np.int64)
        assert _lib.lib().otto_gru_plan(C.byref(job), n.ctypes.data_as(C.c_void_p), err.ctypes.data_as(C.c_void_p)) == -22
        assert n[0] == 0 and tuple(err) == (index, kind)
        assert all(bool((t == -7).all()) for t in outs) and can.intact()
    job = _lib.GruJob()
    job.De, job.H, job.B, job.max_len, job.n_aids = 48, 32, 1, 8, 10
    assert _lib.lib().otto_gru_workspace(C.byref(job), 0) == -22 and b'De' in _lib.lib().otto_last_error()


def _chain(model, ev, c, work=None):
    """plan, the first batch's gradients, one update, the encoding of every session: everything the model computes"""
    plan = model.plan_epoch(ev, I.SEED, I.EPOCH, c['L'], work=None if work is None else work[0])
    b = slice(0, c['batch'])
    g = model.grad(ev.aid, plan.seq_lo[b], plan.seq_len[b], plan.target[b], plan.neg[b], c['L'], want_o=True,
                   work=None if work is None else work[1])
    model.apply(g, t=1, **I.ADAM)
    return [plan.p, plan.neg, g.o, g.ids, g.rows, g.count, g.loss_sum, *g.dense.values(), *model.state_dict().values(),
            model.encode_sessions(ev, c['L'])]


def _same_bytes(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        if i in (3, 4):                                          # the list: its first count entries
            n = int(want[5][0])
            a, b = a[:n], b[:n]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), i


def test_reused_scratch_and_a_side_stream_with_late_inputs(gpu_device):
    dev = gpu_device
    c = I.training_corpus()
    decoy, _ = I.corpus(np.diff(c['sess_off']), c['n_aids'], 99)
    assert not np.array_equal(decoy, c['aid'])
    want = _chain(_model(dev, c), Events(dev, c['aid'], c['sess_off'], c['n_aids']), c)
    # scratch that other calls have dirtied, twice in a row
    work = [torch.empty(4 << 20, dtype=torch.uint8, device=dev), torch.empty(64 << 20, dtype=torch.uint8, device=dev)]
    for aid in (decoy, c['aid'], c['aid']):
        if aid is decoy:
            for w in work:
                w.random_(0, 256)                                # after that, what the call before left behind
        got = _chain(_model(dev, c), Events(dev, aid, c['sess_off'], c['n_aids']), c, work)
    _same_bytes(got, want)
    # a side stream: the inputs hold the decoy until a copy that is enqueued behind a delay
    ev = Events(dev, decoy, c['sess_off'], c['n_aids'])
    pinned = torch.from_numpy(c['aid']).pin_memory()
    model = _model(dev, c)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))        # about 30 ms
    side = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        ev.aid.copy_(pinned, non_blocking=True)
        got = _chain(model, ev, c, work)
    side.synchronize()
    assert e0.elapsed_time(e1) >= 10.0
    _same_bytes(got, want)


def test_three_training_steps(gpu_device):
    from otto_amd.recbole import gru4rec
    dev = gpu_device
    c = I.training_corpus()
    ev = Events(dev, c['aid'], c['sess_off'], c['n_aids'])
    model = _model(dev, c)
    loss = gru4rec.train_epoch(model, ev, batch=c['batch'], seed=I.SEED, epoch=I.EPOCH, max_len=c['L'], steps=3, **I.ADAM)
    state, losses = R.train(c['P'], c['aid'], c['sess_off'], c['n_aids'], c['batch'], I.ADAM['lr'], I.ADAM['betas'], I.ADAM['eps'], I.SEED,
                            I.EPOCH, c['L'], steps=3)
    n = len(R.plan(c['aid'], c['sess_off'], c['n_aids'], I.SEED, I.EPOCH, c['L'])[0])
    sizes = [min(c['batch'], n - q * c['batch']) for q in range(3)]
    want = float(np.dot(losses, sizes)) / sum(sizes)              # the mean over the samples, not over the batches
    assert model.step_count == 3 and abs(loss - want) <= RTOL * abs(want) + ATOL
    got = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    figures = {k: distance(got[k], state['p'][k]) for k in R.KEYS}
    print('three steps', figures)
    for k, d in figures.items():
        assert d <= BOUNDS['train'][k]['band'], (k, d, BOUNDS['train'][k])
    # the whole epoch: a last batch that is not full
    assert n % c['batch'] != 0
    model = _model(dev, c)
    gru4rec.train_epoch(model, ev, batch=c['batch'], seed=I.SEED, epoch=I.EPOCH, max_len=c['L'], **I.ADAM)
    state, _ = R.train(c['P'], c['aid'], c['sess_off'], c['n_aids'], c['batch'], I.ADAM['lr'], I.ADAM['betas'], I.ADAM['eps'], I.SEED,
                       I.EPOCH, c['L'], dtype=np.float32)
    assert model.step_count == -(-n // c['batch'])
    assert np.allclose(model.dense.weight.data.cpu().numpy(), state['p'][R.KEYS[3]], rtol=1e-2, atol=1e-4)


def test_the_device_learns_the_runs(gpu_device):
    from otto_amd.recbole import gru4rec
    dev = gpu_device
    L = I.LEARN
    aid, off = I.runs(L['n_sessions'], seed=7)
    ev = Events(dev, aid, off, L['n_aids'])
    model = _model(dev, dict(n_aids=L['n_aids'], De=L['De'], H=L['H']), P=I.learn_init())
    epoch = 0
    while model.step_count < L['steps']:
        gru4rec.train_epoch(model, ev, batch=L['batch'], lr=L['lr'], seed=I.SEED, epoch=epoch, max_len=L['L'],
                            steps=L['steps'] - model.step_count)
        epoch += 1
    p_aid, lo, n, answer = I.probe()
    o = model.encode(_dev(p_aid, dev), _dev(lo, dev), _dev(n, dev), L['L'])
    rows, _ = model.full_sort_topk(o, k=5)
    rate = float((rows.cpu().numpy() - 1 == answer[:, None]).any(axis=1).mean())
    print('top-5 hit rate', rate)
    assert rate >= L['bar'] == 0.9


def test_predictions_take_the_three_routes(gpu_device):
    from otto_amd.covisitation.candidates import recency_candidates
    from otto_amd.recbole import inference
    dev = gpu_device
    n_aids = 64
    rng = np.random.default_rng(3)
    sessions = [rng.permutation(40)[:19], rng.permutation(40)[:20], np.concatenate([np.arange(20), np.arange(5)]),   # 19, 20, 20 distinct
                np.array([3, 1, 3]), np.array([3, 50, 3]), np.array([], dtype=np.int64), np.array([61]), np.array([7])]
    aid = np.concatenate(sessions).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sessions])]).astype(np.int64)
    typ = rng.integers(0, 3, len(aid)).astype(np.uint8)
    known = np.ones(n_aids, dtype=bool)
    known[50:] = False
    ev = Events(dev, aid, off, n_aids, typ)
    model = _model(dev, dict(n_aids=n_aids, De=32, H=32), P=I.params(n_aids, 32, 32, 8))
    top = model.full_sort_topk(model.encode_sessions(ev, 50), 20)[0].cpu().numpy() - 1
    r_cand, _, r_n = recency_candidates(ev.aid, ev.type, ev.sess_off, curves=(inference.RECENCY_CURVE,), type_coef=inference.TYPE_COEFFICIENT)
    r_cand, r_n = r_cand[0].cpu().numpy(), r_n.cpu().numpy()
    nb_ids = np.full((n_aids, 4), -1, dtype=np.int32)
    nb_n = rng.integers(0, 5, n_aids).astype(np.int32)
    for a in range(n_aids):
        nb_ids[a, :nb_n[a]] = rng.permutation(n_aids)[:nb_n[a]]
    for table in (None, (_dev(nb_ids, dev), None, _dev(nb_n, dev))):
        pred, n, route = (x.cpu().numpy() for x in inference.predictions(model, ev, known=_dev(known, dev), neighbours=table))
        assert list(route) == [1, 0, 0, 1, 2, 2, 2, 1]
        for s, sess in enumerate(sessions):
            recency = r_cand[off[s]:off[s] + r_n[s]]
            want, w_route = gru_routing.route(sess, known, top[s], recency, None if table is None or not len(sess) else nb_ids[sess[-1]])
            assert w_route == route[s] and n[s] == len(want) and list(pred[s, :n[s]]) == want and (pred[s, n[s]:] == -1).all(), s
    # known defaults to the aids of the events themselves: nothing is unknown
    assert set(inference.predictions(model, ev)[2].cpu().numpy().tolist()) == {0, 1, 2}
