"""Edge-shape parity tests of the MF trainer kernels (csrc/otto_mf.hip: SparseAdam step, eval, the running validation sums,
BPR) against the NumPy oracle: every factor size (d = 4 puts 64 lane groups in a wave, d = 256 one), both losses on both
table modes, batches around one block's worth of groups and with a second, partly filled grid-stride trip, the duplicate
structures of ``tests/mf_inputs.py`` and an engine whose ``max_batch`` exceeds the batch. tests/test_mf_inputs_cpu.py checks
on the CPU that every input used here has the property it is used for.

Bands (the project's own): 1e-4 relative (BASELINE.json north star) on losses and sums and as a relative NORM band on every
table, m and v included -- m is linear and v quadratic in the coalesced gradient, so a lost or doubled occurrence shows
there first; element-wise 1e-3 / 2e-5 as in test_mf_gpu.py. Every test prints the largest fraction of its bands it used."""
import ctypes as C

import numpy as np
import pytest

import mf_inputs as mi
import mf_oracle as mo

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ELEM_RTOL, ELEM_ATOL = 1e-3, 2e-5
PRED_ATOL = 1e-5            # test_forward_all_factor_sizes
BPR_ATOL = 1e-6             # test_bpr_negatives_and_batch_step_vs_oracle
BETAS, EPS = (0.9, 0.999), 1e-8
NAMES = ('E1', 'm1', 'v1', 'E2', 'm2', 'v2')


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Bands:
    """Collects the largest observed error / band per kind of band; asserts at the end so that every figure is printed."""

    def __init__(self, group):
        self.group, self.used, self.where = group, {}, {}

    def add(self, band, ratio, where=''):
        ratio = float(ratio)
        if not np.isfinite(ratio):                          # NaN or inf anywhere is the worst and stays the worst
            ratio = np.inf
        if ratio > self.used.get(band, -1.0):
            self.used[band], self.where[band] = ratio, where

    def scalar(self, band, got, want, where=''):
        self.add(band, abs(got - want) / (RTOL * abs(want)) if want else (0.0 if got == want else np.inf), where)

    def table(self, name, a, ref, where=''):
        nr, err = np.linalg.norm(ref.astype(np.float64)), np.linalg.norm(a.astype(np.float64) - ref)
        self.add('norm', err / (RTOL * nr) if nr else (0.0 if err == 0 else np.inf), f'{name} {where}')
        self.add('element', np.max(np.abs(a.astype(np.float64) - ref) / (ELEM_ATOL + ELEM_RTOL * np.abs(ref))), f'{name} {where}')

    def close(self, band, a, ref, rtol, atol, where=''):
        self.add(band, np.max(np.abs(a.astype(np.float64) - ref) / (atol + rtol * np.abs(ref))) if a.size else 0.0, where)

    def finish(self):
        print(f'[bands {self.group}] ' + ' '.join(f'{k}={v:.3g}' for k, v in sorted(self.used.items())))
        for k, v in self.used.items():
            assert v <= 1.0, f'{k} band exceeded {v:.3g}x at {self.where[k]}'


def _state(s, dev):
    """Device copies of a sequence's initial (E1, m1, v1, E2, m2, v2); a shared table is one tensor under both names."""
    import torch
    E1 = _t(s.E1, dev)
    m1, v1 = torch.zeros_like(E1), torch.zeros_like(E1)
    if s.shared:
        return [E1, m1, v1, E1, m1, v1]
    E2 = _t(s.E2, dev)
    return [E1, m1, v1, E2, torch.zeros_like(E2), torch.zeros_like(E2)]


def _run_sequence(s, dev, bands, max_batch=None):
    """All steps of a sequence on ONE engine; loss, tables and moments against the oracle after every step."""
    import torch
    from otto_amd.matrix_factorization.engine import MFEngine
    eng = MFEngine(s.n1, s.n2, s.d, max_batch or max(len(st[0]) for st in s.steps), shared_table=s.shared, device=dev)
    dv = _state(s, dev)
    loss = torch.zeros(1, device=dev)
    for k, ((i1, i2, tg), want) in enumerate(zip(s.steps, s.want)):
        eng.step_sparse_adam(*dv, _t(i1, dev), _t(i2, dev), _t(tg, dev), mi.KINDS.index(s.kind), mi.LR, BETAS, EPS, k + 1, loss)
        eng.check()
        bands.scalar('loss', loss.item(), want[0], f'step {k + 1}')
        for name, got, ref in zip(NAMES, dv, want[1:]):
            bands.table(name, got.cpu().numpy(), ref, f'step {k + 1}')
    return eng, dv


# ---------------------------------------------------------------------------------------------------------------------
# a. SparseAdam: factor size x loss x table mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,kind,shared,dup', mi.MATRIX_CASES)
def test_sparse_adam_every_factor_size_loss_and_table_mode(gpu_device, d, kind, shared, dup):
    """Three consecutive steps on one engine, B = 3 gpb + 2 twice and then gpb + 1 < max_batch: a role or slot of the larger
    batch that the smaller one read (an index computed with max_batch in place of B) would show in the third step. A counter
    left at 1 would NOT: the row's next first arriver then takes the slot path, which gives the same bits, so 'counters are
    zero between steps' cannot be observed through the step's outputs."""
    bands = Bands('a')
    _run_sequence(mi.matrix_seq(d, kind, shared, dup), gpu_device, bands)
    bands.finish()


# ---------------------------------------------------------------------------------------------------------------------
# b. batch edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,B,dup', mi.EDGE_CASES)
def test_step_and_eval_at_batch_edges(gpu_device, d, B, dup):
    """One step at B = 1, around one block's worth of groups and at the smallest batch with a second, partly filled trip;
    then ``eval`` of the same ids on the tables the step left, against the oracle on exactly those tables."""
    import torch
    bands = Bands('b')
    s = mi.edge_seq(d, B, dup)
    eng, dv = _run_sequence(s, gpu_device, bands)
    i1, i2, tg = s.steps[0]
    loss = torch.zeros(1, device=gpu_device)
    pred = torch.full((B,), 7.0, device=gpu_device)
    eng.eval(dv[0], dv[3], _t(i1, gpu_device), _t(i2, gpu_device), _t(tg, gpu_device), 0, loss, pred)
    eng.check()
    E1, E2 = dv[0].cpu().numpy(), dv[3].cpu().numpy()
    want_loss, _ = mo.eval_batch(E1, E2, i1, i2, tg, 'MSELoss')
    want_pred = (E1[i1].astype(np.float64) * E2[i2].astype(np.float64)).sum(1)
    bands.scalar('loss', loss.item(), want_loss, 'eval')
    bands.close('pred', pred.cpu().numpy(), want_pred, RTOL, PRED_ATOL, 'eval')
    bands.finish()


@pytest.mark.parametrize('d,B', mi.IDENTICAL_CASES)
def test_duplicate_free_step_is_byte_identical_run_to_run(gpu_device, d, B):
    """No row occurs twice, so no float atomic runs: two steps from the same state must agree in every byte."""
    import torch
    from otto_amd.matrix_factorization.engine import MFEngine
    s = mi.edge_seq(d, B, 'none')
    i1, i2, tg = (_t(x, gpu_device) for x in s.steps[0])
    runs = []
    for _ in range(2):
        eng = MFEngine(s.n1, s.n2, d, B, device=gpu_device)
        dv = _state(s, gpu_device)
        loss = torch.zeros(1, device=gpu_device)
        eng.step_sparse_adam(*dv, i1, i2, tg, 0, mi.LR, BETAS, EPS, 1, loss)
        eng.check()
        runs.append(dv + [loss])
    for name, a, b in zip(NAMES + ('loss',), *runs):
        assert torch.equal(a, b), name
    assert not torch.equal(runs[0][0], _t(s.E1, gpu_device)), 'the step moved nothing'


# ---------------------------------------------------------------------------------------------------------------------
# c. duplicate structures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dup,d,shared', mi.DUP_CASES)
def test_sparse_adam_duplicate_structures(gpu_device, dup, d, shared):
    """No duplicate at all (Adam in registers only), every row exactly one second arriver, one row taking the whole batch."""
    bands = Bands('c')
    s = mi.dup_seq(dup, d, shared)
    _, dv = _run_sequence(s, gpu_device, bands)
    if dup == 'one_row':
        i1, i2, _ = s.steps[0]
        for name, got, init, rows in zip(NAMES, dv, (s.E1, None, None, s.E2, None, None), (i1, i1, i1, i2, i2, i2)):
            a = got.cpu().numpy()
            out = np.setdiff1d(np.arange(a.shape[0]), np.r_[i1, i2] if shared else rows)
            assert len(out) >= 3
            want = init[out] if init is not None else np.zeros_like(a[out])
            assert np.array_equal(a[out].view(np.uint32), want.view(np.uint32)), f'{name}: a row outside the batch changed'
    bands.finish()


# ---------------------------------------------------------------------------------------------------------------------
# d. validation sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,kind,shared', mi.SUMS_CASES)
def test_validation_sums_accumulate_across_launches_and_reset(gpu_device, d, kind, shared):
    import torch
    from otto_amd.matrix_factorization.engine import MFEngine
    bands = Bands('d')
    s = mi.sums_case(d, kind, shared)
    code = mi.KINDS.index(kind)
    dev = gpu_device
    eng = MFEngine(s.n1, s.n2, d, max(len(b[0]) for b in s.batches), shared_table=shared, device=dev)
    E1 = _t(s.E1, dev)
    E2 = E1 if shared else _t(s.E2, dev)
    loss = torch.zeros(1, device=dev)
    total = np.zeros(4)

    def launch(k, with_pred, sums=True):
        i1, i2, tg = s.batches[k]
        pred = torch.full((len(i1),), 7.0, device=dev) if with_pred else None
        (eng.eval_sums if sums else eng.eval)(E1, E2, _t(i1, dev), _t(i2, dev), _t(tg, dev), code, loss, pred)
        eng.check()
        bands.scalar('loss', loss.item(), mo.eval_batch(s.E1, s.E2, i1, i2, tg, kind)[0], f'launch {k}')
        if with_pred:
            want = (s.E1[i1].astype(np.float64) * s.E2[i2].astype(np.float64)).sum(1)
            bands.close('pred', pred.cpu().numpy(), want, RTOL, PRED_ATOL, f'launch {k}')
        if sums:
            total[:] += mo.eval_sums(s.E1, s.E2, i1, i2, tg, kind)

    def compare(got, where):
        bands.scalar('sums', got[0], total[0], where + ' sum|e|')
        bands.scalar('sums', got[1], total[1], where + ' sum e^2')
        assert got[2] == total[2] and got[3] == total[3], (where, got, total.tolist())

    launch(0, with_pred=False)
    launch(1, with_pred=True)
    second = eng.read_sums(reset=False)
    compare(second, 'after two launches')
    launch(3, with_pred=True, sums=False)                  # a plain eval in between leaves the sums alone
    assert eng.read_sums(reset=False) == second
    launch(2, with_pred=True)
    compare(eng.read_sums(reset=True), 'after three launches')
    assert eng.read_sums() == (0.0, 0.0, 0.0, 0.0)
    # an engine that has only ever run eval
    other = MFEngine(s.n1, s.n2, d, len(s.batches[1][0]), shared_table=shared, device=dev)
    i1, i2, tg = s.batches[1]
    other.eval(E1, E2, _t(i1, dev), _t(i2, dev), _t(tg, dev), code, loss)
    assert other.read_sums() == (0.0, 0.0, 0.0, 0.0)
    bands.finish()


# ---------------------------------------------------------------------------------------------------------------------
# e. BPR
# ---------------------------------------------------------------------------------------------------------------------
def _bpr_batch(dev, bands, U, V, u, i, seed, epoch, row0, lr, l2, mode, compare_tables=True):
    import torch
    from otto_amd.matrix_factorization.engine import MFEngine
    B, n_items = len(u), V.shape[0]
    eng = MFEngine(U.shape[0], n_items, U.shape[1], B, device=dev)
    dU, dV = _t(U, dev), _t(V, dev)
    neg = torch.full((B,), -7, dtype=torch.int64, device=dev)
    ls = eng.bpr_step(dU, dV, _t(u, dev), _t(i, dev), seed=seed, epoch=epoch, row0=row0, lr=lr, l2=l2, mode=mode, neg_out=neg)
    eng.check()
    j = mo.bpr_negatives(seed, epoch, row0, i, n_items)
    assert np.array_equal(neg.cpu().numpy(), j), 'negative sampler differs from the oracle (integer work: bit-exact)'
    if compare_tables:
        U, V = U.copy(), V.copy()
        want = mo.bpr_step_batch(U, V, u, i, j, lr, l2)
        bands.scalar('loss', ls.item(), want)
        bands.close('tables', dU.cpu().numpy(), U, RTOL, BPR_ATOL, 'U')
        bands.close('tables', dV.cpu().numpy(), V, RTOL, BPR_ATOL, 'V')
    return j


@pytest.mark.parametrize('d,B', mi.BPR_BATCH_CASES)
def test_bpr_batch_step_every_factor_size(gpu_device, d, B):
    from otto_amd.matrix_factorization.engine import BPR_BATCH
    bands = Bands('e')
    U, V, u, i = mi.bpr_case(d, B, np.random.default_rng([5, d, B]))
    _bpr_batch(gpu_device, bands, U, V, u, i, 42, 0, 12345, 0.05, 0.01, BPR_BATCH)
    bands.finish()


@pytest.mark.parametrize('d', [4, 256])
def test_bpr_batch_one_owner_takes_the_whole_batch(gpu_device, d):
    """Every row is the same (u, i) and n_items = 2 leaves one negative: one owner per table row takes all B contributions."""
    from otto_amd.matrix_factorization.engine import BPR_BATCH
    bands = Bands('e')
    rng = np.random.default_rng([6, d])
    B = mi.gpb(d) + 1
    U, V = (rng.standard_normal((5, d)) * 0.2).astype(np.float32), (rng.standard_normal((2, d)) * 0.2).astype(np.float32)
    j = _bpr_batch(gpu_device, bands, U, V, np.full(B, 3), np.full(B, 1), 42, 0, 12345, 0.05, 0.01, BPR_BATCH)
    assert (j == 0).all()
    bands.finish()


@pytest.mark.parametrize('mode', ['batch', 'hogwild'])
def test_bpr_sampler_uses_all_sixteen_attempts_then_falls_back(gpu_device, mode):
    """Global row 6543 draws the positive 16 times at n_items = 2 and takes (pos + 1) % n_items; a row of the n_items = 3
    window draws it 15 times and is accepted on the last attempt with the item the fallback would NOT have given."""
    from otto_amd.matrix_factorization.engine import BPR_BATCH, BPR_HOGWILD
    bands = Bands('e')
    code, batch = (BPR_BATCH, True) if mode == 'batch' else (BPR_HOGWILD, False)
    rng = np.random.default_rng(8)
    d, B = 4, 256
    U = (rng.standard_normal((B, d)) * 0.2).astype(np.float32)
    u = np.arange(B)
    row = mi.FALLBACK_ROWS[0]
    assert mo.bpr_negative(1, 0, row, 1, 2, attempts=True) == (0, 16)
    j = _bpr_batch(gpu_device, bands, U, (rng.standard_normal((2, d)) * 0.2).astype(np.float32), u, np.ones(B, dtype=np.int64),
                   1, 0, row - 100, 0.05, 0.01, code, compare_tables=batch)
    assert j[100] == 0
    row, pos, neg = mi.LAST_ATTEMPT
    assert mo.bpr_negative(1, 0, row, pos, 3, attempts=True) == (neg, 15) and neg != (pos + 1) % 3
    j = _bpr_batch(gpu_device, bands, U, (rng.standard_normal((3, d)) * 0.2).astype(np.float32), u, np.full(B, pos),
                   1, 0, row - 37, 0.05, 0.01, code, compare_tables=batch)
    assert j[37] == neg
    bands.finish()


@pytest.mark.parametrize('l2', [0.01, 0.0])
@pytest.mark.parametrize('d', mi.D_ALL)
def test_bpr_hogwild_on_a_race_free_batch(gpu_device, d, l2):
    import torch
    from otto_amd.matrix_factorization.engine import MFEngine, BPR_HOGWILD
    bands = Bands('e')
    U, V, u, i, j = mi.race_free_triplets(d, 1, mi.race_rng())
    assert len(u) >= 65
    eng = MFEngine(U.shape[0], V.shape[0], d, len(u), device=gpu_device)
    dU, dV = _t(U, gpu_device), _t(V, gpu_device)
    neg = torch.full((len(u),), -7, dtype=torch.int64, device=gpu_device)
    ls = eng.bpr_step(dU, dV, _t(u, gpu_device), _t(i, gpu_device), seed=1, epoch=0, row0=0, lr=0.1, l2=l2, mode=BPR_HOGWILD,
                      neg_out=neg)
    eng.check()
    assert np.array_equal(neg.cpu().numpy(), j)
    want = mo.bpr_step_sequential(U, V, u, i, j, 0.1, l2)
    bands.scalar('loss', ls.item(), want)
    bands.close('tables', dU.cpu().numpy(), U, RTOL, BPR_ATOL, 'U')
    bands.close('tables', dV.cpu().numpy(), V, RTOL, BPR_ATOL, 'V')
    bands.finish()


# ---------------------------------------------------------------------------------------------------------------------
# f. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_and_launch_nothing(gpu_device):
    """Every refusal of the step, eval and BPR entry points: -22, its message in otto_last_error, nothing written."""
    import torch
    from otto_amd import _lib
    from otto_amd.matrix_factorization.engine import MFEngine
    lib = _lib.lib()
    dev = gpu_device
    n1, n2, d, max_batch = 20, 10, 8, 16
    two = MFEngine(n1, n2, d, max_batch, device=dev)
    one = MFEngine(n1, n1, d, max_batch, shared_table=True, device=dev)
    single_item = MFEngine(n1, 1, d, max_batch, device=dev)
    T1 = [torch.full((n1, d), 7.0, device=dev) for _ in range(3)]
    T2 = [torch.full((n2, d), 7.0, device=dev) for _ in range(3)]
    T3 = [torch.full((n1, d), 7.0, device=dev) for _ in range(3)]        # distinct tensors of the shared table's shape
    V1 = torch.full((1, d), 7.0, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    pred = torch.full((max_batch + 1,), 7.0, device=dev)
    neg = torch.full((max_batch + 1,), 7, dtype=torch.int64, device=dev)
    ids = torch.zeros(max_batch + 1, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def step(eng=two, A=T1, Bt=T2, B=4, kind=0, t=1):
        return lib.otto_mf_step_sparse_adam(eng._ctx, p(A[0]), p(A[1]), p(A[2]), p(Bt[0]), p(Bt[1]), p(Bt[2]), p(ids), p(ids),
                                            p(ids), B, kind, 0.05, 0.9, 0.999, 1e-8, t, p(loss), stream)

    def evaluate(fn, B=4, kind=0):
        return fn(two._ctx, p(T1[0]), p(T2[0]), p(ids), p(ids), p(ids), B, kind, p(pred), p(loss), stream)

    def bpr(eng=two, V=T2[0], B=4, mode=1):
        return lib.otto_mf_bpr_step(eng._ctx, p(T1[0]), p(V), p(ids), p(ids), B, 1, 0, 0, 0.05, 0.0, mode, p(loss), p(neg), stream)

    cases = [(lambda: step(B=0), b'outside (0, max_batch'), (lambda: step(B=max_batch + 1), b'outside (0, max_batch'),
             (lambda: step(t=0), b't must be >= 1'), (lambda: step(kind=2), b'unknown loss kind 2'),
             (lambda: step(kind=-1), b'unknown loss kind -1'),
             (lambda: step(eng=one, A=T1, Bt=T3), b'identical table pointers'),
             (lambda: bpr(eng=one, V=T1[0]), b'separate user and item tables'),
             (lambda: bpr(eng=single_item, V=V1), b'at least 2 items'), (lambda: bpr(mode=2), b'unknown BPR mode 2'),
             (lambda: bpr(B=0), b'outside (0, max_batch'), (lambda: bpr(B=max_batch + 1), b'outside (0, max_batch')]
    for fn in (lib.otto_mf_eval, lib.otto_mf_eval_sums):
        cases += [(lambda fn=fn: evaluate(fn, B=0), b'outside (0, max_batch'),
                  (lambda fn=fn: evaluate(fn, B=max_batch + 1), b'outside (0, max_batch'),
                  (lambda fn=fn: evaluate(fn, kind=3), b'unknown loss kind 3')]
    for k, (call, word) in enumerate(cases):
        assert call() == -22 and word in lib.otto_last_error(), (k, word, lib.otto_last_error())
    torch.cuda.synchronize(dev)
    for t in T1 + T2 + T3 + [V1, loss, pred]:
        assert bool((t == 7.0).all()), 'a refused call wrote to its tables or outputs'
    assert bool((neg == 7).all())
    assert two.read_sums() == (0.0, 0.0, 0.0, 0.0)
    two.check(), one.check(), single_item.check()
    assert step() == 0 and step(eng=one, A=T1, Bt=T1) == 0 and bpr() == 0      # the same calls with good arguments run
    torch.cuda.synchronize(dev)
    two.check(), one.check()
