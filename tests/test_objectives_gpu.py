"""SPEC-OBJ on the device against tests/objectives_restatement.py: the pointwise logistic gradients, the label counts, NDCG@k,
AUC, logloss and rank:ndcg. Everything is bit for bit except logloss, whose two device functions (exp, log1p) are not
pinned. The inputs and their references come from tests/objectives_inputs.py (each reference is computed once), whose
shapes and whose restatement tests/test_objectives_cpu.py proves."""
import numpy as np
import pytest

import objectives_inputs as oi
import objectives_restatement as orr
import xgb_inputs as xi
from otto_amd import _lib
from otto_amd.ranker import gbdt, objectives, xgb

pytestmark = pytest.mark.gpu

LOGLOSS_RTOL = oi.LOGLOSS_RTOL


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return np.array_equal(_bits(got.cpu().numpy() if hasattr(got, 'cpu') else got), _bits(want))


@pytest.fixture(scope='module')
def K():
    return objectives.constants()


# ---- otto_obj_binary

def _binary(dev, n, sigma=1.0, w_pos=1.0, w_neg=1.0, floor=0.0, labels='mixed'):
    score, label = oi.binary_rows(n, sigma, labels)
    g, h = objectives.binary_gradients(_t(score, dev), _t(label, dev), sigma, w_pos, w_neg, floor)
    wg, wh, bad = oi.binary_want(n, sigma, w_pos, w_neg, floor, labels)
    assert not bad
    assert _same(g, wg) and _same(h, wh), (n, sigma, w_pos, w_neg, floor, labels)
    return wg, wh


def test_binary_at_every_size(gpu_device, K):
    group, stride = K['threads'], K['threads'] * K['max_blocks']
    assert (group, stride) == (256, 262144)                    # the sizes below stay a few MB
    for n in (1, 63, 64, 65, group - 1, group, group + 1, stride - 1, stride, stride + 1):
        wg, wh = _binary(gpu_device, n, w_pos=2.0, w_neg=0.75)
        assert not np.isnan(wg).any() and (wh >= 0).all()


@pytest.mark.parametrize('sigma', oi.SIGMAS)
def test_binary_sigmas_special_scores_and_floors(gpu_device, sigma):
    for floor in (0.0, 1e-16):
        wg, wh = _binary(gpu_device, 5000, sigma, 3.0, 0.5, floor)
        saturated = wh[[6, 7]]                                  # +-inf with a negative label: p is the table's first / last entry
        assert (saturated >= 0.5 * floor).all() and (floor == 0.0 or (wh > 0).all())
    score, label = oi.binary_rows(5000, sigma)
    assert np.isnan(score).any() and np.isinf(score).any() and (np.abs(score * sigma) == 25.0).any()


@pytest.mark.parametrize('labels', ['all_positive', 'all_negative', 'mixed'])
def test_binary_class_weights_from_the_device_counts(gpu_device, labels):
    n = 3001
    score, label = oi.binary_rows(n, 1.0, labels)
    counts = objectives.label_counts(_t(label, gpu_device))
    assert counts == orr.label_counts(label) == (int((label > 0).sum()), n)
    w = objectives.class_weights(*counts, is_unbalance=True)
    assert w == orr.class_weights(*counts, is_unbalance=True)
    if labels == 'mixed':
        assert w[0] > 1.0 and w[1] == 1.0                       # the positives are the smaller class
        flipped = (label <= 0).astype(np.int32)
        c2 = objectives.label_counts(_t(flipped, gpu_device))
        w2 = objectives.class_weights(*c2, is_unbalance=True)
        assert c2 == (n - counts[0], n) and w2[0] == 1.0 and w2[1] == w[0]
    else:
        assert w == (1.0, 1.0)
    wg, wh = _binary(gpu_device, n, 1.0, w[0], w[1], 0.0, labels)
    assert (wg <= 0).all() if labels == 'all_positive' else (wg >= 0).all() if labels == 'all_negative' else True


def test_label_counts_sizes(gpu_device, K):
    import torch
    stride = K['threads'] * K['max_blocks']
    for n in (0, 1, 64, 65, stride - 1, stride + 1):
        label = (np.arange(n) % 5 == 0).astype(np.int32) * 3
        assert objectives.label_counts(_t(label, gpu_device) if n else torch.empty(0, dtype=torch.int32, device=gpu_device)) == \
            ((n + 4) // 5, n)


@pytest.mark.parametrize('wrong', [32, -1])
def test_binary_refuses_a_label_outside_the_range(gpu_device, wrong):
    import torch
    n = 1000
    score, label = oi.binary_rows(n)
    label = label.copy()
    label[[0, 517, n - 1]] = wrong
    buf = [torch.full((n + 8,), 7.0, dtype=torch.float64, device=gpu_device) for _ in range(2)]
    with pytest.raises(_lib.OttoError, match='label'):
        objectives.binary_gradients(_t(score, gpu_device), _t(label, gpu_device), 1.0, 2.0, 1.0, 0.0, out=(buf[0][:n], buf[1][:n]))
    wg, wh, bad = orr.binary(score, label, 1.0, 2.0, 1.0, 0.0)
    assert bad and wg[0] == wg[517] == wh[n - 1] == 0.0 and wg[1:517].any()
    assert _same(buf[0][:n], wg) and _same(buf[1][:n], wh)
    assert (buf[0][n:] == 7.0).all() and (buf[1][n:] == 7.0).all()       # the words behind both outputs


# ---- otto_obj_ndcg_at_k

@pytest.mark.parametrize('k', oi.NDCG_K)
def test_ndcg_at_every_query_size(gpu_device, k):
    score, label, off = oi.ndcg_problem()
    got = objectives.ndcg_at_k(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), k)
    want, invalid = oi.ndcg_want(k)
    assert invalid == 0 and _same(got, want)
    assert (want[[oi.NDCG_SIZES.index(0), len(oi.NDCG_SIZES) - 4, len(oi.NDCG_SIZES) - 1]] == -1.0).all()
    assert objectives.mean_ndcg(got) == orr.mean_ndcg(want) and objectives.mean_ndcg(got, True) == orr.mean_ndcg(want, True)
    assert objectives.mean_ndcg(got) > objectives.mean_ndcg(got, True)
    tied = want[len(oi.NDCG_SIZES) - 2]                         # every score the same: the rank is the position
    assert 0.0 < tied <= 1.0


def test_ndcg_of_zero_labels_means_one_or_zero(gpu_device):
    score, label, off = oi.ndcg_problem()
    got = objectives.ndcg_at_k(_t(score, gpu_device), _t(np.zeros_like(label), gpu_device), _t(off, gpu_device), 20)
    assert (got == -1.0).all()
    assert objectives.mean_ndcg(got) == 1.0 and objectives.mean_ndcg(got, minus=True) == 0.0


def test_ndcg_refusals_and_no_query(gpu_device):
    import torch
    n = gbdt.MAX_QUERY + 1 + 40
    rng = np.random.default_rng(5)
    score, label = rng.standard_normal(n), rng.integers(0, 3, n).astype(np.int32)
    off = np.array([0, 20, 20 + gbdt.MAX_QUERY + 1, n], dtype=np.int64)
    out = torch.full((3,), 7.0, dtype=torch.float64, device=gpu_device)
    with pytest.raises(_lib.OttoError, match='quer'):
        _lib.call('otto_obj_ndcg_at_k', gpu_device, _t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), 3, n, 20,
                  gbdt._tables(1.0, gpu_device)[3], out)
    want, invalid = orr.ndcg_at_k(score, label, off, 20)
    assert invalid == 1 and want[1] == -1.0 and want[0] > 0 and _same(out, want)
    for k in (0, gbdt.MAX_QUERY + 1):
        with pytest.raises(ValueError, match='k must be'):
            objectives.ndcg_at_k(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), k)
    empty = objectives.ndcg_at_k(_t(score, gpu_device), _t(label, gpu_device), _t(np.zeros(1, dtype=np.int64), gpu_device), 5)
    assert empty.numel() == 0 and np.isnan(objectives.mean_ndcg(empty))


# ---- otto_obj_auc

def _auc(dev, kind, n, tile=4096):
    score, label = oi.auc_rows(kind, n, tile)
    got = objectives.auc_counts(_t(score, dev), _t(label, dev))
    assert got == oi.auc_want(kind, n, tile), (kind, n)
    return got


def test_auc_at_every_size(gpu_device, K):
    tile = K['sort_tile']
    assert tile == K['scan_tile'] == 4096
    for n in (1, 2, tile - 1, tile, tile + 1):
        a2, p, neg = _auc(gpu_device, 'random', n)
        assert p + neg == n and 0 <= a2 <= 2 * p * neg


@pytest.mark.parametrize('kind', oi.AUC_KINDS)
def test_auc_kinds(gpu_device, K, kind):
    tile = K['sort_tile']
    n = 3 * tile + 5                                            # several sort tiles and scan tiles
    a2, p, neg = _auc(gpu_device, kind, n, tile)
    value = objectives.auc_from_counts(a2, p, neg)
    assert value == orr.auc_from_counts(a2, p, neg)
    if kind == 'all_equal':
        assert a2 == p * neg and value == 0.5                   # one tie group over every tile
    elif kind in ('only_positive', 'only_negative'):
        assert a2 == 0 and value == 1.0
    elif kind == 'separable':
        assert value == 1.0
    elif kind == 'reversed':
        assert value == 0.0
    elif kind == 'nan_last':
        score, label = oi.auc_rows(kind, n, tile)
        moved = np.where(np.isnan(score), -np.inf, score)       # NaN last: as if below every number, -inf included
        moved[score == -np.inf] = -1e300
        assert orr.auc_counts(moved, label) == (a2, p, neg)
    else:
        assert 0.0 < value < 1.0


def test_auc_workspace_one_byte_short(gpu_device):
    import torch
    n = 5000
    score, label = oi.auc_rows('random', n)
    need = int(_lib.lib().otto_obj_auc_workspace_bytes(n))
    assert need > 0 and _lib.lib().otto_obj_auc_workspace_bytes(-1) == 0 and _lib.lib().otto_obj_auc_workspace_bytes(1 << 31) == 0
    out = torch.full((3,), 7, dtype=torch.int64, device=gpu_device)
    work = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.OttoError, match='d_work'):
        _lib.call('otto_obj_auc', gpu_device, _t(score, gpu_device), _t(label, gpu_device), n, out, work, need - 1)
    assert out.cpu().tolist() == [7, 7, 7]                      # refused before anything was launched
    _lib.call('otto_obj_auc', gpu_device, _t(score, gpu_device), _t(label, gpu_device), n, out, work, need)
    assert tuple(out.cpu().tolist()) == oi.auc_want('random', n)
    assert objectives.auc_counts(torch.empty(0, dtype=torch.float64, device=gpu_device),
                                 torch.empty(0, dtype=torch.int32, device=gpu_device)) == (0, 0, 0)


# ---- otto_obj_logloss

def test_logloss_is_close_and_does_not_depend_on_the_grid(gpu_device, K):
    """The sum has the same bits on every grid, and lies within objectives_inputs.LOGLOSS_RTOL = 1.5e-15 of the float64 NumPy
    value: measured on an MI355X, the largest relative difference over these inputs and the two logloss training histories
    was 3.667e-16, and the tolerance is four times that. Each figure is printed before it is asserted."""
    stride = K['threads'] * K['max_blocks']
    worst = 0.0
    for n, sigma in ((1, 1.0), (255, 1.0), (256, 0.5), (257, 2.0), (5000, 1.0), (stride + 1, 2.0), (stride + 1, 0.5)):
        score, label = oi.logloss_rows(n, sigma)
        ds, dl = _t(score, gpu_device), _t(label, gpu_device)
        sums = [objectives.logloss_sum(ds, dl, sigma, grid=g) for g in (None, 1, 7, K['logloss_parts'])]
        assert len({np.float64(s).view(np.uint64) for s in sums}) == 1, (n, sigma, sums)
        want = orr.logloss_sum(score, label, sigma)
        assert np.isfinite(sums[0]) and sums[0] >= 0
        rel = abs(sums[0] - want) / want if want else abs(sums[0])
        print(f'logloss n = {n} sigma = {sigma}: device {sums[0]!r} numpy {want!r} relative difference {rel:.3e}')
        worst = max(worst, rel)
        assert rel <= LOGLOSS_RTOL, (n, sigma, sums[0], want)
        assert abs(objectives.logloss(ds, dl, sigma) - orr.logloss(score, label, sigma)) <= LOGLOSS_RTOL * orr.logloss(score, label, sigma)
    print(f'logloss: largest relative difference {worst:.3e}')


def test_logloss_at_800_has_no_infinite_term(gpu_device):
    for sigma in oi.SIGMAS:
        score = np.array([800.0, -800.0, 800.0, -800.0]) / sigma
        label = np.array([1, 1, 0, 0], dtype=np.int32)
        for i in range(4):
            got = objectives.logloss_sum(_t(score[i:i + 1], gpu_device), _t(label[i:i + 1], gpu_device), sigma)
            assert got == (0.0 if (score[i] > 0) == (label[i] > 0) else 800.0)
        assert objectives.logloss_sum(_t(score, gpu_device), _t(label, gpu_device), sigma) == 1600.0


# ---- otto_xgb_lambdamart

def test_lambdamart_without_weights_has_the_bits_of_pairwise(gpu_device):
    for case in (xi.objective_sizes(), xi.objective_edge(), xi.objective_kind('labels_0_to_31'), xi.objective_kind('nan_score')):
        s, l, o = (_t(a, gpu_device) for a in case)
        for it in (0, 1):
            a = xgb.pairwise_gradients(s, l, o, xi.OBJECTIVE_SEED, it)
            b = xgb.lambdamart_gradients(s, l, o, xi.OBJECTIVE_SEED, it, weighting=0)
            assert _same(a[0], b[0].cpu().numpy()) and _same(a[1], b[1].cpu().numpy())
    wg, wh, _, _ = xi.objective_want('sizes')
    assert _same(xgb.lambdamart_gradients(*(_t(a, gpu_device) for a in xi.objective_sizes()), xi.OBJECTIVE_SEED, 0, 0)[0], wg)


def test_lambdamart_weights_at_every_query_size_and_two_iterations(gpu_device):
    s, l, o = (_t(a, gpu_device) for a in oi.lambdamart_problem())
    off = oi.lambdamart_problem()[2]
    for it in (0, 1):
        g, h = xgb.lambdamart_gradients(s, l, o, oi.OBJECTIVE_SEED, it, weighting=1)
        wg, wh, invalid, bad = oi.lambdamart_want(it, 1)
        assert invalid == 0 and not bad and _same(g, wg) and _same(h, wh)
        for q in (oi.LAMBDAMART_SIZES.index(1), oi.LAMBDAMART_SIZES.index(30)):     # one row; one label: IDCG or m is 0
            assert not wg[off[q]:off[q + 1]].any() and not wh[off[q]:off[q + 1]].any()
    assert not np.array_equal(oi.lambdamart_want(0, 1)[0], oi.lambdamart_want(1, 1)[0])
    with pytest.raises(_lib.OttoError, match='weighting'):
        xgb.lambdamart_gradients(s, l, o, oi.OBJECTIVE_SEED, 0, weighting=2)


def test_lambdamart_refuses_a_long_query(gpu_device):
    import torch
    n = gbdt.MAX_QUERY + 1 + 40
    rng = np.random.default_rng(3)
    score, label = rng.standard_normal(n), rng.integers(0, 3, n).astype(np.int32)
    off = np.array([0, 20, 20 + gbdt.MAX_QUERY + 1, n], dtype=np.int64)
    out = tuple(torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device) for _ in range(2))
    with pytest.raises(_lib.OttoError, match='quer'):
        xgb.lambdamart_gradients(_t(score, gpu_device), _t(label, gpu_device), _t(off, gpu_device), oi.OBJECTIVE_SEED, 0, 1, out=out)
    wg, wh, invalid, _ = orr.lambdamart(score, label, off, oi.OBJECTIVE_SEED, 0, 1)
    assert invalid == 1 and wg[:20].any() and not wg[20:20 + gbdt.MAX_QUERY + 1].any()
    assert _same(out[0], wg) and _same(out[1], wh)
