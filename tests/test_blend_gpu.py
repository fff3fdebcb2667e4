"""SPEC-BLEND on the device: robust statistics and scaling, the outer-join blend and the end-to-end top-k, each against
the NumPy restatement (tests/blend_restatement.py), the hand fixture or the committed scikit-learn / pandas golden data --
never against the code under test. Comparisons are bit-exact; zeros are sign-blind where the spec says so."""
import json
import os

import numpy as np
import pytest

import blend_inputs as bi
import blend_restatement as br
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def blend(gpu_device):
    import __graft_entry__ as g
    g.build()
    from otto_amd.ranker import blend as mod
    return mod


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'blend_golden.npz'))


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'blend_hand.json')) as f:
        return json.load(f)


def dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)


def dev_models(models, gpu_device):
    return [tuple(dev(c, gpu_device) for c in m) for m in models]


def check_scale(blend, gpu_device, x, tag):
    nv_want, stats_want = br.robust_stats(x)
    out_want, center_want, scale_want = br.robust_scale(x)
    dx = dev(x, gpu_device)
    nv, stats = blend.robust_stats(dx)
    assert nv == nv_want, tag
    assert br.same_bits(stats, stats_want), (tag, stats, stats_want)
    center, scale = blend.center_scale(nv, stats)
    assert br.same_bits(np.float64(center), center_want) and br.same_bits(np.float64(scale), scale_want), tag
    out, center2, scale2 = blend.robust_scale(dx)
    assert (center2, scale2) == (center, scale), tag
    assert br.same_bits(out.cpu().numpy(), out_want), tag
    assert np.array_equal(dx.cpu().numpy().view(np.uint64), np.asarray(x).view(np.uint64)), f'{tag}: the input was written'


@pytest.mark.parametrize('family', bi.SCALE_FAMILIES)
def test_robust_scale_families_and_sizes(blend, gpu_device, family):
    for n in bi.SCALE_SIZES:
        check_scale(blend, gpu_device, bi.scale_input(family, n), (family, n))


def test_robust_scale_float32_column_is_widened(blend, gpu_device):
    x32 = bi.scale_input('normal', 1003).astype(np.float32)
    out, center, scale = blend.robust_scale(dev(x32, gpu_device))
    want, c, s = br.robust_scale(x32.astype(np.float64))
    assert (center, scale) == (c, s) and br.same_bits(out.cpu().numpy(), want)


def test_robust_scale_hand_fixture(blend, gpu_device, hand):
    sc = hand['scale']
    x = np.array([float(v) for v in sc['x']])
    nv, stats = blend.robust_stats(dev(x, gpu_device))
    assert nv == sc['nv'] and stats.tolist() == sc['stats']
    out, center, scale = blend.robust_scale(dev(x, gpu_device))
    assert (center, scale) == (sc['center'], sc['scale'])
    assert br.same_bits(out.cpu().numpy(), np.array([float(v) for v in sc['scaled']]).astype(np.float32))


def test_robust_scale_reproduces_golden_robust_scaler(blend, gpu_device, golden):
    for i in range(int(golden['n_scale'])):
        out, center, scale = blend.robust_scale(dev(golden[f'scale_{i}_x'], gpu_device))
        assert br.same_bits(np.float64(center), golden[f'scale_{i}_center']), i
        assert br.same_bits(np.float64(scale), golden[f'scale_{i}_scale']), i
        assert br.same_bits(out.cpu().numpy(), golden[f'scale_{i}_out']), i


def test_robust_stats_refusals(blend, gpu_device):
    import torch
    from otto_amd._lib import OttoError
    with pytest.raises(OttoError, match=r'code -22.*empty'):
        blend.robust_stats(torch.zeros(0, dtype=torch.float64, device=gpu_device))
    with pytest.raises(OttoError, match=r'code -22.*NaN'):
        blend.robust_stats(dev(np.full(1001, np.nan), gpu_device))
    for name, x in bi.inf_cases().items():
        with pytest.raises(OttoError, match=r'code -22.*infinite'):
            blend.robust_stats(dev(x, gpu_device))
    # the library is still usable afterwards
    check_scale(blend, gpu_device, bi.scale_input('normal', 65), 'after refusals')


def check_join(blend, gpu_device, models, weights, left, tag):
    sid_w, off_w, aid_w, pred_w = br.blend(models, weights, left)
    sid, off, aid, pred, pred64 = blend.blend_predictions(dev_models(models, gpu_device), weights, left, scale=False, _want64=True)
    assert aid.numel() == aid_w.size and sid.numel() == sid_w.size, (tag, aid.numel(), aid_w.size)
    assert np.array_equal(sid.cpu().numpy(), sid_w), tag
    assert np.array_equal(off.cpu().numpy(), off_w), tag
    assert np.array_equal(aid.cpu().numpy(), aid_w), tag
    got = pred.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), pred_w.view(np.uint32)), tag
    assert np.array_equal(pred64.cpu().numpy().view(np.uint64), got.astype(np.float64).view(np.uint64)), tag


@pytest.mark.parametrize('name', sorted(bi.join_cases()))
def test_join_matches_restatement(blend, gpu_device, name):
    models, weights, left = bi.join_cases()[name]
    check_join(blend, gpu_device, models, weights, left, name)


def test_join_hand_fixture(blend, gpu_device, hand):
    models = [(np.array(m['session'], np.int32), np.array(m['aid'], np.int32), np.array(m['score'], np.float32)) for m in hand['models']]
    sid, off, aid, pred = blend.blend_predictions(dev_models(models, gpu_device), hand['weights'], hand['left_of_base'], scale=False)
    want = hand['out']
    assert sid.tolist() == want['session_id'] and off.tolist() == want['row_off'] and aid.tolist() == want['aid']
    assert pred.tolist() == want['pred']
    sid, top, n = blend.blend_topk(dev_models(models, gpu_device), hand['weights'], hand['left_of_base'], k=2, scale=False)
    assert sid.tolist() == want['session_id'] and top.tolist() == want['top2'] and n.tolist() == [2, 2]


def test_join_all_models_empty(blend, gpu_device):
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    sid, off, aid, pred = blend.blend_predictions(dev_models([e, e], gpu_device), (0.5, 0.5), scale=False)
    assert sid.numel() == 0 and aid.numel() == 0 and pred.numel() == 0 and off.tolist() == [0]


def test_join_reproduces_golden_pandas_merge(blend, gpu_device, golden):
    models = [(golden[f'join_m{m}_session'], golden[f'join_m{m}_aid'], golden[f'join_m{m}_score']) for m in range(4)]
    cols = golden['join_out_cols']
    # weight 1 on one model, 0 on the others: the prediction is that model's zero-filled column
    for m in range(4):
        w = [1.0 if i == m else 0.0 for i in range(4)]
        sid, off, aid, pred = blend.blend_predictions(dev_models(models, gpu_device), w, (0, 1, 0, 0), scale=False)
        ses = np.repeat(sid.cpu().numpy(), np.diff(off.cpu().numpy()))
        assert np.array_equal(ses, golden['join_out_session']) and np.array_equal(aid.cpu().numpy(), golden['join_out_aid'])
        assert br.same_bits(pred.cpu().numpy(), cols[m]), m
    check_join(blend, gpu_device, models, br.CLICK_WEIGHTS, (0, 1, 0, 0), 'golden')
    assert br.same_bits(br.prediction(cols, br.CLICK_WEIGHTS), br.blend(models, br.CLICK_WEIGHTS, (0, 1, 0, 0))[3])


def test_join_refusals(blend, gpu_device):
    from otto_amd._lib import OttoError
    for name, (models, weights) in bi.duplicate_cases().items():
        with pytest.raises(OttoError, match=r'code -22.*repeat'):
            blend.blend_predictions(dev_models(models, gpu_device), weights, scale=False)
    for name, (models, weights) in bi.negative_cases().items():
        with pytest.raises(OttoError, match=r'code -22.*negative'):
            blend.blend_predictions(dev_models(models, gpu_device), weights, scale=False)
    models, weights, left = bi.join_cases()['total_65']
    check_join(blend, gpu_device, models, weights, left, 'after refusals')


@pytest.mark.parametrize('k', (1, 20, 64))
def test_blend_topk_end_to_end(blend, gpu_device, k):
    models, weights, left = bi.topk_case()
    scaled = [(s, a, br.robust_scale(v)[0]) for s, a, v in models]
    sid_w, off_w, aid_w, pred_w = br.blend(scaled, weights, left)
    top_w, n_w = br.topk(sid_w, off_w, aid_w, pred_w, k)
    sid, top, n = blend.blend_topk(dev_models(models, gpu_device), weights, left, k=k, scale=True)
    assert np.array_equal(sid.cpu().numpy(), sid_w)
    assert np.array_equal(n.cpu().numpy(), n_w)
    assert np.array_equal(top.cpu().numpy(), top_w)
