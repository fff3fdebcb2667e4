"""SPEC-BLEND without a GPU: the NumPy restatement against the committed golden data (scikit-learn's RobustScaler, a
pandas left / outer / outer merge), the hand-computed fixture and, where they are installed, the live libraries; and
that the test inputs contain what they claim (duplicates, negative ids, inf, rows an FMA would round differently)."""
import json
import os

import numpy as np
import pytest

import blend_inputs as bi
import blend_restatement as br
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'blend_golden.npz'))


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'blend_hand.json')) as f:
        return json.load(f)


def test_restatement_reproduces_golden_scaler(golden):
    for i in range(int(golden['n_scale'])):
        out, center, scale = br.robust_scale(golden[f'scale_{i}_x'])
        assert br.same_bits(np.float64(center), golden[f'scale_{i}_center']), i
        assert br.same_bits(np.float64(scale), golden[f'scale_{i}_scale']), i
        assert br.same_bits(out, golden[f'scale_{i}_out']), i


def test_restatement_reproduces_golden_join(golden):
    models = [(golden[f'join_m{m}_session'], golden[f'join_m{m}_aid'], golden[f'join_m{m}_score']) for m in range(4)]
    s, a, cols = br.join(models, (0, 1, 0, 0))
    assert np.array_equal(s, golden['join_out_session']) and np.array_equal(a, golden['join_out_aid'])
    assert br.same_bits(cols, golden['join_out_cols'])


def test_restatement_reproduces_hand_fixture(hand):
    models = [(np.array(m['session'], np.int32), np.array(m['aid'], np.int32), np.array(m['score'], np.float32)) for m in hand['models']]
    sid, off, aid, pred = br.blend(models, hand['weights'], hand['left_of_base'])
    want = hand['out']
    assert sid.tolist() == want['session_id'] and off.tolist() == want['row_off'] and aid.tolist() == want['aid']
    assert pred.tolist() == want['pred']
    top, n = br.topk(sid, off, aid, pred, 2)
    assert top.tolist() == want['top2'] and n.tolist() == [2, 2]
    sc = hand['scale']
    x = np.array([float(v) for v in sc['x']])
    nv, stats = br.robust_stats(x)
    assert nv == sc['nv'] and stats.tolist() == sc['stats']
    out, center, scale = br.robust_scale(x)
    assert (center, scale) == (sc['center'], sc['scale'])
    assert br.same_bits(out, np.array([float(v) for v in sc['scaled']]).astype(np.float32))


def test_restatement_equals_live_robust_scaler():
    RobustScaler = pytest.importorskip('sklearn.preprocessing').RobustScaler
    for family in bi.SCALE_FAMILIES:
        for n in bi.SCALE_SIZES[:-1]:
            x = bi.scale_input(family, n)
            sc = RobustScaler()
            want = sc.fit_transform(x.reshape(-1, 1).copy())[:, 0].astype(np.float32)
            out, center, scale = br.robust_scale(x)
            assert br.same_bits(np.float64(center), np.float64(sc.center_[0])), (family, n)
            assert br.same_bits(np.float64(scale), np.float64(sc.scale_[0])), (family, n)
            assert br.same_bits(out, want), (family, n)


def test_restatement_equals_live_pandas_merge():
    pd = pytest.importorskip('pandas')
    for name in ('M4_click', 'M5_cart', 'one_empty', 'straddle_200001'):
        models, _, left = bi.join_cases()[name]
        left = left or (0,) * len(models)
        # the reference's shape: the base, the left joins, then the outer joins
        order = [0] + [m for m in range(1, len(models)) if left[m]] + [m for m in range(1, len(models)) if not left[m]]
        frames = [pd.DataFrame({'session': models[m][0], 'aid': models[m][1], f'p{m}': models[m][2]}) for m in range(len(models))]
        df = frames[order[0]]
        for m in order[1:]:
            df = df.merge(frames[m], how='left' if left[m] else 'outer', on=['session', 'aid'])
        df = df.fillna(0).sort_values(['session', 'aid']).reset_index(drop=True)
        s, a, cols = br.join(models, left)
        assert np.array_equal(s, df['session'].to_numpy()) and np.array_equal(a, df['aid'].to_numpy()), name
        for m in range(len(models)):
            assert br.same_bits(cols[m], df[f'p{m}'].to_numpy().astype(np.float32)), (name, m)


def test_fma_would_differ_on_the_arithmetic_inputs():
    for name in ('M4_click', 'M5_cart', 'straddle_200001'):
        models, weights, left = bi.join_cases()[name]
        _, _, cols = br.join(models, left)
        spec, fma = br.prediction(cols, weights), br.prediction_fma(cols, weights)
        assert (spec.view(np.uint32) != fma.view(np.uint32)).any(), name


def test_inputs_contain_what_they_claim():
    for name, (models, _) in bi.duplicate_cases().items():
        with pytest.raises(ValueError, match='duplicate'):
            br.join(models)
        k = (models[1][0].astype(np.int64) << 32) | models[1][1]
        assert np.unique(k).size == k.size - 1, name
        if name == 'first_and_last':
            assert k[0] == k[-1]
        for m in (0, 2):
            km = (models[m][0].astype(np.int64) << 32) | models[m][1]
            assert np.unique(km).size == km.size
    for name, (models, _) in bi.negative_cases().items():
        with pytest.raises(ValueError, match='negative'):
            br.join(models)
        assert sum(int((np.asarray(c) < 0).sum()) for m in models for c in m[:2]) == 1
    for name, x in bi.inf_cases().items():
        assert np.isinf(x).sum() == 1 and (x[np.isinf(x)][0] > 0) == (name == 'plus_inf')
        with pytest.raises(ValueError, match='infinite'):
            br.robust_stats(x)
    models, weights, left = bi.join_cases()['straddle_200001']
    assert sum(m[0].size for m in models) == 200001 and len({m[0].size for m in models}) == 1
    models, weights, left = bi.join_cases()['ids_to_int32_max']
    assert max(int(m[0].max()) for m in models) == 2 ** 31 - 1 and max(int(m[1].max()) for m in models) == 2 ** 31 - 1
    models, weights, left = bi.topk_case()
    sc = [(s, a, br.robust_scale(v)[0]) for s, a, v in models]
    sid, off, aid, pred = br.blend(sc, weights, left)
    assert np.isnan(pred).any() and (np.diff(off) == 1).any() and (np.diff(off) > 64).any()
    tied = any(np.unique(pred[off[j]:off[j + 1]][~np.isnan(pred[off[j]:off[j + 1]])]).size < (~np.isnan(pred[off[j]:off[j + 1]])).sum()
               for j in range(len(sid)))
    assert tied


def test_join_sort_edge_cases_contain_what_they_claim():
    cases = bi.join_cases()
    for tot in (4095, 4096, 4097, 16383, 16384, 16385):
        models, weights, left = cases[f'total_{tot}']
        assert [m[0].size for m in models] == [tot - tot // 3, tot // 3]
        keys = [set(zip(m[0].tolist(), m[1].tolist())) for m in models]
        assert keys[0] & keys[1] and keys[1] - keys[0], tot          # keys in both models, and keys of model 1 alone
        sid, off, aid, pred = br.blend(models, weights, left)        # valid for the restatement: no duplicate, no negative id
        assert aid.size == len(keys[0] | keys[1])
    models, weights, left = cases['every_digit_varies']
    o, a = bi.key_bits(models)
    assert all(((o ^ a) >> (8 * d)) & 255 for d in range(8)) and sum(m[0].size for m in models) > 5000
    assert min(int(c.min()) for m in models for c in m[:2]) == 0 and max(int(c.max()) for m in models for c in m[:2]) == 2 ** 31 - 1
    br.blend(models, weights, left)
    models, weights, left = cases['single_key']
    o, a = bi.key_bits(models)
    assert o == a and len(models) == 3 and all(m[0].size == 1 for m in models)
    sid, off, aid, pred = br.blend(models, weights, left)
    assert aid.size == 1 and off.tolist() == [0, 1]


def test_every_size_residue_and_parity_is_covered():
    nvs = {n for n in bi.SCALE_SIZES}
    assert {(n - 1) % 4 for n in nvs if n >= 1000} == {0, 1, 2, 3} and {n % 2 for n in nvs} == {0, 1}
