"""SPEC-OBJ without a device: tests/objectives_restatement.py against independent formulations (all pairs for AUC, a plain
sort and sum for NDCG, the exact sigmoid for the gradients, the hand fixture), ``resolve_params`` of both families with
every accepted key, alias and refusal, the model writers and parsers for the binary objectives, the host halves of
``ranker.objectives``, and the shapes of tests/objectives_inputs.py that the device tests rely on."""
import json
import math
import os

import numpy as np
import pytest

import gbdt_restatement as gr
import objectives_inputs as oi
import objectives_restatement as orr
import xgb_restatement as xr
from conftest import GOLDEN
from otto_amd.ranker import gbdt, objectives, xgb
from otto_amd.ranker.forest import parse_lightgbm_model

ULP4 = 4 * 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'objectives_hand.json')) as f:
        return json.load(f)


# ---- the hand fixture

def test_the_fixture_is_what_its_script_writes(hand, tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_objectives_hand', os.path.join(GOLDEN, 'make_objectives_hand.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, 'HERE', str(tmp_path))
    mod.main()
    with open(tmp_path / 'objectives_hand.json') as f:
        assert json.load(f) == hand


def test_restatement_and_host_halves_equal_the_hand_fixture(hand):
    b = hand['binary']
    g, h, bad = orr.binary(b['score'], np.array(b['label']), b['sigma'], b['w_pos'], b['w_neg'], b['hess_floor'])
    assert not bad and g.tolist() == b['grad'] and h.tolist() == b['hess']
    for w in hand['weights']:
        for fn in (orr.class_weights, objectives.class_weights):
            assert list(fn(w['n_pos'], w['n'], w['is_unbalance'], w['scale_pos_weight'])) == w['w']
    for c in hand['init']:
        for fn in (orr.init_score, objectives.init_score):
            assert abs(fn(c['n_pos'], c['n'], c['sigma']) - c['value']) <= ULP4 * abs(c['value'])
    assert orr.init_score(1, 4, 2.0) == objectives.init_score(1, 4, 2.0) and orr.init_score(4, 4) == objectives.init_score(4, 4) > 34
    for c in hand['margin']:
        for fn in (orr.base_margin, objectives.base_margin):
            assert abs(fn(c['base_score']) - c['value']) <= ULP4 * abs(c['value'])
    assert objectives.base_margin(0.5) == 0.0 and not np.signbit(objectives.base_margin(0.5))
    a = hand['auc']
    assert orr.auc_counts(a['score'], a['label']) == (a['a2'], a['p'], a['n'])
    assert orr.auc(a['score'], a['label']) == a['auc'] == objectives.auc_from_counts(a['a2'], a['p'], a['n'])
    n = hand['ndcg']
    off = np.array([0, 4])
    assert orr.ndcg_at_k(n['score'], n['label'], off, 1)[0][0] == n['at_1']
    assert abs(orr.ndcg_at_k(n['score'], n['label'], off, 4)[0][0] - n['at_4']) <= ULP4
    assert abs(orr.ndcg_at_k(n['score'], n['label'], off, 1024)[0][0] - n['at_4']) <= ULP4       # k beyond the query
    ll = hand['logloss']
    assert abs(orr.logloss_sum([0.0, 0.0, -0.0], [1, 0, 5]) - ll['zeros']) <= ULP4 * ll['zeros']
    assert orr.logloss_sum([400.0], [1], 2.0) == ll['positive_at_800'] and orr.logloss_sum([400.0], [0], 2.0) == ll['negative_at_800']
    assert orr.logloss_sum([-800.0], [0]) == 0.0 and orr.logloss_sum([-800.0], [1]) == 800.0
    m = hand['lambdamart']
    g, h, invalid, bad = orr.lambdamart(m['score'], np.array(m['label']), np.array([0, 2]), oi.OBJECTIVE_SEED, 0, 1)
    assert invalid == 0 and not bad
    assert np.allclose(g, m['grad'], rtol=ULP4, atol=0) and np.allclose(h, m['hess'], rtol=ULP4, atol=0)


# ---- the restatement against independent formulations

@pytest.mark.parametrize('kind', oi.AUC_KINDS)
def test_auc_equals_the_count_over_all_pairs(kind):
    score, label = oi.auc_rows(kind, 300, tile=64)
    a2, p, n = orr.auc_counts(score, label)
    pos, neg = score[label > 0], score[label <= 0]
    assert (p, n) == (pos.size, neg.size)
    # NaN sorts last: below every number, tied with every other NaN; -0.0 == +0.0
    key = lambda v: np.where(np.isnan(v), -np.inf, v)
    rank = lambda v: np.where(np.isnan(v), 0, np.where(np.isneginf(v), 1, 2))     # NaN < -inf < the rest
    kp, kn, rp, rn = key(pos)[:, None], key(neg)[None, :], rank(pos)[:, None], rank(neg)[None, :]
    wins = ((rp > rn) | ((rp == rn) & (kp > kn))).sum()
    ties = ((rp == rn) & (kp == kn)).sum()
    assert a2 == 2 * int(wins) + int(ties)
    if p and n:
        assert orr.auc(score, label) == (wins + 0.5 * ties) / (p * n)
    else:
        assert orr.auc(score, label) == 1.0
    if kind == 'all_equal':
        assert a2 == p * n and orr.auc(score, label) == 0.5
    if kind in ('separable', 'reversed'):
        assert orr.auc(score, label) == (1.0 if kind == 'separable' else 0.0)


@pytest.mark.parametrize('k', oi.NDCG_K)
def test_ndcg_equals_a_plain_sort_and_sum(k):
    score, label, off = oi.ndcg_problem()
    got, invalid = oi.ndcg_want(k)
    assert invalid == 0
    for q in range(off.size - 1):
        rows = list(range(int(off[q]), int(off[q + 1])))
        ranked = sorted(rows, key=lambda r: (-(score[r] + 0.0), r))               # + 0.0 folds -0.0; position breaks ties
        dcg = math.fsum((2.0 ** label[r] - 1.0) / math.log2(2.0 + i) for i, r in enumerate(ranked[:k]))
        ideal = math.fsum((2.0 ** l - 1.0) / math.log2(2.0 + i) for i, l in enumerate(sorted(label[rows].tolist(), reverse=True)[:k]))
        if ideal == 0:
            assert got[q] == -1.0, q
        else:
            assert abs(got[q] - dcg / ideal) <= 1e-12, q
    empty, zeros = oi.NDCG_SIZES.index(0), len(oi.NDCG_SIZES) - 4
    assert got[empty] == -1.0 and got[zeros] == -1.0 and got[-1] == -1.0
    # the three queries above and whichever short query drew zeros only
    assert (got < 0).sum() >= 3 and orr.mean_ndcg(got) - orr.mean_ndcg(got, minus=True) == pytest.approx((got < 0).sum() / got.size)
    assert orr.mean_ndcg(np.array([-1.0])) == 1.0 and orr.mean_ndcg(np.array([-1.0]), True) == 0.0
    assert objectives.mean_ndcg(got) == orr.mean_ndcg(got) and objectives.mean_ndcg(got, True) == orr.mean_ndcg(got, True)


@pytest.mark.parametrize('sigma', oi.SIGMAS)
def test_binary_gradients_follow_the_exact_sigmoid_to_the_table_step(sigma):
    """|p - sigmoid(sigma * score)| <= (hi - lo) / BINS / 4 with hi - lo = 50: one table step of sigma * score times the
    sigmoid's largest slope, 1/4. Beyond +-25 both sides are within sigmoid(-25) < 1.4e-11 of 0 or 1."""
    score, label = oi.binary_rows(5000, sigma)
    w_pos, w_neg = 3.0, 0.5
    g, h, bad = orr.binary(score, label, sigma, w_pos, w_neg, 0.0)
    assert not bad
    ok = np.isfinite(score)
    bound = 50.0 / orr.BINS / 4
    p = 1.0 / (1.0 + np.exp(-sigma * score[ok]))
    t, w = (label[ok] > 0).astype(np.float64), np.where(label[ok] > 0, w_pos, w_neg)
    assert np.all(np.abs(g[ok] - sigma * (p - t) * w) <= sigma * w * bound * (1 + 1e-9))
    assert np.all(np.abs(h[ok] - sigma * sigma * p * (1 - p) * w) <= sigma * sigma * w * bound * (1 + 1e-9))
    # the special rows: 0.0 and -0.0 read the same entry, the ends and everything beyond them the first / last entry
    table = gr._tables(1.0)[0]
    first, last = table[0], table[-1]                                            # sigmoid(+25), sigmoid(-25) of the lookup's argument
    sp = oi.special_scores(sigma)
    gs, hs, _ = orr.binary(sp, np.zeros(sp.size, dtype=np.int32), sigma)
    assert gs[0] == gs[1] == sigma * 0.5
    assert gs[2] == gs[4] == gs[6] == sigma * first and gs[3] == gs[5] == gs[7] == sigma * last
    assert gs[8] == sigma * first and not np.isnan(hs).any()                    # NaN -> index 0
    # the table saturates at sigmoid(-25): p * (1 - p) stays near 1.4e-11, so XGBoost's floor of 1e-16 never bites here, and
    # a floor above that does
    hf = orr.binary(sp, np.zeros(sp.size, dtype=np.int32), sigma, hess_floor=1e-16)[1]
    assert np.array_equal(hf, hs) and hs.min() > 1e-16
    hf = orr.binary(sp, np.zeros(sp.size, dtype=np.int32), sigma, hess_floor=1e-3)[1]
    assert np.array_equal(hf[:2], hs[:2]) and (hf[2:] == 1e-3).all()
    # a label outside 0..31 zeroes its row and is reported
    g2, h2, bad = orr.binary([0.3, 0.3, 0.3], np.array([32, -1, 31]), sigma)
    assert bad and g2[0] == g2[1] == h2[0] == h2[1] == 0.0 and g2[2] < 0


def test_lambdamart_without_weights_is_the_pairwise_restatement():
    score, label, off = oi.lambdamart_problem()
    for it in (0, 1):
        a, b = orr.lambdamart(score, label, off, oi.OBJECTIVE_SEED, it, 0), xr.pairwise(score, label, off, oi.OBJECTIVE_SEED, it)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2:] == b[2:]
    g, h, invalid, bad = oi.lambdamart_want(0, 1)
    assert invalid == 0 and not bad
    one, single = oi.LAMBDAMART_SIZES.index(1), oi.LAMBDAMART_SIZES.index(30)
    for q in range(off.size - 1):
        zero = q in (one, single)
        assert g[off[q]:off[q + 1]].any() != zero and h[off[q]:off[q + 1]].any() != zero, q
    # every pair adds g to one row and -g to another: the gradients of a query cancel up to rounding
    assert all(abs(g[a:b].sum()) < 1e-12 for a, b in zip(off[:-1], off[1:]))
    assert not np.array_equal(g, oi.lambdamart_want(1, 1)[0])


def test_logloss_is_the_textbook_sum_and_survives_800():
    score, label = oi.logloss_rows(3000, 2.0)
    terms = orr.logloss_terms(score, label, 2.0)
    assert np.isfinite(terms).all() and (terms >= 0).all()
    y = np.where(label > 0, 1.0, -1.0)
    small = np.abs(2.0 * score) < 30
    assert np.allclose(terms[small], np.log(1.0 + np.exp(-y[small] * 2.0 * score[small])), rtol=1e-12)
    assert sorted(terms[-4:].tolist()) == [0.0, 0.0, 800.0, 800.0]
    assert orr.logloss(score, label, 2.0) == orr.logloss_sum(score, label, 2.0) / 3000


# ---- resolve_params, LightGBM family

def test_gbdt_accepts_objectives_metrics_and_their_aliases():
    R = lambda **kw: gbdt.resolve_params(kw, extended=True)
    assert R()['objective'] == 'lambdarank' and R()['metric'] == 'map'
    for key in ('objective', 'objective_type', 'app', 'application', 'loss'):
        assert R(**{key: 'binary'})['objective'] == 'binary' and R(**{key: 'lambdarank'})['objective'] == 'lambdarank'
    assert R(objective='binary', app='lambdarank')['objective'] == 'binary'              # the main name wins
    names = {'map': 'map', 'mean_average_precision': 'map', 'ndcg': 'ndcg', 'lambdarank': 'ndcg', 'xendcg': 'ndcg', 'auc': 'auc',
             'binary_logloss': 'logloss', 'binary': 'logloss'}
    for name, want in names.items():
        for key in ('metric', 'metrics', 'metric_types'):
            assert R(**{key: name})['metric'] == want
        assert R(metric=[name, 'auc'])['metric'] == want and R(metric=f'{name},auc')['metric'] == want
    assert R(metric='auc', metrics='ndcg')['metric'] == 'auc'
    # without the key the metric stays AP@k whatever the objective; LightGBM's default only on request
    assert R(objective='binary')['metric'] == 'map'
    for blank in ('', 'default'):
        assert R(objective='binary', metric=blank)['metric'] == 'logloss' and R(metric=blank)['metric'] == 'ndcg'
    p = R(objective='binary', sigmoid=2, is_unbalance='true', boost_from_average=False)
    assert p['sigmoid'] == 2.0 and p['is_unbalance'] is True and p['boost_from_average'] is False and p['scale_pos_weight'] == 1.0
    assert R(unbalance=True)['is_unbalance'] and R(unbalanced_sets=1)['is_unbalance'] and not R(is_unbalance=False, unbalance=True)['is_unbalance']
    assert R(scale_pos_weight=3)['scale_pos_weight'] == 3.0
    assert set(R(objective='binary', metric='auc')) == set(gbdt.DEFAULTS)


@pytest.mark.parametrize('params,word', [({'objective': 'rank_xendcg'}, 'objective'), ({'objective': 'multiclass'}, 'objective'),
                                         ({'app': 'regression'}, 'objective'), ({'metric': 'l2'}, 'metric'),
                                         ({'metrics': ['rmse', 'auc']}, 'metrics'), ({'metric': 'multi_logloss'}, 'metric'),
                                         ({'is_unbalance': True, 'scale_pos_weight': 2.0}, 'is_unbalance'),
                                         ({'is_unbalance': 'maybe'}, 'is_unbalance'), ({'boost_from_average': 2}, 'boost_from_average'),
                                         ({'scale_pos_weight': 0}, 'scale_pos_weight'), ({'scale_pos_weight': -1.0}, 'scale_pos_weight'),
                                         ({'sigmoid': 0}, 'sigmoid'), ({'lambda_l1': 0.5}, 'lambda_l1')])
def test_gbdt_refusals_name_the_key(params, word):
    with pytest.raises(ValueError, match=word):
        gbdt.resolve_params(params, extended=True)


def test_gbdt_first_contract_is_unchanged():
    """``resolve_params(params)`` alone refuses what it refused and ignores the new keys."""
    with pytest.raises(ValueError, match='objective'):
        gbdt.resolve_params({'objective': 'binary'})
    p = gbdt.resolve_params({'metric': 'auc', 'is_unbalance': True, 'scale_pos_weight': 4, 'boost_from_average': False})
    assert p == gbdt.resolve_params({}) and p['metric'] == 'map' and p['objective'] == 'lambdarank'


@pytest.mark.parametrize('event_type', ['click', 'cart', 'order'])
def test_reference_config_resolves_as_before(event_type):
    with open(os.path.join(GOLDEN, 'lgb_config_model_fit.json')) as fh:
        model = json.load(fh)['model'][event_type]
    rest, _ = gbdt.sampling_from_params(model)
    first, now = gbdt.resolve_params(rest), gbdt.resolve_params(rest, extended=True)
    assert first == now and now['objective'] == 'lambdarank' and now['metric'] == 'map' and now['eval_at'] == 20
    old_keys = ('num_leaves', 'min_data_in_leaf', 'min_sum_hessian_in_leaf', 'lambda_l2', 'min_gain_to_split', 'learning_rate',
                'lambdarank_truncation_level', 'lambdarank_norm', 'sigmoid', 'max_bin', 'eval_at')
    want = dict(num_leaves=128, min_data_in_leaf=2000, min_sum_hessian_in_leaf=1e-3, lambda_l2=0.01, min_gain_to_split=1e-5,
                learning_rate=model['learning_rate'], lambdarank_truncation_level=30, lambdarank_norm=True, sigmoid=1.0, max_bin=255,
                eval_at=20)
    assert {k: now[k] for k in old_keys} == want


# ---- resolve_params, XGBoost family

def test_xgb_accepts_objectives_and_metrics():
    R = lambda **kw: xgb.resolve_params(kw, extended=True)[0]
    assert R()['objective'] == 'rank:pairwise' and R()['metric'] == ('map', 1024, False)
    for o in xgb.OBJECTIVES:
        assert R(objective=o)['objective'] == o
    want = {'map': ('map', 1024, False), 'map-': ('map', 1024, True), 'map@20': ('map', 20, False), 'map@20-': ('map', 20, True),
            'ndcg': ('ndcg', 1024, False), 'ndcg-': ('ndcg', 1024, True), 'ndcg@5': ('ndcg', 5, False), 'ndcg@1024-': ('ndcg', 1024, True)}
    for name, m in want.items():
        for o in xgb.OBJECTIVES:
            assert R(objective=o, eval_metric=name)['metric'] == m == orr.parse_metric(name)
        assert R(eval_metric=[name])['eval_metric'] == name
    for name in ('auc', 'logloss'):
        assert R(objective='binary:logistic', eval_metric=name)['metric'] == (name, 1024, False)
    p = R(objective='binary:logistic', scale_pos_weight=4, base_score=0.25)
    assert p['scale_pos_weight'] == 4.0 and p['base_score'] == 0.25
    assert R(objective='rank:ndcg', scale_pos_weight=1)['scale_pos_weight'] == 1.0


@pytest.mark.parametrize('params,word', [
    ({'objective': 'rank:map'}, 'objective'), ({'objective': 'multi:softmax'}, 'objective'), ({'objective': 'reg:squarederror'}, 'objective'),
    ({'eval_metric': 'auc'}, 'eval_metric'), ({'eval_metric': 'logloss', 'objective': 'rank:ndcg'}, 'eval_metric'),
    ({'eval_metric': 'ndcg@0'}, 'eval_metric'), ({'eval_metric': 'ndcg@1025'}, 'eval_metric'), ({'eval_metric': 'ndcg@'}, 'eval_metric'),
    ({'eval_metric': 'error'}, 'eval_metric'), ({'eval_metric': ['ndcg', 'map']}, 'eval_metric'),
    ({'scale_pos_weight': 2}, 'scale_pos_weight'), ({'scale_pos_weight': 2, 'objective': 'rank:ndcg'}, 'scale_pos_weight'),
    ({'scale_pos_weight': 0, 'objective': 'binary:logistic'}, 'scale_pos_weight'),
    ({'base_score': 0.0, 'objective': 'binary:logistic'}, 'base_score'), ({'base_score': 1.0, 'objective': 'binary:logistic'}, 'base_score'),
    ({'base_score': 1.5, 'objective': 'binary:logistic'}, 'base_score'), ({'booster': 'dart', 'objective': 'binary:logistic'}, 'booster')])
def test_xgb_refusals_name_the_key(params, word):
    with pytest.raises(ValueError, match=word):
        xgb.resolve_params(params, extended=True)


def test_xgb_first_contract_is_unchanged():
    for params, word in (({'objective': 'rank:ndcg'}, 'objective'), ({'objective': 'binary:logistic'}, 'objective'),
                         ({'eval_metric': 'ndcg'}, 'eval_metric'), ({'eval_metric': 'auc'}, 'eval_metric'),
                         ({'scale_pos_weight': 2}, 'scale_pos_weight')):
        with pytest.raises(ValueError, match=word):
            xgb.resolve_params(params)
    assert xgb.resolve_params({'base_score': 1.5})[0]['base_score'] == 1.5       # the rank objectives add it as it is
    assert xgb.resolve_params({})[0] == xgb.resolve_params({}, extended=True)[0]


# ---- model writers and parsers

def test_lightgbm_text_round_trip_of_a_binary_model():
    want = oi.gbdt_want('auc')
    forest = gr.to_forest(want['trees'], oi.TRAIN_F)
    forest.objective = 'binary sigmoid:2'
    text = gbdt.write_lightgbm_model(forest)
    assert '\nobjective=binary sigmoid:2\n' in text
    back = parse_lightgbm_model(text)
    assert back.objective == 'binary sigmoid:2'
    for k in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value'):
        assert getattr(back, k).tobytes() == getattr(forest, k).tobytes(), k
    # the first tree carries the initial score: the restated trees scored from 0.0 give the trainer's bits
    d = oi.train_problem()
    assert want['init'] != 0.0
    score = np.zeros(oi.TRAIN_N)
    for tree in want['trees']:
        score = score + tree['leaf_value'][gr.route(d['bins'], tree)]
    assert np.array_equal(_bits(score), _bits(want['train_score']))


def test_xgboost_json_round_trip_of_a_binary_model():
    want = oi.xgb_want('binary_logloss_early')

    class R:
        pass
    r = R()
    r.trees = [xgb.XgbTree(**{k: v for k, v in t.items() if k not in ('leaf_rows', 'n_levels')}) for t in want['trees']]
    r.forest = gr.to_forest(want['trees'], oi.TRAIN_F)
    r.base_score, r.objective = 0.2, 'binary:logistic'
    text = xgb.write_xgboost_json(r, params={'objective': 'binary:logistic', 'scale_pos_weight': 2.0, 'eta': 3.0})
    doc = json.loads(text)
    assert doc['learner']['objective'] == {'name': 'binary:logistic', 'reg_loss_param': {'scale_pos_weight': '2.0'}}
    assert float(doc['learner']['learner_model_param']['base_score']) == 0.2                 # the probability, not the margin
    m = xgb.parse_xgboost_json(text)
    assert m.objective == 'binary:logistic' and m.base_score == 0.2 and m.base_margin == orr.base_margin(0.2) == want['base_margin']
    for k in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value'):
        assert getattr(m.forest, k).tobytes() == getattr(r.forest, k).tobytes(), k
    r.objective = 'rank:ndcg'
    m = xgb.parse_xgboost_json(xgb.write_xgboost_json(r, params={'objective': 'rank:ndcg'}))
    assert m.objective == 'rank:ndcg' and m.base_margin == m.base_score == 0.2


# ---- the shapes the device tests rely on, and the restated trainings

def test_input_shapes():
    score, label = oi.binary_rows(65)
    assert np.isnan(score[:18]).sum() == 2 and np.isinf(score[:18]).sum() == 4 and label[:9].max() <= 0 < label[9:18].min()
    assert (oi.binary_rows(5000)[1] == 31).any()
    sp = oi.special_scores(0.5)
    assert sp[2] == 50.0 and sp[4] > 50.0 and sp[5] < -50.0
    _, _, off = oi.ndcg_problem()
    assert tuple(np.diff(off)) == oi.NDCG_SIZES
    _, _, off = oi.lambdamart_problem()
    assert tuple(np.diff(off)) == oi.LAMBDAMART_SIZES
    score, _ = oi.auc_rows('straddle', 3 * 64 + 5, tile=64)
    runs = np.unique(score, return_counts=True)[1]
    assert runs.max() == 64 // 2 + 3                               # no run fits between two multiples of the tile
    score, _ = oi.auc_rows('zeros', 100)
    assert (np.signbit(score) & (score == 0)).any() and (~np.signbit(score) & (score == 0)).any()
    d = oi.train_problem()
    lens = np.diff(d['query_off'])
    assert d['X'].shape == (2048, 6) and lens.min() == 1 and lens.max() == 40 and int(d['query_off'][-1]) == 2048
    assert any(not d['vlabel'][a:b].any() for a, b in zip(d['voff'][:-1], d['voff'][1:]))


def test_restated_trainings_do_what_their_names_say():
    for name, c in oi.GBDT_CASES.items():
        w = oi.gbdt_want(name)
        assert len(w['trees']) == w['best_iteration'] >= 1 and all(t['leaf_value'].size >= 3 for t in w['trees'])
        assert (w['init'] == 0.0) == (c['params'].get('boost_from_average') is False)
    w = oi.gbdt_want('logloss_early_unbalanced')
    assert w['best_iteration'] < len(w['history']) <= 8 and w['history'][w['best_iteration'] - 1] == min(w['history'])
    a, n = oi.gbdt_want('auc'), oi.gbdt_want('ndcg_no_average')
    assert all(0.5 < v <= 1.0 for v in a['history']) and a['history'][-1] > a['history'][0]
    assert all(0.0 < v <= 1.0 for v in n['history'])
    for name in oi.XGB_CASES:
        w = oi.xgb_want(name)
        assert len(w['trees']) == w['best_iteration'] >= 1
    w = oi.xgb_want('binary_logloss_early')
    assert w['best_iteration'] < len(w['history']) and w['base_margin'] == orr.base_margin(0.2)
    assert oi.xgb_want('binary_auc')['base_margin'] == 0.0
