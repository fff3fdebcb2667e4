"""SPEC-XGB without a device: the restatement against the hand fixture, the draw rule, the ``map`` metric, the JSON model
writer and parser, ``resolve_params`` and ``feature_importance`` of ``ranker.xgb``, and the shapes of tests/xgb_inputs.py
that the device tests rely on."""
import json
import math
import os

import numpy as np
import pytest

import gbdt_restatement as gr
import xgb_inputs as xi
import xgb_restatement as xr
from conftest import GOLDEN
from otto_amd.ranker import gbdt, xgb
from otto_amd.ranker.forest import Forest, ModelFormatError


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'xgb_hand.json')) as f:
        return json.load(f)


# ---- the hand fixture

def test_the_fixture_is_what_its_script_writes(hand, tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_xgb_hand', os.path.join(GOLDEN, 'make_xgb_hand.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, 'HERE', str(tmp_path))
    mod.main()
    with open(tmp_path / 'xgb_hand.json') as f:
        assert json.load(f) == hand


def test_restated_objective_equals_the_hand_fixture(hand):
    o = hand['objective']
    score, label, off = np.array(o['score']), np.array(o['label'], dtype=np.int32), np.array(o['query_off'])
    assert xr.seeds(o['seed'])[0] == 309689372594955804 == xgb.derived_seeds(o['seed'])[0]
    g, h, invalid, bad, pairs = xr.pairwise(score, label, off, xr.seeds(o['seed'])[0], o['it'], want_pairs=True)
    assert invalid == 0 and not bad
    order = gr.rank_order(score)
    assert [int(order[r]) for r in xr.record_order(label[order])] == o['rec_rows']
    assert [[int(order[hi]), int(order[lo])] for _, hi, lo in pairs[0]] == o['pairs_rows']
    assert [pid for pid, _, _ in pairs[0]] == [0, 1, 2, 3, 4]
    assert np.array_equal(_bits(g), _bits(o['grad'])) and np.array_equal(_bits(h), _bits(o['hess']))
    # the table entries the fixture types in are the spec's: 1 / (1 + exp(lo + index / factor))
    table, lo, factor, _ = gr._tables(1.0)
    for d, p in ((3.0, 0.04742707953910805), (1.5, 0.18242751513476982), (0.0, 0.5), (-0.5, 0.6224620206021405)):
        assert table[int((d - lo) * factor)] == p
        assert abs(p - 1.0 / (1.0 + math.exp(d))) < 1e-4      # sigmoid(s_high - s_low), to the table's resolution


def test_restated_tree_equals_the_hand_fixture(hand):
    t = hand['tree']
    bins = np.array(t['bins'], dtype=np.uint8)
    q = np.stack([t['qg'], t['qh']], axis=1).astype(np.int32)
    edge_list = [np.array(e, dtype=np.float32) for e in t['edges']]
    got = xr.grow_tree(bins, q, t['exps'], edge_list, t['params'])
    for k in ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'count', 'left_id', 'right_id', 'leaf_count'):
        assert got[k].tolist() == t[k], k
    for k in ('threshold', 'split_gain', 'cover', 'sum_grad', 'leaf_value', 'leaf_cover', 'leaf_sum_grad'):
        assert np.array_equal(_bits(got[k]), _bits(t[k])), k
    assert got['hist_rows'] == t['hist_rows'] and got['n_levels'] == 2
    assert [r.tolist() for r in got['leaf_rows']] == [[0, 1, 2], [6, 7, 8, 9, 10, 11], [3, 4, 5]]


# ---- the draw rule

def test_top_bucket_draws_right_and_bottom_bucket_draws_left():
    lab = np.array([2, 2, 1, 0, 0, 0])                      # by rank; rec = ranks 0..5
    rows = np.arange(100, 106)
    for seed_it in range(50):
        for pid, high, low in xr.query_pairs(lab, rows, seed_it):
            r = pid                                         # rec is the identity here
            if lab[r] == 2:
                assert high == r and lab[low] < 2           # nleft = 0: every draw lands right
            if lab[r] == 0:
                assert low == r and lab[high] > 0           # nright = 0: every draw lands left
            assert lab[high] > lab[low]


def test_every_admissible_partner_is_drawn_and_none_from_the_own_bucket():
    lab = np.array([2, 1, 1, 1, 0, 0, 2, 0, 1, 0])          # one three-label layout, by rank
    rec = xr.record_order(lab)
    drawn = {r: set() for r in range(lab.size)}
    n_draws = 0
    for block in range(1000):                               # 10,000 rows: the same layout at 1,000 row offsets
        rows = np.arange(lab.size) + block * lab.size
        for pid, high, low in xr.query_pairs(lab, rows, 12345):
            r = rec[pid]
            partner = low if high == r else high
            assert r in (high, low) and lab[partner] != lab[r] and lab[high] > lab[low]
            drawn[r].add(partner)
            n_draws += 1
    assert n_draws == 10000
    for r in range(lab.size):
        assert drawn[r] == {o for o in range(lab.size) if lab[o] != lab[r]}, r


def test_a_query_with_one_label_draws_nothing():
    assert xr.query_pairs(np.array([1, 1, 1]), np.arange(3), 5) == []
    g, h, invalid, bad = xr.pairwise(np.array([0.3, 0.1, 0.2]), np.array([1, 1, 1]), np.array([0, 3]), 1, 0)
    assert not g.any() and not h.any() and invalid == 0 and not bad


# ---- map

def test_map_hand_values():
    #          query 0: ranks by score = labels 1, 0, 1 -> AP = (1/1 + 2/3) / 2;  query 1: no positive;  query 2: labels 0, 1
    score = np.array([3.0, 2.0, 1.0, 0.5, 0.4, 0.9, 0.1])
    label = np.array([1, 0, 1, 0, 0, 0, 1], dtype=np.int32)
    off = np.array([0, 3, 5, 7])
    ap0, ap2 = (1.0 + 2.0 / 3.0) / 2.0, 0.5
    assert xr.mean_average_precision(score, label, off) == float(np.sum(np.array([ap0, 1.0, ap2])) / 3)
    assert xr.mean_average_precision(score, label, off, minus=True) == float(np.sum(np.array([ap0, 0.0, ap2])) / 3)
    ap = gr.ap_at_k(score, label, off, xr.MAX_QUERY)[0]
    assert ap.tolist() == [ap0, -1.0, ap2]
    assert xgb.mean_average_precision(ap) == xr.mean_average_precision(score, label, off)
    assert xgb.mean_average_precision(ap, minus=True) == xr.mean_average_precision(score, label, off, minus=True)


# ---- JSON

def _result_of(trees, F, base_score=0.5):
    """What ``write_xgboost_json`` reads of a ``TrainResult``, from restated trees."""
    class R:
        pass
    r = R()
    r.trees = [xgb.XgbTree(**{k: v for k, v in t.items() if k not in ('leaf_rows', 'n_levels')}) for t in trees]
    r.forest = gr.to_forest(trees, F)
    r.base_score = base_score
    return r


def test_json_round_trip_gives_identical_arrays():
    trees = [xi.grow_want('depth6'), xi.grow_want('depth2_bag_list'), xi.grow_want('depth10')]
    r = _result_of(trees, xi.GROW_F, base_score=0.5)
    text = xgb.write_xgboost_json(r, [f'f{i}' for i in range(xi.GROW_F)])
    m = xgb.parse_xgboost_json(text)
    assert m.base_score == 0.5 and m.objective == 'rank:pairwise' and m.feature_names == [f'f{i}' for i in range(xi.GROW_F)]
    for k in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child', 'right_child', 'leaf_value'):
        a, b = getattr(m.forest, k), getattr(r.forest, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    doc = json.loads(text)
    assert doc['version'] == [1, 7, 2] and doc['learner']['objective']['name'] == 'rank:pairwise'
    lp = doc['learner']['learner_model_param']
    assert lp['num_feature'] == str(xi.GROW_F) and lp['num_class'] == '0' and float(lp['base_score']) == 0.5
    model = doc['learner']['gradient_booster']['model']
    assert model['gbtree_model_param']['num_trees'] == '3' and model['tree_info'] == [0, 0, 0]
    for k, (t, w) in enumerate(zip(model['trees'], trees)):
        N = 2 * w['leaf_value'].size - 1
        assert t['id'] == k and t['tree_param']['num_nodes'] == str(N)
        for name in ('left_children', 'right_children', 'parents', 'split_indices', 'default_left', 'split_conditions', 'split_type',
                     'base_weights', 'loss_changes', 'sum_hessian'):
            assert len(t[name]) == N, name
        assert t['parents'][0] == 2147483647 and t['categories'] == []
        left, right = np.array(t['left_children']), np.array(t['right_children'])
        # XGBoost's ids: the children of the split nodes, taken in ascending id, are 1, 2, 3, ...
        ids = np.flatnonzero(left >= 0)
        assert np.array_equal(np.stack([left[ids], right[ids]], axis=1).ravel(), np.arange(1, N))
        assert ((left < 0) == (right < 0)).all()
        leaves = np.flatnonzero(left < 0)
        assert sorted(np.array(t['split_conditions'])[leaves].tolist()) == sorted(w['leaf_value'].tolist())
        assert np.array_equal(np.array(t['sum_hessian'])[ids], w['cover'].astype(np.float32).astype(np.float64))
        assert np.array_equal(np.array(t['loss_changes'])[ids], w['split_gain'].astype(np.float32).astype(np.float64))


def test_threshold_identity():
    f32 = np.float32
    tiny, big = np.nextafter(f32(0), f32(1)), np.finfo(np.float32).max
    edges = np.array([0.0, -0.0, tiny, -tiny, big, -big, 1.0, -2.5, 1e-30, 3.4e38], dtype=np.float32)
    with np.errstate(over='ignore'):
        for e in edges:
            cond = xgb.split_condition(e)
            back = xgb.threshold_of(cond)
            assert back == e and back.dtype == np.float32
            xs = [e, np.nextafter(e, f32(np.inf)), np.nextafter(e, f32(-np.inf)), f32(-0.0), f32(0.0), f32(np.nan), f32(np.inf),
                  f32(-np.inf)]
            for x in xs:
                assert bool(x < cond) == bool(x <= e), (e, x)
                assert bool(x <= back) == bool(x <= e), (e, x)


def test_parser_refuses_what_it_cannot_score():
    r = _result_of([xi.grow_want('depth2')], xi.GROW_F)
    doc = json.loads(xgb.write_xgboost_json(r))
    xgb.parse_xgboost_json(json.dumps(doc))

    def broken(change):
        d = json.loads(json.dumps(doc))
        change(d)
        with pytest.raises(ModelFormatError):
            xgb.parse_xgboost_json(json.dumps(d))
    tree = lambda d: d['learner']['gradient_booster']['model']['trees'][0]
    broken(lambda d: d['learner']['learner_model_param'].update(num_class='3'))
    broken(lambda d: tree(d)['split_type'].__setitem__(0, 1))
    broken(lambda d: tree(d).update(categories=[1]))
    broken(lambda d: d['learner']['gradient_booster'].update(name='gblinear'))
    broken(lambda d: tree(d)['left_children'].__setitem__(0, 99))
    broken(lambda d: tree(d)['split_indices'].__setitem__(0, xi.GROW_F))
    broken(lambda d: tree(d)['right_children'].pop())
    broken(lambda d: d['learner'].pop('learner_model_param'))
    broken(lambda d: d['learner']['gradient_booster']['model'].update(trees=[]))
    with pytest.raises(ModelFormatError):
        xgb.parse_xgboost_json('[1, 2]')


# ---- resolve_params

REFUSED = [({'objective': 'rank:ndcg'}, 'objective'), ({'booster': 'dart'}, 'booster'), ({'tree_method': 'exact'}, 'tree_method'),
           ({'tree_method': 'approx'}, 'tree_method'), ({'grow_policy': 'lossguide'}, 'grow_policy'), ({'max_leaves': 31}, 'max_leaves'),
           ({'alpha': 0.1}, 'alpha'), ({'reg_alpha': 0.1}, 'reg_alpha'), ({'max_delta_step': 1}, 'max_delta_step'),
           ({'colsample_bylevel': 0.5}, 'colsample_bylevel'), ({'colsample_bynode': 0.5}, 'colsample_bynode'),
           ({'scale_pos_weight': 2}, 'scale_pos_weight'), ({'num_pairsample': 2}, 'num_pairsample'),
           ({'num_parallel_tree': 4}, 'num_parallel_tree'), ({'eval_metric': 'ndcg'}, 'eval_metric'),
           ({'eval_metric': ['map', 'ndcg']}, 'eval_metric'), ({'sampling_method': 'gradient_based'}, 'sampling_method'),
           ({'max_depth': 0}, 'max_depth'), ({'max_depth': 11}, 'max_depth'), ({'max_bin': 257}, 'max_bin'),
           ({'subsample': 0.0}, 'subsample'), ({'colsample_bytree': 1.5}, 'colsample_bytree')]


@pytest.mark.parametrize('params,key', REFUSED)
def test_resolve_params_refuses(params, key):
    with pytest.raises(ValueError, match=key):
        xgb.resolve_params(params)


def test_resolve_params_defaults_aliases_and_seeds():
    p, s = xgb.resolve_params(None)
    assert (p['max_depth'], p['min_child_weight'], p['lambda'], p['gamma'], p['eta'], p['max_bin'], p['base_score'], p['eval_metric']) \
        == (6, 1.0, 1.0, 0.0, 0.3, 255, 0.5, 'map')
    assert not s.bag_active and not s.features_active
    assert p['objective_seed'] == gbdt.mix(0, 1) and s.bagging_seed == gbdt.mix(0, 2) and s.feature_fraction_seed == gbdt.mix(0, 3)
    assert xgb.resolve_params({'max_bin': 256})[0]['max_bin'] == 255
    for alias, main, val in (('learning_rate', 'eta', 0.05), ('min_split_loss', 'gamma', 2.0), ('reg_lambda', 'lambda', 3.0),
                             ('random_state', 'seed', 11)):
        assert xgb.resolve_params({alias: val})[0][main] == val == xgb.resolve_params({main: val})[0][main]
        assert xgb.resolve_params({alias: val, main: DEFAULT_OF[main]})[0][main] == DEFAULT_OF[main]     # the main name wins
    p, s = xgb.resolve_params({'seed': 7, 'subsample': 0.8, 'colsample_bytree': 0.75, 'eval_metric': ['map-'], 'nthread': 8,
                               'verbosity': 0, 'predictor': 'gpu_predictor', 'gpu_id': 0, 'objective': 'rank:pairwise',
                               'tree_method': 'gpu_hist', 'booster': 'gbtree', 'grow_policy': 'depthwise', 'max_leaves': 0})
    assert (p['objective_seed'], s.bagging_seed, s.feature_fraction_seed) == xr.seeds(7) == xgb.derived_seeds(7)
    assert s == gbdt.Sampling(0.8, 1, 0.75, xr.seeds(7)[1], xr.seeds(7)[2]) and s.bag_active and s.features_active
    assert p['eval_metric'] == 'map-'
    assert len({*xr.seeds(7), *xr.seeds(8)}) == 6


DEFAULT_OF = {'eta': 0.3, 'gamma': 0.0, 'lambda': 1.0, 'seed': 0}


# ---- feature importance

def test_feature_importance_on_a_hand_tree(hand):
    t = hand['tree']
    tree = xgb.XgbTree(split_feature=np.array([0, 0, 1]), split_gain=np.array([8.0, 2.0, 3.0]), cover=np.array([12.0, 6.0, 5.0]))
    gain, weight, cover = xgb.feature_importance([tree, tree], 3)
    assert gain.tolist() == [5.0, 3.0, 0.0] and weight.tolist() == [4, 2, 0] and cover.tolist() == [9.0, 5.0, 0.0]
    tree = xgb.XgbTree(**{k: np.array(t[k]) for k in ('split_feature', 'split_gain', 'cover')})
    gain, weight, cover = xgb.feature_importance([tree], 2)
    assert gain.tolist() == [(t['split_gain'][0] + t['split_gain'][1]) / 2, 0.0] and weight.tolist() == [2, 0]
    assert cover.tolist() == [9.0, 0.0]
    want = xr.feature_importance([xi.grow_want('depth6')], xi.GROW_F)
    w = xi.grow_want('depth6')
    got = xgb.feature_importance([xgb.XgbTree(**{k: w[k] for k in ('split_feature', 'split_gain', 'cover')})], xi.GROW_F)
    for a, b in zip(got, want):
        assert np.allclose(a, b, rtol=1e-12)


# ---- the shapes the device tests rely on

def test_input_shapes():
    score, label, off = xi.objective_sizes()
    assert tuple(np.diff(off)) == xi.OBJECTIVE_SIZES and score.size / (off.size - 1) > 96        # four waves per query
    for kind in xi.OBJECTIVE_KINDS:
        score, label, off = xi.objective_kind(kind)
        assert score.size / (off.size - 1) <= 96                                                # one wave per query
    score, label, off = xi.objective_kind('beyond_table')
    assert max(np.ptp(score[a:b]) for a, b in zip(off[:-1], off[1:])) > 25
    assert not xi.objective_want('all_equal_labels')[0].any()
    g = xi.objective_want('no_positive')[0]
    score, label, off = xi.objective_kind('no_positive')
    assert not g[off[0]:off[1]].any() and g[off[1]:off[2]].any()
    assert np.isnan(xi.objective_kind('nan_score')[0]).any()
    assert set(xi.objective_kind('labels_0_to_31')[1].tolist()) == set(range(32))
    # growth: a leaf at depth 2 beside leaves at depth 6, so that the levels below have gaps in their live nodes
    d6 = xi.leaf_depths(xi.grow_want('depth6'))
    assert 2 in d6 and d6.max() == 6 and xi.grow_want('depth6')['n_levels'] == 6
    assert xi.leaf_depths(xi.grow_want('depth10')).max() == 10
    assert xi.grow_want('depth1')['leaf_value'].size == 2 and xi.grow_want('depth2')['leaf_value'].size == 4
    assert xi.grow_want('root_cannot_split')['leaf_value'].size == 1 and xi.grow_want('gamma_above_every_gain')['leaf_value'].size == 1
    assert xi.grow_want('depth10_mcw0')['leaf_value'].size != xi.grow_want('depth10')['leaf_value'].size     # min_child_weight binds
    assert set(xi.grow_want('depth6_list')['split_feature'].tolist()) <= set(xi.GROW_FEATURES.tolist())
    assert xi.grow_want('depth6_bag')['leaf_count'].sum() == int(0.7 * xi.GROW_N)
    # every leaf value is a float32
    lv = xi.grow_want('depth10')['leaf_value']
    assert np.array_equal(lv, lv.astype(np.float32).astype(np.float64))
    # training: the early-stopping case cuts, the sampled case samples
    w = xi.train_want('early_stopping')
    assert w['best_iteration'] < w['n_grown'] and len(w['history']) == w['n_grown']
    w = xi.train_want('sampled')
    assert all(b.size == int(0.8 * xi.train_problem()['label'].size) for b in w['bags']) and all(f.size == 9 for f in w['features'])
    w = xi.train_want('sampled_stop')                                       # sampling and the early-stopping cut together
    assert w['best_iteration'] < w['n_grown'] < 10
    assert all(b.size == int(0.7 * xi.train_problem()['label'].size) for b in w['bags']) and all(f.size == 6 for f in w['features'])
    d = xi.train_problem()
    assert not d['vlabel'][d['voff'][3]:d['voff'][4]].any()
