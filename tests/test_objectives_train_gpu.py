"""The two train loops with SPEC-OBJ's objectives and metrics on the device against tests/objectives_restatement.py, on 2,048
rows x 6 features in queries of 1 to 40 rows (tests/objectives_inputs.py): trees and scores bit for bit, the AUC and NDCG
histories exactly, the logloss history within the tolerance tests/test_objectives_gpu.py states; the initial-score fold
through ``forest_predict``; and the fold trainer with both boosters and a binary objective."""
import numpy as np
import pytest

import objectives_inputs as oi
from otto_amd.ranker import folds, gbdt, objectives, xgb
from otto_amd.ranker.forest import forest_predict

LOGLOSS_RTOL = oi.LOGLOSS_RTOL

pytestmark = pytest.mark.gpu

GBDT_INT = ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'decision_type', 'leaf_count')
GBDT_FLOAT = ('threshold', 'split_gain', 'leaf_value')
XGB_INT = GBDT_INT + ('count', 'left_id', 'right_id')
XGB_FLOAT = GBDT_FLOAT + ('cover', 'sum_grad', 'leaf_cover', 'leaf_sum_grad')


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mapper(edge_list):
    edges = np.full((len(edge_list), gbdt.MAX_EDGES), np.inf, dtype=np.float32)
    for f, e in enumerate(edge_list):
        edges[f, :len(e)] = e
    return gbdt.BinMapper(edges, [len(e) for e in edge_list])


def _same_trees(got, want, ints, floats, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ints:
            assert np.array_equal(getattr(g, k), w[k]), (where, i, k)
        for k in floats:
            assert np.array_equal(_bits(getattr(g, k)), _bits(w[k])), (where, i, k)


def _same_history(got, want, metric, where):
    assert len(got) == len(want), where
    if metric in ('binary_logloss', 'logloss'):
        assert all(abs(a - b) <= LOGLOSS_RTOL * b for a, b in zip(got, want)), (where, got, want)
    else:
        assert got == want, (where, got, want)


def _train(dev, module, params, c):
    d = oi.train_problem()
    dev_args = (_t(d['bins'], dev), _t(d['label'], dev), _t(d['query_off'], dev), _mapper(d['edge_list']))
    valid = (_t(d['vbins'], dev), _t(d['vlabel'], dev), _t(d['voff'], dev))
    return module.train(*dev_args, params, valid=valid, num_boost_round=c['rounds'], early_stopping_rounds=c['early'])


@pytest.mark.parametrize('name', list(oi.GBDT_CASES))
def test_gbdt_binary_training_equals_the_restatement(gpu_device, name):
    c, want = oi.GBDT_CASES[name], oi.gbdt_want(name)
    res = _train(gpu_device, gbdt, c['params'], c)
    _same_trees(res.trees, want['trees'], GBDT_INT, GBDT_FLOAT, name)
    assert res.best_iteration == want['best_iteration']
    _same_history(res.history, want['history'], c['params']['metric'], name)
    train_score = res.train_score.cpu().numpy()
    assert np.array_equal(_bits(train_score), _bits(want['train_score']))
    # the initial score sits in the first tree: the forest scored from 0.0 over the float32 matrix gives the trainer's bits
    X = _t(oi.train_problem()['X'], gpu_device)
    assert np.array_equal(_bits(forest_predict(res.forest, X).cpu().numpy()), _bits(train_score))
    assert res.forest.objective == f'binary sigmoid:{c["params"].get("sigmoid", 1.0):g}'
    assert f'\nobjective={res.forest.objective}\n' in gbdt.write_lightgbm_model(res.forest)
    if c['early']:
        assert res.best_iteration < len(res.history)            # the cut happened, on a decrease of the logloss
    p = objectives.transform(res.train_score, c['params'].get('sigmoid', 1.0)).cpu().numpy()
    assert ((p > 0) & (p < 1)).all()


@pytest.mark.parametrize('name', list(oi.XGB_CASES))
def test_xgb_training_with_the_new_objectives_equals_the_restatement(gpu_device, name):
    c, want = oi.XGB_CASES[name], oi.xgb_want(name)
    res = _train(gpu_device, xgb, c['params'], c)
    _same_trees(res.trees, want['trees'], XGB_INT, XGB_FLOAT, name)
    assert res.best_iteration == want['best_iteration']
    _same_history(res.history, want['history'], c['params']['eval_metric'], name)
    train_score = res.train_score.cpu().numpy()
    assert np.array_equal(_bits(train_score), _bits(want['train_score']))
    assert res.objective == res.forest.objective == c['params']['objective'] and res.base_margin == want['base_margin']
    X = _t(oi.train_problem()['X'], gpu_device)
    assert np.array_equal(_bits(xgb.predict(res, X, output_margin=True).cpu().numpy()), _bits(train_score))
    model = xgb.parse_xgboost_json(xgb.write_xgboost_json(res, params=c['params']))
    assert np.array_equal(_bits(xgb.predict(model, X, output_margin=True).cpu().numpy()), _bits(train_score))
    prediction = xgb.predict(res, X).cpu().numpy()
    if c['params']['objective'] == 'binary:logistic':
        assert ((prediction > 0) & (prediction < 1)).all()
        assert np.allclose(prediction, 1.0 / (1.0 + np.exp(-train_score)), rtol=1e-12)
        if c['early']:
            assert res.best_iteration < len(res.history)
    else:
        assert np.array_equal(_bits(prediction), _bits(train_score))      # a rank objective predicts its margin


def test_the_new_objectives_are_refused_without_the_feature_and_train_with_it(gpu_device):
    """On the commit before SPEC-OBJ both calls raised ``ValueError`` (objective 'binary' / 'rank:ndcg' not supported)."""
    c = dict(rounds=1, early=None)
    assert _train(gpu_device, gbdt, {'objective': 'binary', 'num_leaves': 4, 'min_data_in_leaf': 20}, c).best_iteration == 1
    assert _train(gpu_device, xgb, {'objective': 'rank:ndcg', 'max_depth': 2}, c).best_iteration == 1


@pytest.mark.parametrize('booster', ['lightgbm', 'xgboost'])
def test_cross_validate_with_a_binary_objective(gpu_device, booster):
    rng = np.random.default_rng(402)
    sizes = rng.integers(20, 41, 120)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, F = int(off[-1]), 6
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[rng.random((n, F)) < 0.02] = np.nan
    label, aid = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
    t_off, t_aid = [0], []
    for q in range(sizes.size):
        a, b = off[q], off[q + 1]
        aid[a:b] = rng.choice(5000, b - a, replace=False)
        if rng.random() >= 0.15:
            pos = a + int(np.argmax(np.nan_to_num(X[a:b, 0]) + 0.5 * rng.standard_normal(b - a)))
            label[pos] = 1
            t_aid.append(aid[pos])
        t_off.append(len(t_aid))
    truth = (_t(np.array(t_off, dtype=np.int64), gpu_device), _t(np.array(t_aid, dtype=np.int32), gpu_device))
    if booster == 'lightgbm':
        params = {'objective': 'binary', 'metric': 'auc', 'num_leaves': 8, 'min_data_in_leaf': 10, 'learning_rate': 0.2, 'is_unbalance': True}
    else:
        params = {'objective': 'binary:logistic', 'eval_metric': 'logloss', 'max_depth': 3, 'eta': 0.3, 'scale_pos_weight': 5.0}
    res = folds.cross_validate(_t(X, gpu_device), _t(label, gpu_device), _t(off, gpu_device), params, n_splits=3,
                               negative_sampling_ratio=0.5, seed=42, num_boost_round=4, early_stopping_rounds=2, aid=_t(aid, gpu_device),
                               truth=truth, booster=booster)
    assert np.isfinite(res.recall) and 0.0 < res.recall <= 1.0
    assert all(len(h) >= 1 and np.isfinite(h).all() for h in res.histories)
    oof = res.oof_prediction.cpu().numpy()
    assert np.isfinite(oof).all() and oof.std() > 0               # raw scores, one per row
    assert all(f.objective.startswith('binary') for f in res.forests)
