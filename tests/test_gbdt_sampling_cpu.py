"""The sampling of SPEC-GBDT without a GPU: the sampler against the hand-worked golden file, the host helpers of
``ranker.gbdt``, ``sampling_from_params`` over the reference's config, and the proof that every problem of
tests/test_gbdt_sampling_gpu.py has the shape that test relies on."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import gbdt_restatement as gr
import gbdt_sampling_inputs as si
import gbdt_sampling_restatement as sr
from otto_amd.ranker import gbdt


def _hand():
    with open(os.path.join(GOLDEN, 'gbdt_sampling_hand.json')) as fh:
        return json.load(fh)


# ---- the sampler

def test_golden_file_is_what_its_script_writes():
    spec = importlib.util.spec_from_file_location('make_gbdt_sampling_hand', os.path.join(GOLDEN, 'make_gbdt_sampling_hand.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.compute() == _hand()


def test_mix_bag_and_feature_list_equal_the_golden_file():
    h = _hand()
    assert any(int(e['s']) == 2 ** 64 - 1 for e in h['mix']) and len(h['mix']) >= 5
    for e in h['mix']:
        s, i, want = int(e['s']), int(e['i']), int(e['value'])
        assert sr.mix(s, i) == want and gbdt.mix(s, i) == want, e
    b = h['bag']
    assert (b['n'], b['bagging_fraction'], b['bagging_seed']) == (16, 0.5, 42)
    assert sr.bag_size(b['bagging_fraction'], b['n']) == gbdt.bag_size(b['bagging_fraction'], b['n']) == b['m'] == 8
    assert [d['draw'] for d in b['draws']] == [0, 1] and b['draws'][0]['rows'] != b['draws'][1]['rows']
    for d in b['draws']:
        seed = sr.mix(b['bagging_seed'], 2 * d['draw'])
        assert seed == int(d['seed'])
        got = sr.bag(b['n'], b['m'], seed)
        assert got.dtype == np.int32 and got.tolist() == d['rows']
    f = h['features']
    assert (f['F'], f['feature_fraction'], f['feature_fraction_seed']) == (10, 0.5, 42) and f['n_used'] == 5
    assert [e['iteration'] for e in f['iterations']] == [0, 1] and f['iterations'][0]['features'] != f['iterations'][1]['features']
    for e in f['iterations']:
        want = e['features']
        assert sr.feature_list(f['F'], f['feature_fraction'], f['feature_fraction_seed'], e['iteration']).tolist() == want
        got = gbdt.sample_features(f['F'], f['feature_fraction'], f['feature_fraction_seed'], e['iteration'])
        assert got.dtype == np.int32 and got.tolist() == want


def test_mix_is_a_bijection_in_i_on_a_window():
    for s in (0, 42, 2 ** 64 - 1):
        assert len({gbdt.mix(s, i) for i in range(4096)}) == 4096


@pytest.mark.parametrize('F,q,want', [(54, 0.9, 49), (54, 1.0, 54), (1, 0.5, 1), (2, 0.1, 2), (3, 0.1, 2), (128, 0.5, 64)])
def test_n_used(F, q, want):
    assert gbdt.n_used_features(F, q) == sr.n_used(F, q) == want
    got = gbdt.sample_features(F, q, 2, 0)
    assert got.size == want and (np.diff(got) > 0).all() and got[0] >= 0 and got[-1] < F


def test_bag_size_truncates_the_float64_product():
    assert gbdt.bag_size(0.9, 10) == 9              # int(0.9 * 10) == int(9.0) == 9
    assert gbdt.bag_size(0.3, 10) == 3              # int(0.3 * 10) == int(3.0) == 3: the product is exactly 3.0
    assert gbdt.bag_size(0.7, 10) == 7              # int(0.7 * 10) == int(7.0) == 7: this product is exactly 7.0 too
    assert gbdt.bag_size(0.29, 100) == 28           # int(0.29 * 100) == int(28.999999999999996) == 28: truncation, not rounding
    assert 0.3 * 10 == 3.0 and 0.7 * 10 == 7.0 and 0.29 * 100 == 28.999999999999996 and round(0.29 * 100) == 29
    assert gbdt.bag_size(0.07, 100) == 7            # int(0.07 * 100) == int(7.000000000000001) == 7
    assert 0.07 * 100 == 7.000000000000001
    for p, n in ((0.9, 10), (0.3, 10), (0.7, 10), (0.29, 100), (0.07, 100), (0.5, 3841), (0.9, 19948)):
        assert gbdt.bag_size(p, n) == sr.bag_size(p, n) == int(p * n)
    for p, n in ((0.5, 1), (0.09, 10), (0.999, 1)):
        assert int(p * n) == 0
        with pytest.raises(ValueError, match='empty bag'):
            gbdt.bag_size(p, n)


# ---- Sampling and the reference's config

def test_sampling_defaults_and_validation():
    s = gbdt.Sampling()
    assert (s.bagging_fraction, s.bagging_freq, s.feature_fraction, s.bagging_seed, s.feature_fraction_seed) == (1.0, 0, 1.0, 3, 2)
    assert not s.bag_active and not s.features_active
    assert gbdt.Sampling(0.9, 1, 0.9, 42, 42) == gbdt.Sampling(bagging_fraction=0.9, bagging_freq=1, feature_fraction=0.9,
                                                              bagging_seed=42, feature_fraction_seed=42)
    for kw, key in ((dict(bagging_fraction=0.0), 'bagging_fraction'), (dict(bagging_fraction=1.5), 'bagging_fraction'),
                    (dict(bagging_fraction=-0.1), 'bagging_fraction'), (dict(feature_fraction=0.0), 'feature_fraction'),
                    (dict(feature_fraction=1.01), 'feature_fraction'), (dict(bagging_freq=-1), 'bagging_freq'),
                    (dict(bagging_freq=1.5), 'bagging_freq'), (dict(bagging_seed=-1), 'bagging_seed'),
                    (dict(feature_fraction_seed=2 ** 64), 'feature_fraction_seed')):
        with pytest.raises(ValueError, match=key):
            gbdt.Sampling(**kw)


@pytest.mark.parametrize('event_type', ['click', 'cart', 'order'])
def test_reference_config_passes_whole(event_type):
    with open(os.path.join(GOLDEN, 'lgb_config_model_fit.json')) as fh:
        model = json.load(fh)['model'][event_type]
    rest, sampling = gbdt.sampling_from_params(model)
    assert sampling == gbdt.Sampling(0.9, 1, 0.9, 42, 42) and sampling.bag_active and sampling.features_active
    assert set(model) - set(rest) == {'bagging_fraction', 'bagging_freq', 'feature_fraction', 'feature_fraction_bynode',
                                      'bagging_seed', 'feature_fraction_seed'}
    p = gbdt.resolve_params(rest)
    assert p['num_leaves'] == 128 and p['min_data_in_leaf'] == 2000 and p['learning_rate'] == model['learning_rate']
    assert set(p) == set(gbdt.DEFAULTS)
    with pytest.raises(ValueError, match='bagging_fraction|feature_fraction'):     # resolve_params itself still refuses them
        gbdt.resolve_params(model)


def test_sampling_from_params_aliases_refusals_and_the_inactive_bag():
    rest, s = gbdt.sampling_from_params({'subsample': 0.8, 'subsample_freq': 2, 'colsample_bytree': 0.7, 'num_leaves': 31,
                                         'seed': 7})
    assert s == gbdt.Sampling(0.8, 2, 0.7, 3, 2) and rest == {'num_leaves': 31, 'seed': 7}      # `seed` derives nothing
    # a main name beside its alias wins in either order, for a sampling key and for a refused one
    for params in ({'subsample': 0.8, 'bagging_fraction': 0.6, 'bagging_freq': 1, 'subsample_freq': 5},
                   {'subsample_freq': 5, 'bagging_freq': 1, 'bagging_fraction': 0.6, 'subsample': 0.8}):
        rest, s = gbdt.sampling_from_params(params)
        assert s == gbdt.Sampling(0.6, 1) and rest == {}
    assert gbdt.sampling_from_params({'colsample_bynode': 0.5, 'feature_fraction_bynode': 1})[1] == gbdt.Sampling()
    with pytest.raises(ValueError, match='feature_fraction_bynode'):
        gbdt.sampling_from_params({'feature_fraction_bynode': 0.5, 'colsample_bynode': 1})
    rest, s = gbdt.sampling_from_params({'bagging_fraction': 0.5})
    assert s.bagging_fraction == 0.5 and s.bagging_freq == 0 and not s.bag_active and rest == {}
    assert gbdt.sampling_from_params(None) == ({}, gbdt.Sampling())
    assert gbdt.sampling_from_params({'feature_fraction_bynode': 1, 'pos_bagging_fraction': 1.0, 'neg_bagging_fraction': 1})[0] == {}
    for params, key in (({'feature_fraction_bynode': 0.5}, 'feature_fraction_bynode'), ({'colsample_bynode': 0.9}, 'feature_fraction_bynode'),
                        ({'pos_bagging_fraction': 0.5}, 'pos_bagging_fraction'), ({'neg_bagging_fraction': 0.5}, 'neg_bagging_fraction'),
                        ({'neg_subsample': 0.5}, 'neg_bagging_fraction'), ({'bagging_fraction': 0.0}, 'bagging_fraction'),
                        ({'bagging_fraction': 1.2}, 'bagging_fraction'), ({'subsample': -1}, 'bagging_fraction'),
                        ({'feature_fraction': 0}, 'feature_fraction'), ({'feature_fraction': 2}, 'feature_fraction'),
                        ({'bagging_freq': -1}, 'bagging_freq'), ({'subsample_freq': -3}, 'bagging_freq')):
        with pytest.raises(ValueError, match=key):
            gbdt.sampling_from_params(params)


def test_train_refuses_a_sampling_that_is_no_sampling():
    # the check comes before anything touches the bins, so no GPU is needed to see it raise
    class Bins:
        pass
    with pytest.raises(ValueError, match='gbdt.Sampling'):
        gbdt.train(Bins(), None, None, None, sampling={'bagging_fraction': 0.5})


# ---- the shapes the device tests rely on

def _unsampled_root_feature(case):
    p, prm = case['problem'], case['params']
    rows = np.arange(p['n']) if case['bag'] is None else case['bag']
    s = gr.best_split(gr.histogram(p['bins'], p['q'], rows), [len(e) for e in p['edge_list']], p['exps'], prm['min_data_in_leaf'],
                      prm['min_sum_hessian_in_leaf'], prm['lambda_l2'], prm['min_gain_to_split'])
    return s['feature']


def test_tree_cases_have_their_shape():
    assert {c[1] for c in si.TREE_CASES} == {3, 9, 54} and {c[3] for c in si.TREE_CASES} == {8, 16}
    root_outside = without_zero = 0
    for name, F, _, num_leaves, p_bag, q_feat in si.TREE_CASES:
        c = si.tree_case(name)
        p, w = c['problem'], c['want']
        assert 3800 <= p['n'] <= 20500 and p['bins'].shape == (F, p['n']) and c['params']['min_data_in_leaf'] == 20
        assert w['leaf_value'].size >= 3, name
        if p_bag is not None:
            m = int(p_bag * p['n'])
            assert c['bag'].size == m < p['n'] and (np.diff(c['bag']) > 0).all() and w['leaf_count'].sum() == m
            assert m <= w['hist_rows'] < p['n'] * 2
        else:
            assert c['bag'] is None and w['leaf_count'].sum() == p['n']
        if q_feat is not None:
            listed = set(c['features'].tolist())
            assert len(listed) == sr.n_used(F, q_feat) < F and set(w['split_feature'].tolist()) <= listed
            root_outside += _unsampled_root_feature(c) not in listed
            without_zero += 0 not in listed
            # the unlisted planes would have offered a split: the list is what keeps the tree off them
            free = sr.grow_tree(p['bins'], p['q'], p['exps'], p['edge_list'], c['params'], c['bag'], None)
            assert not set(free['split_feature'].tolist()) <= listed, name
        else:
            assert c['features'] is None
    assert root_outside >= 1 and without_zero >= 1


def test_training_cases_have_their_shape():
    for name, (sampling, valid, rounds, stop) in si.TRAIN_CASES.items():
        c = si.training(name)
        w, d = c['want'], c['problem']
        n, F = d['bins'].shape[1], d['bins'].shape[0]
        assert all(t['leaf_value'].size >= 3 for t in w['trees']), name
        m = int(sampling['bagging_fraction'] * n)
        assert all(t['leaf_count'].sum() == m < n for t in w['trees'])
        k = sampling['bagging_freq']
        for it, (bag, features) in enumerate(zip(w['bags'], w['features'])):
            assert np.array_equal(bag, sr.bag(n, m, sr.mix(si.BAGGING_SEED, 2 * (it // k))))
            assert np.array_equal(features, sr.feature_list(F, sampling['feature_fraction'], si.FEATURE_SEED, it))
            assert set(w['trees'][it]['split_feature'].tolist()) <= set(features.tolist())
        if k == 3 and len(w['bags']) >= 4:
            assert np.array_equal(w['bags'][0], w['bags'][2]) and not np.array_equal(w['bags'][2], w['bags'][3])
        if k == 1:
            assert not np.array_equal(w['bags'][0], w['bags'][1])
        assert any(0 not in f for f in w['features']) and any(0 in f for f in w['features'])
        # the out-of-bag rows moved too: a score update over the bag alone would leave them at zero
        out_of_bag = np.setdiff1d(np.arange(n), w['bags'][0])
        assert out_of_bag.size >= n // 20 and (w['train_score'][out_of_bag] != 0).all()
        if stop:
            assert 1 <= w['best_iteration'] < w['n_grown'] <= rounds and w['n_grown'] == w['best_iteration'] + stop
            assert w['best_iteration'] >= 4                       # the cut keeps trees of both the first and the second bag
        else:
            assert w['best_iteration'] == w['n_grown'] == rounds == 6 and (len(w['history']) == 6) == valid
    assert {c[0]['bagging_freq'] for c in si.TRAIN_CASES.values()} == {1, 3}
