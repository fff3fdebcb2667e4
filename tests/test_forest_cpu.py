"""SPEC-FOREST without a GPU: the LightGBM text parser on both fixtures, the restatement against the hand-computed
leaves and scores, the float32 threshold equivalence the packed image rests on, and otto_forest_pack's validation (a
host function: it runs wherever the library loads)."""
import json
import os
import struct

import numpy as np
import pytest

import forest_restatement as fr
from conftest import GOLDEN

HEAD = os.path.join(GOLDEN, 'forest_order_fold1_head.lgb.txt')


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'forest_hand.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def hand_forest(hand):
    from otto_amd.ranker.forest import parse_lightgbm_model
    return parse_lightgbm_model(hand['model'])


@pytest.fixture(scope='module')
def head_forest():
    from otto_amd.ranker.forest import load_lightgbm_model
    return load_lightgbm_model(HEAD)


def hand_rows(hand):
    X = np.array([[np.float32(s) for s in r['x']] for r in hand['rows']], dtype=np.float32)
    return X, np.array([r['leaves'] for r in hand['rows']], dtype=np.int32), np.array([r['score'] for r in hand['rows']], dtype=np.float64)


def test_parser_hand_fixture(hand, hand_forest):
    f = hand_forest
    assert f.n_trees == hand['n_trees'] == 4 and f.num_leaves.tolist() == hand['num_leaves']
    assert f.n_features == 3 and f.feature_names == ['f_a', 'f_b', 'f_c'] and f.objective == 'lambdarank'
    assert sorted(set(f.decision_type.tolist())) == hand['decision_types'] == [2, 4, 6, 8, 10]
    assert f.threshold.dtype == np.float64 and f.threshold[1] == 1.5000000000000002 and f.threshold[1] != 1.5
    assert f.left_child.tolist() == [1, -1, -1, -1, -2, -3] and f.right_child.tolist() == [-3, -2, -2, 1, 2, -4]
    assert f.leaf_value.tolist() == [1, 2, 4, 0.25, 0.5, 8, 16, 32, 64, 128]
    fr.validate(f)
    # the right spine of the last tree is three nodes deep
    n0, c, depth = int(f.node_off[3]), 0, 0
    while c >= 0:
        c, depth = int(f.right_child[n0 + c]), depth + 1
    assert depth == 3


def test_parser_real_fixture(head_forest):
    f = head_forest
    assert f.n_trees == 8 and (f.num_leaves == 128).all() and f.threshold.size == 8 * 127 and f.leaf_value.size == 8 * 128
    assert f.n_features == 54 and f.objective == 'lambdarank'
    with open(HEAD) as fh:
        names = [l for l in fh.read().splitlines() if l.startswith('feature_names=')][0].split('=', 1)[1].split()
    assert f.feature_names == names and len(names) == 54 and names[0] == 'candidate_scores' and names[39] == 'session_count'
    assert set(f.decision_type.tolist()) <= {2, 8, 10}
    fr.validate(f, max_leaves=2048, max_features=128)
    assert not np.isnan(f.threshold).any() and np.abs(f.leaf_value).max() < 0.2      # shrinkage 0.05 is inside


def _mutate(text, old, new, count=1):
    assert old in text
    return text.replace(old, new, count)


@pytest.mark.parametrize('old,new,needle', [
    ('num_class=1', 'num_class=3', 'num_class'),
    ('num_tree_per_iteration=1', 'num_tree_per_iteration=2', 'num_tree_per_iteration'),
    ('Tree=1\nnum_leaves=2\nnum_cat=0', 'Tree=1\nnum_leaves=2\nnum_cat=1', 'num_cat'),
    ('leaf_value=8\nis_linear=0', 'leaf_value=8\nis_linear=1', 'is_linear'),
    ('objective=lambdarank\n', 'objective=lambdarank\naverage_output\n', 'average_output'),
    ('tree_sizes=300 200 100 400', 'tree_sizes=300 200 100', 'tree_sizes'),
    ('threshold=0 -1 1.0000000180025095e-35', 'threshold=0 -1', 'threshold'),
    ('split_feature=0 1 2', 'split_feature=0 1 2 0', 'split_feature'),
    ('decision_type=10', 'decision_type=10 2', 'decision_type'),
    ('left_child=1 -1', 'left_child=1', 'left_child'),
    ('right_child=1 2 -4', 'right_child=1 2 -4 -5', 'right_child'),
    ('leaf_value=0.25 0.5', 'leaf_value=0.25 0.5 1', 'leaf_value'),
    ('leaf_value=8\n', 'leaf_value=8 9\n', 'leaf_value'),
])
def test_parser_refusals_name_the_line(hand, old, new, needle):
    from otto_amd.ranker.forest import ModelFormatError, parse_lightgbm_model
    text = _mutate(hand['model'], old, new)
    with pytest.raises(ModelFormatError) as e:
        parse_lightgbm_model(text)
    msg = str(e.value)
    assert msg.startswith('line ') and needle in msg
    lineno = int(msg.split()[1].rstrip(':'))
    assert needle in text.splitlines()[lineno - 1], (msg, text.splitlines()[lineno - 1])


def test_parser_ignores_what_follows_end_of_trees(hand):
    from otto_amd.ranker.forest import parse_lightgbm_model
    f = parse_lightgbm_model(hand['model'] + '\nTree=9\nnum_class=7\nthis is not a model line\n')
    assert f.n_trees == 4


def test_restatement_reproduces_the_hand_computed_rows(hand, hand_forest):
    X, leaf, score = hand_rows(hand)
    assert len(hand['rows']) >= 12 and all(r['why'] for r in hand['rows'])
    got = fr.leaves(hand_forest, X)
    assert np.array_equal(got, leaf), np.argwhere(got != leaf)
    assert np.array_equal(fr.raw_scores(hand_forest, X), score)
    # the fixture covers what it claims to cover
    flat = X.ravel()
    e = np.float32(1e-35)
    for v in (e, np.nextafter(e, np.float32(1)), np.float32(np.inf), np.float32(-np.inf), np.nextafter(np.float32(0.5), np.float32(1)),
              np.nextafter(np.float32(1.5), np.float32(2))):
        assert (flat == v).any(), v
    assert np.isnan(X).all(axis=1).any() and (np.signbit(flat) & (flat == 0)).any() and (~np.signbit(flat) & (flat == 0)).any()


def test_restatement_ensemble_and_topk_definitions():
    sc = np.array([1.0, np.nan, 2.0, 2.0, -0.0, 0.0, -np.inf, np.nan, 5.0])
    aid = np.arange(10, 19, dtype=np.int32)
    ta, ts, n, bad = fr.session_topk(sc, aid, np.array([0, 0, 8, 9, 9]), 8)
    assert bad == 0 and n.tolist() == [0, 8, 1, 0]
    assert ta[1].tolist() == [12, 13, 10, 14, 15, 16, 11, 17]         # ties by position, -0.0 == +0.0, NaN last by position
    assert np.signbit(ts[1, 3]) and not np.signbit(ts[1, 4]) and np.isnan(ts[1, 6:]).all() and ts[1, 5] == -np.inf
    assert ta[0].tolist() == [-1] * 8 and np.isneginf(ts[0]).all() and ta[2, 0] == 18
    ta, _, n, bad = fr.session_topk(sc, aid, np.array([0, 5, 3, 9]), 2)
    assert bad == 1 and n.tolist() == [2, 0, 2] and ta[0].tolist() == [12, 13] and ta[2].tolist() == [18, 13]


def _f32_neighbours(t32):
    out = [t32]
    for d in (np.float32(np.inf), np.float32(-np.inf)):
        if t32 != d:
            with np.errstate(over='ignore'):
                out.append(np.nextafter(t32, d, dtype=np.float32))
    return out


def test_threshold_equivalence(head_forest):
    """(double)x <= t  <=>  x <= t32 for the float32 values around t32 = the largest float32 <= t."""
    halfway = (np.float64(np.float32(1.5)) + np.float64(np.nextafter(np.float32(1.5), np.float32(2)))) / 2
    ts = list(np.unique(head_forest.threshold)) + [1e300, -1e300, np.inf, -np.inf, halfway, -halfway, 1.0000000180025095e-35]
    assert len(ts) > 100
    n_checked = 0
    for t in ts:
        t = np.float64(t)
        t32 = fr.floor_f32(t)
        assert t32.dtype == np.float32 and np.float64(t32) <= t
        if np.isfinite(t32) or t32 > 0:
            with np.errstate(over='ignore'):
                up = np.nextafter(t32, np.float32(np.inf), dtype=np.float32)
            assert t32 == np.inf or np.float64(up) > t, 't32 is not the largest float32 <= t'
        for x in _f32_neighbours(t32):
            assert x.dtype == np.float32
            assert (np.float64(x) <= t) == (x <= t32), (t, t32, x)
            n_checked += 1
    assert fr.floor_f32(1e300) == np.finfo(np.float32).max and fr.floor_f32(-1e300) == -np.inf
    assert fr.floor_f32(halfway) == np.float32(1.5) and fr.floor_f32(1.5000000000000002) == np.float32(1.5)
    assert n_checked >= 3 * 100


# ---- otto_forest_pack: a host function of the library

@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from otto_amd import _lib
    return _lib.lib()


def _image_sections(img):
    magic, version, T, F, n_groups, max_leaves, total_nodes, total_leaves, total_bytes, off_trees, off_groups, off_blob = \
        struct.unpack_from('<IIiiiiiiqqqq', img, 0)
    return dict(magic=magic, version=version, T=T, F=F, n_groups=n_groups, max_leaves=max_leaves, total_nodes=total_nodes,
                total_leaves=total_leaves, total_bytes=total_bytes, off_trees=off_trees, off_groups=off_groups, off_blob=off_blob)


def test_pack_accepts_both_fixtures_and_holds_t32(lib, hand_forest, head_forest):
    for f in (hand_forest, head_forest):
        img = f.pack()
        h = _image_sections(img.tobytes())
        assert h['magic'] == 0x3152464F and h['T'] == f.n_trees and h['F'] == f.n_features and h['total_bytes'] == img.size
        assert h['total_nodes'] == f.threshold.size and h['total_leaves'] == f.leaf_value.size and h['max_leaves'] == f.num_leaves.max()
        raw = img.tobytes()
        for t in range(f.n_trees):
            off16, L = struct.unpack_from('<Ii', raw, h['off_trees'] + 8 * t)
            assert L == f.num_leaves[t]
            base, n0 = h['off_blob'] + 16 * off16, int(f.node_off[t])
            nodes = np.frombuffer(raw, dtype=np.uint32, count=4 * (L - 1), offset=base).reshape(L - 1, 4)
            want = np.array([fr.floor_f32(x) for x in f.threshold[n0:n0 + L - 1]], dtype=np.float32)
            assert np.array_equal(nodes[:, 0].view(np.float32), want), 'the image holds t32'
            assert np.array_equal(nodes[:, 1] & 0xFFFF, f.split_feature[n0:n0 + L - 1])
            assert np.array_equal(nodes[:, 2].view(np.int32), f.left_child[n0:n0 + L - 1])
            lv = np.frombuffer(raw, dtype=np.float64, count=L, offset=base + 16 * (L - 1))
            assert np.array_equal(lv, f.leaf_value[int(f.leaf_off[t]):int(f.leaf_off[t]) + L])
    # 8 trees of 128 leaves are one LDS group
    assert _image_sections(head_forest.pack().tobytes())['n_groups'] == 1


def _copy(f, **changes):
    from otto_amd.ranker.forest import Forest
    a = {k: getattr(f, k).copy() for k in ('node_off', 'leaf_off', 'split_feature', 'threshold', 'decision_type', 'left_child',
                                           'right_child', 'leaf_value')}
    for k, (i, v) in changes.items():
        a[k][i] = v
    return Forest(n_features=f.n_features, **a)


@pytest.mark.parametrize('name,changes,needle', [
    ('cycle', {'right_child': (4, 0)}, 'reached twice'),                     # T3 n1 -> right back to its root n0
    ('unreachable leaf', {'right_child': (5, -3)}, 'reached twice'),         # T3 n2: both children leaf 2, leaf 3 orphaned
    ('feature index', {'split_feature': (2, 3)}, 'split_feature'),
    ('categorical bit', {'decision_type': (0, 3)}, 'categorical'),
    ('non-finite leaf', {'leaf_value': (5, np.inf)}, 'non-finite'),
    ('NaN leaf', {'leaf_value': (0, np.nan)}, 'non-finite'),
    ('child out of range', {'left_child': (3, 3)}, 'outside the tree'),
    ('leaf out of range', {'left_child': (2, -3)}, 'outside the tree'),
])
def test_pack_refuses(lib, hand_forest, name, changes, needle):
    from otto_amd import _lib
    bad = _copy(hand_forest, **changes)
    with pytest.raises(_lib.OttoError, match=needle):
        bad.pack()
    with pytest.raises(ValueError):
        fr.validate(bad)


def test_pack_refuses_an_orphaned_subtree_and_the_limits(lib, hand_forest):
    from otto_amd import _lib
    from otto_amd.ranker.forest import Forest, MAX_FEATURES, MAX_LEAVES
    # T3: the root's right child skips n1 (n0 -> n2), n1 and its leaf hang in the air
    with pytest.raises(_lib.OttoError, match='unreachable'):
        _copy(hand_forest, right_child=(3, 2)).pack()
    f = hand_forest
    with pytest.raises(_lib.OttoError, match='F must be'):
        Forest(f.node_off, f.leaf_off, f.split_feature, f.threshold, f.decision_type, f.left_child, f.right_child, f.leaf_value,
               MAX_FEATURES + 1).pack()
    big = fr.random_forest(np.random.default_rng(0), 1, MAX_LEAVES + 1, 3, shape='left_chain')
    with pytest.raises(_lib.OttoError, match='leaves outside'):
        big.pack()
    fr.random_forest(np.random.default_rng(0), 1, MAX_LEAVES, 3, shape='left_chain').pack()
    assert lib.otto_forest_packed_bytes(0, 0, 0) == 0 and lib.otto_forest_packed_bytes(2, 5, 5) == 0


def test_engines_refuse_cpu_tensors(hand_forest):
    import torch
    from otto_amd import _lib
    from otto_amd.ranker import forest as fo
    X = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(_lib.OttoError):
        fo.forest_predict(hand_forest, X)
    with pytest.raises(_lib.OttoError):
        fo.ensemble_predict([hand_forest], X)
    with pytest.raises(_lib.OttoError):
        fo.session_topk(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4]), k=2)
    with pytest.raises(_lib.OttoError):
        hand_forest.to('cpu')
