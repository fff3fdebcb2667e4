"""SPEC-FOREST on the device (csrc/otto_forest.hip) against the float64 restatement (tests/forest_restatement.py).

Everything is bit-exact: routing compares against t32 = the largest float32 <= the model's float64 threshold, which
decides exactly as the float64 comparison does (test_forest_cpu.py::test_threshold_equivalence), and a row's leaf values
are added in tree order in float64. So np.array_equal on scores, ids and counts; no tolerance anywhere."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import forest_restatement as fr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HEAD = os.path.join(GOLDEN, 'forest_order_fold1_head.lgb.txt')
GROUP_TREES_128 = 8        # OTTO_FOREST_GROUP_BYTES // (127 * 16 + 128 * 8): trees of 128 leaves per LDS group


def _t(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _predict(forest, X, dev):
    from otto_amd.ranker.forest import forest_leaves, forest_predict
    Xd = _t(X, dev)
    return forest_predict(forest, Xd).cpu().numpy(), forest_leaves(forest, Xd).cpu().numpy()


def _check(forest, X, dev, want_leaf=None):
    want_leaf = fr.leaves(forest, X) if want_leaf is None else want_leaf
    want = fr.raw_scores(forest, X, want_leaf)
    got, got_leaf = _predict(forest, X, dev)
    assert got.dtype == np.float64 and got.shape == (X.shape[0],) and got_leaf.dtype == np.int32
    assert np.array_equal(got_leaf, want_leaf), f'{(got_leaf != want_leaf).sum()} leaves differ'
    assert np.array_equal(_bits(got), _bits(want)), f'{(got != want).sum()} scores differ'


def test_hand_fixture(gpu_device):
    from otto_amd.ranker.forest import parse_lightgbm_model
    with open(os.path.join(GOLDEN, 'forest_hand.json')) as f:
        hand = json.load(f)
    forest = parse_lightgbm_model(hand['model'])
    X = np.array([[np.float32(s) for s in r['x']] for r in hand['rows']], dtype=np.float32)
    got, got_leaf = _predict(forest, X, gpu_device)
    assert got_leaf.tolist() == [r['leaves'] for r in hand['rows']]
    assert got.tolist() == [r['score'] for r in hand['rows']]


# ---- the 8-tree head of the reference's order model

@pytest.fixture(scope='module')
def head():
    """(forest, X float32 [1000, 54], leaves, scores): each column uniform over its feature_infos range, then 10 % NaN,
    10 % an exact t32 of a node on that feature, 5 % the float32 next above one, a few +-0, +-1e-35f, +-inf."""
    from otto_amd.ranker.forest import load_lightgbm_model
    forest = load_lightgbm_model(HEAD)
    with open(HEAD) as fh:
        infos = [l for l in fh.read().splitlines() if l.startswith('feature_infos=')][0].split('=', 1)[1].split()
    rng = np.random.default_rng(54)
    n, F = 1000, forest.n_features
    assert len(infos) == F
    X = np.empty((n, F), dtype=np.float32)
    for f, info in enumerate(infos):
        lo, hi = (float(v) for v in info.strip('[]').split(':'))
        X[:, f] = rng.uniform(lo, hi, n).astype(np.float32)
        t32 = np.array([fr.floor_f32(t) for t in forest.threshold[forest.split_feature == f]], dtype=np.float32)
        m = rng.random(n)
        X[m < 0.10, f] = np.nan
        if t32.size:
            pick = (m >= 0.10) & (m < 0.20)
            X[pick, f] = t32[rng.integers(0, t32.size, int(pick.sum()))]
            pick = (m >= 0.20) & (m < 0.25)
            with np.errstate(over='ignore'):
                X[pick, f] = np.nextafter(t32[rng.integers(0, t32.size, int(pick.sum()))], np.float32(np.inf), dtype=np.float32)
        pick = (m >= 0.25) & (m < 0.28)
        specials = np.array([0.0, -0.0, 1e-35, -1e-35, np.inf, -np.inf], dtype=np.float32)
        X[pick, f] = specials[rng.integers(0, specials.size, int(pick.sum()))]
    leaf = fr.leaves(forest, X)
    return forest, X, leaf, fr.raw_scores(forest, X, leaf)


@pytest.mark.parametrize('n_rows', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_real_fixture_rows(gpu_device, head, n_rows):
    forest, X, leaf, _ = head
    _check(forest, X[:n_rows], gpu_device, leaf[:n_rows])


def test_real_fixture_row_stride_above_F(gpu_device, head):
    import torch
    from otto_amd.ranker.forest import forest_predict
    forest, X, _, score = head
    wide = np.full((X.shape[0], 61), np.float32(7e9), dtype=np.float32)
    wide[:, :54] = X
    Xd = _t(wide, gpu_device)[:, :54]
    assert Xd.stride(0) == 61 and not Xd.is_contiguous()
    assert np.array_equal(_bits(forest_predict(forest, Xd).cpu().numpy()), _bits(score))
    assert forest_predict(forest, torch.empty((0, 54), dtype=torch.float32, device=gpu_device)).shape == (0,)


# ---- seeded synthetic forests: group edges, tree sizes, feature counts, the global-memory fallback

SYNTH = [  # (T, leaves, F, shape)
    (1, 128, 54, 'random'), (2, 128, 54, 'random'), (GROUP_TREES_128 - 1, 128, 54, 'random'), (GROUP_TREES_128, 128, 54, 'random'),
    (GROUP_TREES_128 + 1, 128, 54, 'random'), (31, 128, 54, 'random'), (32, 3, 1, 'random'), (33, 128, 1, 'random'),
    (65, 2, 54, 'random'), (285, 128, 54, 'random'), (33, 1, 54, 'random'), (2, 128, 128, 'random'), (31, 3, 128, 'random'),
    (3, 128, 54, 'left_chain'), (2, 2048, 54, 'left_chain'),        # above 1024 leaves a tree is walked from global memory
    (3, 2048, 128, 'random'), (2, 1024, 54, 'random'),              # 1024 leaves: 24,560 bytes, the largest tree that is staged
    (2, 1025, 54, 'random'),                                        # 24,584 bytes: the smallest that is not
]


@pytest.mark.parametrize('T,L,F,shape', SYNTH)
def test_synthetic_forest(gpu_device, T, L, F, shape):
    from otto_amd.ranker.forest import MAX_FEATURES, MAX_LEAVES
    assert MAX_LEAVES == 2048 and MAX_FEATURES == 128, 'the cases above name the limits'
    rng = np.random.default_rng([T, L, F])
    X = fr.random_rows(rng, 1000, F)
    _check(fr.random_forest(rng, T, L, F, X=X, shape=shape), X, gpu_device)


def test_synthetic_mixed_tree_sizes(gpu_device):
    """Small trees, a tree above the group budget in the middle, two trees that each fill most of a group."""
    import struct
    rng = np.random.default_rng(99)
    X = fr.random_rows(rng, 1000, 54)
    parts = [fr.random_forest(rng, 10, 3, 54, X=X), fr.random_forest(rng, 1, 2048, 54, X=X), fr.random_forest(rng, 9, 128, 54, X=X),
             fr.random_forest(rng, 2, 1, 54), fr.random_forest(rng, 2, 700, 54, X=X), fr.random_forest(rng, 1, 2048, 54, X=X, shape='left_chain')]
    forest = fr.concat_forests(parts)
    n_groups = struct.unpack_from('<i', forest.pack().tobytes(), 16)[0]
    assert forest.n_trees == 25 and n_groups == 6       # [10 x 3] [2048] [8 x 128] [128, 1, 1, 700] [700] [2048]
    _check(forest, X, gpu_device)


def test_ensemble_predict(gpu_device, head):
    from otto_amd.ranker.forest import ensemble_predict
    forest, X, _, score = head
    rng = np.random.default_rng(5)
    forests = [forest] + [fr.random_forest(rng, 9, 128, 54, X=X) for _ in range(4)]
    Xd = _t(X, gpu_device)
    for m in (1, 2, 5):
        want = fr.ensemble(forests[:m], X)
        got = ensemble_predict(forests[:m], Xd).cpu().numpy()
        again = ensemble_predict(forests[:m], Xd).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), f'{m} forests: {(got != want).sum()} scores differ'
        assert got.tobytes() == again.tobytes()
    assert not np.array_equal(fr.ensemble(forests[:1], X), score), 'the float32 cast of the fold formula is visible'


# ---- session top-k

def _topk_case(k):
    rng = np.random.default_rng(1000 + k)
    lens = [0, 1, k - 1, k, k + 1, 63, 64, 65, 300, 5000, 40, 40, 40, 0]
    lens = [max(l, 0) for l in lens]
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(row_off[-1])
    values = np.array([-2.5, -1.0, -0.0, 0.0, 0.75, 3.0, 1e300])
    score = values[rng.integers(0, values.size, n)]
    s_eq, s_zero, s_nan = len(lens) - 4, len(lens) - 3, len(lens) - 2
    score[row_off[s_eq]:row_off[s_eq + 1]] = 0.75                                     # all equal
    score[row_off[s_zero]:row_off[s_zero + 1]] = np.where(rng.random(40) < 0.5, -0.0, 0.0)
    score[row_off[s_zero] + 7] = -3.0
    seg = score[row_off[s_nan]:row_off[s_nan + 1]]
    seg[rng.random(40) < 0.4] = np.nan
    seg[3], seg[11] = -np.inf, np.inf
    aid = rng.integers(0, 1 << 31, n).astype(np.int32)
    return score, aid, row_off


@pytest.mark.parametrize('k', [1, 20, 64])
def test_session_topk(gpu_device, k):
    from otto_amd.ranker.forest import session_topk
    score, aid, row_off = _topk_case(k)
    w_aid, w_score, w_n, bad = fr.session_topk(score, aid, row_off, k)
    assert bad == 0
    g_aid, g_score, g_n = (t.cpu().numpy() for t in session_topk(_t(score, gpu_device), _t(aid, gpu_device), _t(row_off, gpu_device), k=k))
    assert g_aid.shape == (row_off.size - 1, k) and g_aid.dtype == np.int32 and g_score.dtype == np.float64 and g_n.dtype == np.int32
    assert np.array_equal(g_n, w_n) and np.array_equal(g_aid, w_aid)
    assert np.array_equal(_bits(g_score), _bits(w_score)), 'scores differ (bitwise: -0.0 and NaN included)'
    empty = session_topk(_t(score[:0], gpu_device), _t(aid[:0], gpu_device), _t(np.zeros(3, dtype=np.int64), gpu_device), k=k)
    assert empty[2].cpu().tolist() == [0, 0] and (empty[0].cpu().numpy() == -1).all()


def _raw_topk(lib, score, aid, row_off, k, dev):
    import torch
    S = row_off.numel() - 1
    out = (torch.full((S, k), 77, dtype=torch.int32, device=dev), torch.zeros((S, k), dtype=torch.float64, device=dev),
           torch.full((S,), 77, dtype=torch.int32, device=dev))
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.otto_forest_session_topk(p(score), p(aid), p(row_off), S, score.numel(), k, p(out[0]), p(out[1]), p(out[2]),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return rc, tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize('damage', ['decreasing', 'beyond n_rows', 'negative'])
def test_session_topk_bad_row_off(gpu_device, damage):
    from otto_amd import _lib
    from otto_amd.ranker.forest import session_topk
    lib = _lib.lib()
    score, aid, row_off = _topk_case(20)
    row_off = row_off.copy()
    if damage == 'decreasing':
        row_off[9] = row_off[8] - 5              # session 8 = [off8, off8 - 5): invalid; session 9 starts 5 rows early: valid
    elif damage == 'beyond n_rows':
        row_off[-1] = score.size + 1
    else:
        row_off[0] = -1
    w_aid, w_score, w_n, bad = fr.session_topk(score, aid, row_off, 20)
    assert bad == 1
    rc, (g_aid, g_score, g_n) = _raw_topk(lib, _t(score, gpu_device), _t(aid, gpu_device), _t(row_off, gpu_device), 20, gpu_device)
    assert rc == -22 and b'row_off' in lib.otto_last_error()
    assert np.array_equal(g_n, w_n) and np.array_equal(g_aid, w_aid) and np.array_equal(_bits(g_score), _bits(w_score))
    with pytest.raises(_lib.OttoError):
        session_topk(_t(score, gpu_device), _t(aid, gpu_device), _t(row_off, gpu_device), k=20)


def test_rank_candidates_end_to_end(gpu_device, head):
    from otto_amd.ranker.forest import rank_candidates
    forest, X, _, _ = head
    rng = np.random.default_rng(8)
    forests = [forest, fr.random_forest(rng, 3, 128, 54, X=X)]
    lens = [0, 100, 1, 37, 0, 64, 20, 21, 500, 257, 0]
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert row_off[-1] == X.shape[0]
    aid = rng.integers(0, 1855603, X.shape[0]).astype(np.int32)
    want = fr.session_topk(fr.ensemble(forests, X), aid, row_off, 20)
    got = [t.cpu().numpy() for t in rank_candidates(forests, _t(X, gpu_device), _t(aid, gpu_device), _t(row_off, gpu_device), k=20)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[2], want[2])


def test_damaged_image_is_refused_not_walked_forever(gpu_device, head):
    """Child indices overwritten after packing so that the root of one tree and one of its children point at each other:
    the walk is bounded by L - 1 steps, the call returns OTTO_EINVAL. The bad indices stay inside the tree, so nothing
    is read out of bounds."""
    import struct
    import torch
    from otto_amd import _lib
    lib = _lib.lib()
    forest, X, _, score = head
    img = forest.pack().copy()
    off_trees, _, off_blob = struct.unpack_from('<qqq', img.tobytes(), 40)
    off16, L = struct.unpack_from('<Ii', img.tobytes(), off_trees + 8 * 3)
    n0 = int(forest.node_off[3])
    child = max(int(forest.left_child[n0]), int(forest.right_child[n0]))
    assert L == 128 and 0 < child < L - 1, 'the root of tree 3 has an internal child'
    # both children of the root := that child, both of its children := the root: every row circles
    root = off_blob + 16 * off16
    img[root + 8:root + 16] = np.frombuffer(struct.pack('<ii', child, child), dtype=np.uint8)
    img[root + 16 * child + 8:root + 16 * child + 16] = np.frombuffer(struct.pack('<ii', 0, 0), dtype=np.uint8)
    d_img, Xd = _t(img, gpu_device), _t(X, gpu_device)
    raw = torch.zeros(X.shape[0], dtype=torch.float64, device=gpu_device)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    rc = lib.otto_forest_predict(p(d_img), img.size, p(Xd), 54, X.shape[0], 54, p(raw), None, 1.0, stream)
    assert rc == -22 and b'walk' in lib.otto_last_error()
    # a wrong size, a wrong F and a damaged header are refused before any tree is walked
    assert lib.otto_forest_predict(p(d_img), img.size - 16, p(Xd), 54, X.shape[0], 54, p(raw), None, 1.0, stream) == -22
    assert b'image' in lib.otto_last_error()
    assert lib.otto_forest_predict(p(d_img), img.size, p(Xd), 54, X.shape[0], 53, p(raw), None, 1.0, stream) == -22
    # the intact image still scores
    good = _t(forest.pack(), gpu_device)
    assert lib.otto_forest_predict(p(good), good.numel(), p(Xd), 54, X.shape[0], 54, p(raw), None, 1.0, stream) == 0
    assert np.array_equal(_bits(raw.cpu().numpy()), _bits(score))
