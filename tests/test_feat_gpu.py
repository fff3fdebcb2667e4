"""The device feature tables and the feature matrix (include/otto_feat.h, otto_amd.ranker.features) against the NumPy
restatement of SPEC-FEAT (tests/feat_restatement.py). Every column is compared bit for bit: all sums are exact integers
or float64 sums in event order on both sides."""
import os

import numpy as np
import pytest

import feat_inputs as fi
import feat_restatement as fr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _dev(gpu_device, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device) for a in arrays]


def _tables(gpu_device, aid, ts, typ, off, n_aids):
    from otto_amd.ranker import features as ft
    d = _dev(gpu_device, aid, ts, typ, off)
    at, names = ft.aid_feature_table(*d, n_aids)
    assert names == fr.AID_COLUMNS
    st = ft.session_feature_table(*d, at)
    return at, st


def _check(got_a, got_s, want_a, want_s):
    got_a, got_s = got_a.cpu().numpy(), got_s.cpu().numpy()
    for q, name in enumerate(fr.AID_COLUMNS):
        assert fi.same(got_a[:, q], want_a[:, q]), (name, np.flatnonzero(got_a[:, q].view(np.uint32) != want_a[:, q].view(np.uint32))[:8])
    for q, name in enumerate(fr.SESSION_COLUMNS):
        assert fi.same(got_s[:, q], want_s[:, q]), (name, np.flatnonzero(got_s[:, q].view(np.uint32) != want_s[:, q].view(np.uint32))[:8])


@pytest.fixture(scope='module')
def edge():
    aid, ts, typ, off, n_aids = fi.edge_events()
    want_a = fr.aid_table(aid, ts, typ, off, n_aids)
    want_s = fr.session_table(aid, ts, typ, off, want_a)
    return aid, ts, typ, off, n_aids, want_a, want_s


def test_edge_shapes_are_what_the_kernels_branch_on(edge):
    aid, ts, typ, off, n_aids, want_a, _ = edge
    counts = np.bincount(aid, minlength=n_aids)
    assert counts[:6].tolist() == [1, 63, 64, 65, 1025, 4097] and n_aids % 64 != 0 and (counts == 0).sum() == 12
    lengths = np.diff(off)
    assert lengths.max() == 512 and (lengths == 1).any()
    assert len(fr.week_slots(fr.calendar(ts)[3])) == 10
    day = fr.calendar(ts)[0]
    assert day.max() - day.min() == 63
    for col in (8, 9, 10, 13, 16, 19, 29):                                # ties in the ranked columns
        v = want_a[:, col][~np.isnan(want_a[:, col])]
        assert len(np.unique(v)) < len(v)


def test_tables_at_the_edge_shapes(gpu_device, edge):
    aid, ts, typ, off, n_aids, want_a, want_s = edge
    at, st = _tables(gpu_device, aid, ts, typ, off, n_aids)
    _check(at, st, want_a, want_s)
    assert np.isnan(at.cpu().numpy()[np.bincount(aid, minlength=n_aids) == 0]).all()


def test_tables_on_the_reference_input_and_the_hand_case(gpu_device):
    from test_feat_cpu import hand_case
    g = np.load(os.path.join(GOLDEN, 'feat_golden.npz'))
    n_aids = int(g['aid'].max()) + 1
    want_a = fr.aid_table(g['aid'], g['ts'], g['type'], g['sess_off'], n_aids)
    at, st = _tables(gpu_device, g['aid'], g['ts'], g['type'], g['sess_off'], n_aids)
    _check(at, st, want_a, fr.session_table(g['aid'], g['ts'], g['type'], g['sess_off'], want_a))
    aid, ts, typ, off, n_aids, want_a, want_s = hand_case()
    _check(*_tables(gpu_device, aid, ts, typ, off, n_aids), want_a, want_s)


def test_one_week_only_and_a_session_table_over_other_events(gpu_device):
    """One week: every pct_change is NaN. Then the reference's submission mode: the aid table over all events, the session
    table over the later half of the sessions only."""
    from otto_amd.ranker import features as ft
    rng = np.random.default_rng(3)
    aid, ts, typ, off, n_aids = fi.events(rng.integers(0, 9, 70).tolist(), 6, seed=4)
    ts = (ts + 86400).astype(np.int32)                                    # Monday .. Saturday of one ISO week
    assert len(fr.week_slots(fr.calendar(ts)[3])) == 1
    want_a = fr.aid_table(aid, ts, typ, off, n_aids)
    assert np.isnan(want_a[:, 25:28]).all()
    at, st = _tables(gpu_device, aid, ts, typ, off, n_aids)
    _check(at, st, want_a, fr.session_table(aid, ts, typ, off, want_a))
    h = (len(off) - 1) // 2
    e0 = off[h]
    sub = (aid[e0:], ts[e0:], typ[e0:], off[h:] - e0)
    got = ft.session_feature_table(*_dev(gpu_device, *sub), at)
    want = fr.session_table(*sub, want_a)
    assert fi.same(got.cpu().numpy(), want)


def test_a_span_of_64_days_is_an_error(gpu_device):
    from otto_amd import _lib
    from otto_amd.ranker import features as ft
    aid = np.array([0, 1], dtype=np.int32)
    ts = np.array([fi.SUNDAY, fi.SUNDAY + 64 * 86400], dtype=np.int32)
    typ = np.zeros(2, dtype=np.uint8)
    off = np.array([0, 1, 2], dtype=np.int64)
    d = _dev(gpu_device, aid, ts, typ, off)
    with pytest.raises(_lib.OttoError, match='days'):
        ft.aid_feature_table(*d, 2)
    ok = _dev(gpu_device, aid, np.array([fi.SUNDAY, fi.SUNDAY + 63 * 86400], dtype=np.int32), typ, off)
    at, _ = ft.aid_feature_table(*ok, 2)                                  # 63 days apart: fine, and the device still works
    with pytest.raises(_lib.OttoError, match='days'):
        ft.session_feature_table(*d, at)
    with pytest.raises(_lib.OttoError, match='bad inputs'):
        ft.aid_feature_table(*ok, 1)                                      # aid 1 >= n_aids: the error word, no fault


def _matrix_inputs(rng, sizes, n_aids):
    row_off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    R, S = int(row_off[-1]), len(sizes)
    holes = lambda a: np.where(rng.random(a.shape) < 0.1, np.float32(np.nan), a).astype(np.float32)
    inter_row = rng.integers(0, 4, (R, 5)).astype(np.uint16)
    return {'row_off': row_off, 'cand': rng.integers(0, n_aids, R).astype(np.int32), 'score': rng.standard_normal(R).astype(np.float32),
            'inter_row': inter_row, 'inter_sess': holes(rng.standard_normal((S, 10))), 'inter_aid': holes(rng.standard_normal((n_aids, 9))),
            'aid_tab': holes(rng.standard_normal((n_aids, 31))), 'sess_tab': holes(rng.standard_normal((S, 15)))}


def _matrix(gpu_device, m, names):
    from otto_amd.ranker import features as ft
    d = dict(zip(m, _dev(gpu_device, *[m[k].view(np.int16) if k == 'inter_row' else m[k] for k in m])))
    table = {'row_off': d['row_off'], 'candidates': d['cand'], 'candidate_scores': d['score']}
    return ft.feature_matrix(table, d['inter_row'], d['inter_sess'], d['inter_aid'], d['aid_tab'], d['sess_tab'], names)


def _all_names():
    from otto_amd.ranker import interaction_feature_engineering as ife
    return ['candidate_scores'] + list(ife.ROW_COLUMNS) + list(ife.SESSION_COLUMNS) + list(ife.AID_COLUMNS) + list(fr.AID_COLUMNS) + \
        list(fr.SESSION_COLUMNS)


@pytest.mark.parametrize('n_rows', [0, 1, 63, 65, 5001])
def test_matrix_against_a_numpy_gather(gpu_device, n_rows):
    from otto_amd.ranker import interaction_feature_engineering as ife
    from otto_amd.ranker.forest import load_lightgbm_model
    rng = np.random.default_rng(100 + n_rows)
    sizes = []
    while sum(sizes) < n_rows:
        sizes.append(min(int(rng.integers(0, 130)), n_rows - sum(sizes)))
    sizes = [0] + sizes + [0, 0]                                          # empty sessions at both ends and inside
    if n_rows > 100:
        sizes.insert(3, 0)
    m = _matrix_inputs(rng, sizes, n_aids=997)
    every = _all_names()
    model = load_lightgbm_model(os.path.join(GOLDEN, 'forest_order_fold1_head.lgb.txt')).feature_names
    for names in (['session_candidate_cumcount_last'], model, rng.permutation(model).tolist(), rng.permutation(every)[:64].tolist()):
        prog = fr.resolve(names, ife.ROW_COLUMNS, ife.SESSION_COLUMNS, ife.AID_COLUMNS)
        want = fr.matrix(m['row_off'], m['cand'], m['score'], m['inter_row'], m['inter_sess'], m['inter_aid'], m['aid_tab'], m['sess_tab'], prog)
        got = _matrix(gpu_device, m, names)
        assert got.shape == (n_rows, len(names)) and fi.same(got.cpu().numpy(), want), len(names)
    if n_rows:
        assert np.isnan(fr.matrix(m['row_off'], m['cand'], m['score'], m['inter_row'], m['inter_sess'], m['inter_aid'], m['aid_tab'],
                                  m['sess_tab'], [(fr.SRC_INTER_ROW, 1)])[m['inter_row'][:, 1] == 0]).all()


def test_matrix_refuses_a_bad_candidate(gpu_device):
    from otto_amd import _lib
    rng = np.random.default_rng(9)
    m = _matrix_inputs(rng, [3, 0, 70], n_aids=50)
    for bad in (-1, 50):
        m['cand'][40] = bad
        with pytest.raises(_lib.OttoError, match='bad inputs'):
            _matrix(gpu_device, m, ['candidate_scores', 'aid_count'])
    m['cand'][40] = 49
    assert _matrix(gpu_device, m, ['aid_count']).shape == (73, 1)


def test_events_to_top20_matches_the_forest_on_the_gathered_matrix(gpu_device):
    """About 200 sessions: candidate rows -> interaction features -> aid and session tables -> feature_matrix with the model's
    feature_names -> forest scores -> top-20, against the same forest on the matrix NumPy gathers from the same tables."""
    import torch
    from otto_amd.ranker import features as ft
    from otto_amd.ranker import forest as fo
    from otto_amd.ranker import interaction_feature_engineering as ife
    rng = np.random.default_rng(21)
    aid, ts, typ, off, n_aids = fi.events(rng.integers(1, 40, 150).tolist(), 28, seed=22, max_len=30)
    S = len(off) - 1
    assert 150 <= S <= 400
    cands = []
    for s in range(S):
        own = np.unique(aid[off[s]:off[s + 1]])
        cands.append(np.r_[own, rng.permutation(np.setdiff1d(np.arange(n_aids), own))[:40]].astype(np.int32))
    row_off = np.r_[0, np.cumsum([len(c) for c in cands])].astype(np.int64)
    cand = np.concatenate(cands)
    score = rng.integers(1, 30, len(cand)).astype(np.float32)
    d_aid, d_ts, d_typ, d_off, d_cand, d_score, d_row_off = _dev(gpu_device, aid, ts, typ, off, cand, score, row_off)
    table = {'candidates': d_cand, 'candidate_scores': d_score, 'row_off': d_row_off}
    row, sf, af = ife.interaction_features_rows(d_aid, d_typ, d_off, table, n_aids)
    at, _ = ft.aid_feature_table(d_aid, d_ts, d_typ, d_off, n_aids)
    st = ft.session_feature_table(d_aid, d_ts, d_typ, d_off, at)
    forest = fo.load_lightgbm_model(os.path.join(GOLDEN, 'forest_order_fold1_head.lgb.txt'))
    X = ft.feature_matrix(table, row, sf, af, at, st, forest.feature_names)
    prog = fr.resolve(forest.feature_names, ife.ROW_COLUMNS, ife.SESSION_COLUMNS, ife.AID_COLUMNS)
    want_X = fr.matrix(row_off, cand, score, row.cpu().numpy().view(np.uint16), sf.cpu().numpy(), af.cpu().numpy(), at.cpu().numpy(),
                       st.cpu().numpy(), prog)
    assert fi.same(X.cpu().numpy(), want_X)
    assert fi.same(at.cpu().numpy(), fr.aid_table(aid, ts, typ, off, n_aids))
    got = fo.rank_candidates([forest], X, d_cand, d_row_off, k=20)
    want = fo.rank_candidates([forest], torch.from_numpy(want_X).to(gpu_device), d_cand, d_row_off, k=20)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert len(torch.unique(got[1][:, 0])) > 10                           # the scores tell the sessions apart
