"""The device feature tables and the feature matrix at the sizes their kernels branch on (tests/feat_edge_inputs.py; what
each input holds is asserted in tests/test_feat_edge_inputs_cpu.py), against the NumPy restatement of SPEC-FEAT
(tests/feat_restatement.py), bit for bit and column by column."""
import numpy as np
import pytest

import feat_edge_inputs as fe
import feat_inputs as fi
import feat_restatement as fr
from test_feat_gpu import _check, _dev, _matrix, _tables

pytestmark = pytest.mark.gpu


def _want(case):
    aid, ts, typ, off, n_aids = case[:5]
    want_a = fr.aid_table(aid, ts, typ, off, n_aids)
    return want_a, fr.session_table(aid, ts, typ, off, want_a)


def _aid_case(gpu_device, case, want):
    """Both tables of the case on the device against the restatement; the rows of absent aids are NaN in every column."""
    aid, ts, typ, off, n_aids = case[:5]
    at, st = _tables(gpu_device, aid, ts, typ, off, n_aids)
    assert tuple(at.shape) == (n_aids, 31) and tuple(st.shape) == (len(off) - 1, 15)
    _check(at, st, *want)
    got = at.cpu().numpy()
    present = np.bincount(aid, minlength=n_aids) > 0
    assert np.isnan(got[~present]).all()
    assert not np.isnan(got[present][:, [0, 28, 29]]).any()                 # a skipped aid would show as NaN or as leftover memory
    return at


@pytest.fixture(scope='module')
def stride():
    case = fe.stride()
    return case, _want(case)


@pytest.fixture(scope='module')
def sess_table():
    """The aid table of `sess_lengths` and `sess_errors`, from its own smaller event set: NaN rows for aids 500 .. 599."""
    return fr.aid_table(*fe.sess_table_events())


def test_stride(gpu_device, stride):
    case, want = stride
    _aid_case(gpu_device, case, want)


def test_stride_with_an_aid_beyond_the_table(gpu_device, stride):
    from otto_amd import _lib
    from otto_amd.ranker import features as ft
    case, want = stride
    aid, ts, typ, off, n_aids, _ = fe.stride_bad_aid()
    with pytest.raises(_lib.OttoError, match='bad inputs'):
        ft.aid_feature_table(*_dev(gpu_device, aid, ts, typ, off), n_aids)
    _aid_case(gpu_device, case, want)                                       # and the next call on the device is right


def test_hot_stride(gpu_device):
    case = fe.hot_stride()
    aid, ts, typ, off, n_aids, facts = case
    want_a = fr.aid_table(aid, ts, typ, off, n_aids)
    from otto_amd.ranker import features as ft
    at, _ = ft.aid_feature_table(*_dev(gpu_device, aid, ts, typ, off), n_aids)
    got = at.cpu().numpy()
    for q, name in enumerate(fr.AID_COLUMNS):
        assert fi.same(got[:, q], want_a[:, q]), (name, np.flatnonzero(got[:, q].view(np.uint32) != want_a[:, q].view(np.uint32))[:8])
    assert np.isnan(got[facts['absent']]).all() and not np.isnan(got[facts['counts'] > 0][:, [0, 28, 29]]).any()


def test_hot_edges(gpu_device):
    case = fe.hot_edges()
    _aid_case(gpu_device, case, _want(case))


def test_runs(gpu_device):
    case = fe.runs()
    _aid_case(gpu_device, case, _want(case))


def test_weeks(gpu_device):
    case = fe.weeks()
    _aid_case(gpu_device, case, _want(case))


def test_tiny(gpu_device):
    for case in fe.tiny():
        at = _aid_case(gpu_device, case, _want(case))
        if len(case[0]) == 0:
            assert tuple(at.shape) == (3, 31) and np.isnan(at.cpu().numpy()).all()


def _session_case(gpu_device, case, table):
    """The session table of the case over the restatement's aid table (uploaded as it is) against the restatement."""
    from otto_amd.ranker import features as ft
    aid, ts, typ, off = case[:4]
    want = fr.session_table(aid, ts, typ, off, table)
    got = ft.session_feature_table(*_dev(gpu_device, aid, ts, typ, off, table))
    assert tuple(got.shape) == (len(off) - 1, 15)
    got = got.cpu().numpy()
    for q, name in enumerate(fr.SESSION_COLUMNS):
        assert fi.same(got[:, q], want[:, q]), (name, np.flatnonzero(got[:, q].view(np.uint32) != want[:, q].view(np.uint32))[:8])
    return got


def test_sess_stride(gpu_device, stride):
    case = fe.sess_stride()
    got = _session_case(gpu_device, case, stride[1][0])
    lens = np.diff(case[3])
    assert np.array_equal(got[:, 0], lens.astype(np.float32))               # every session written, none twice over another
    assert (got[lens == 0, 1] == 0).all() and np.isnan(got[lens == 0, 2:]).all()


def test_sess_lengths(gpu_device, sess_table):
    case = fe.sess_lengths()
    got = _session_case(gpu_device, case, sess_table)
    facts = case[5]
    wrapped = {255: 255, 256: 0, 257: 1, 512: 0, 1: 1}
    for s, d in facts['distinct'].items():
        assert got[s, 1] == wrapped[d]
    assert np.isnan(got[facts['all_nan'], 5:]).all() and got[facts['all_nan'], 0] == 10


@pytest.mark.parametrize('name', ['too_long', 'aid_beyond_the_table'])
def test_sess_errors(gpu_device, sess_table, name):
    from otto_amd import _lib
    from otto_amd.ranker import features as ft
    aid, ts, typ, off, n_aids = fe.sess_errors()[name]
    assert n_aids == sess_table.shape[0]
    with pytest.raises(_lib.OttoError, match='bad inputs'):
        ft.session_feature_table(*_dev(gpu_device, aid, ts, typ, off, sess_table))
    ok = fe.sess_errors()['too_long']
    short = (ok[0][:3], ok[1][:3], ok[2][:3], ok[3][:2])                    # its first session alone: a valid call
    _session_case(gpu_device, short, sess_table)


def _matrix_case(gpu_device, sizes, F, seed):
    from otto_amd.ranker import interaction_feature_engineering as ife
    m, names = fe.matrix_case(sizes, F, seed)
    prog = fr.resolve(names, ife.ROW_COLUMNS, ife.SESSION_COLUMNS, ife.AID_COLUMNS)
    want = fr.matrix(m['row_off'], m['cand'], m['score'], m['inter_row'], m['inter_sess'], m['inter_aid'], m['aid_tab'], m['sess_tab'], prog)
    got = _matrix(gpu_device, m, names)
    assert tuple(got.shape) == (sum(sizes), F)
    got = got.cpu().numpy()
    bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
    assert fi.same(got, want), (names, bad[:8])


@pytest.mark.parametrize('n_rows,F', fe.matrix_pairs())
def test_matrix_rows_and_columns(gpu_device, n_rows, F):
    _matrix_case(gpu_device, fe.matrix_sizes(n_rows), F, seed=1000 * F + n_rows)


@pytest.mark.parametrize('F', fe.MATRIX_F)
def test_matrix_big_sessions(gpu_device, F):
    _matrix_case(gpu_device, fe.BIG_SESSIONS, F, seed=7000 + F)
