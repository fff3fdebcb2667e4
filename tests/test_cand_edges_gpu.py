"""``k_cand`` (csrc/otto_cand.hip) against oracle/cand_oracle.py on the hand-built inputs of tests/cand_inputs.py: every table
size, first-level partition count, split, sweep, select width, n_common, key field and work-list edge, in the plain lookup and
in ``otto_cand_lookup_self``. Everything is an integer and is compared exactly: the number of candidates, the candidates in
order, their counts, the -1 / 0 padding and the own counts. tests/test_cand_inputs_cpu.py proves that each case reaches the
branch it is named after."""
import ctypes as C

import numpy as np
import pytest

import cand_oracle as cdo
import cand_inputs as ci

pytestmark = pytest.mark.gpu
SENTINEL = -77
_want, _dev, _got = {}, {}, {}


def _sessions_of(case):
    if case.name == 'i-513-events':                           # the accepted call: the 513-event session cut to 512
        return [(a[:512], t[:512]) for a, t in case.sessions]
    return case.sessions


def expected(case, self_counts):
    """Per session (candidates, counts[, own]) from the oracle, computed once per case and mode; the work-list cases repeat
    a few templates, the oracle runs once per template."""
    key = (case.name, self_counts)
    if key not in _want:
        top, f = case.top(), cdo.session_candidates_self if self_counts else cdo.session_candidates
        sessions = _sessions_of(case)
        template = getattr(case, 'template', np.arange(len(sessions)))
        once = {}
        for s, t in enumerate(template.tolist()):
            if t not in once:
                once[t] = f(sessions[s][0], sessions[s][1], top, case.recipe, case.n_common)
        _want[key] = [once[t] for t in template.tolist()]
    return _want[key]


def device_inputs(case, dev):
    """Matrices and events of a case on the device; one case is kept (the 2^26-row matrices are built once for both modes)."""
    import torch
    if case.name not in _dev:
        _dev.clear()
        sessions = _sessions_of(case)
        aid = np.array([x for a, _ in sessions for x in a], dtype=np.uint32)
        typ = np.array([x for _, t in sessions for x in t], dtype=np.uint8)
        off = np.r_[0, np.cumsum([len(a) for a, _ in sessions])].astype(np.int64)
        _dev[case.name] = (case.device_matrices(dev), torch.from_numpy(aid.astype(np.int32)).to(dev), torch.from_numpy(typ).to(dev),
                           torch.from_numpy(off).to(dev), off)
    return _dev[case.name]


def lookup_prefilled(aid, typ, off, mats, recipe, n_common, self_counts):
    """The C-ABI called directly on outputs pre-filled with a sentinel: a session the work list skipped keeps it."""
    import torch
    from otto_amd import _lib
    from otto_amd.covisitation.candidates import SOURCES
    dev = aid.device
    kinds = list(dict.fromkeys(kind for kind, _ in recipe))
    p = _lib.CandParams()
    widths = [int(mats[kd][0].shape[1]) for kd in kinds]
    p.n_aids, p.n_matrices, p.k = int(mats[kinds[0]][0].shape[0]), len(kinds), min(max(widths), 32)
    for i, kind in enumerate(kinds):
        p.d_mat_y[i], p.d_mat_n[i], p.mat_k[i] = mats[kind][0].data_ptr(), mats[kind][-1].data_ptr(), widths[i]
    p.n_terms, p.n_common = len(recipe), n_common
    for t, (kind, src) in enumerate(recipe):
        p.term_matrix[t], p.term_source[t] = kinds.index(kind), SOURCES[src]
    S = off.numel() - 1
    cand, count = (torch.full((S, n_common), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2))
    n_out = torch.full((S,), SENTINEL, dtype=torch.int32, device=dev)
    own = torch.full((aid.numel(),), SENTINEL, dtype=torch.int32, device=dev)
    v = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if self_counts:
            _lib.check(_lib.lib().otto_cand_lookup_self(C.byref(p), v(aid), v(typ), v(off), S, v(cand), v(count), v(n_out), v(own), stream),
                       'otto_cand_lookup_self')
            return cand, count, n_out, own
        _lib.check(_lib.lib().otto_cand_lookup(C.byref(p), v(aid), v(typ), v(off), S, v(cand), v(count), v(n_out), stream), 'otto_cand_lookup')
    return cand, count, n_out


def compare(case, got, want, off, self_counts):
    """Every row of every output against the oracle, padding included."""
    cand, cnt, n = (t.cpu().numpy() for t in got[:3])
    S, nc = len(want), case.n_common
    assert cand.shape == (S, nc) and cnt.shape == (S, nc) and n.shape == (S,)
    w_cand, w_cnt = np.full((S, nc), -1, dtype=np.int32), np.zeros((S, nc), dtype=np.int32)
    w_n = np.array([len(w[0]) for w in want], dtype=np.int32)
    for s, w in enumerate(want):
        w_cand[s, :len(w[0])], w_cnt[s, :len(w[1])] = w[0], w[1]
    bad = np.flatnonzero((n != w_n) | (cand != w_cand).any(axis=1) | (cnt != w_cnt).any(axis=1))
    if len(bad):
        s = int(bad[0])
        k = int(np.flatnonzero(np.r_[(cand[s] != w_cand[s]) | (cnt[s] != w_cnt[s]), True])[0])
        pytest.fail(f'{case.name} ({case.branch}), self_counts={self_counts}: {len(bad)} of {S} sessions differ; session {s} '
                    f'({off[s + 1] - off[s]} events): n {n[s]} vs {w_n[s]}, first difference at rank {k}: '
                    f'got {cand[s, k:k + 4].tolist()} x {cnt[s, k:k + 4].tolist()}, want {w_cand[s, k:k + 4].tolist()} x {w_cnt[s, k:k + 4].tolist()}')
    if self_counts:
        own = got[3].cpu().numpy()
        w_own = np.array([x for w in want for x in w[2]], dtype=np.int32)
        assert own.shape == w_own.shape
        bad = np.flatnonzero(own != w_own)
        assert len(bad) == 0, f'{case.name}: own counts differ at {len(bad)} events, first {int(bad[0])}: {own[bad[0]]} vs {w_own[bad[0]]}'


def run_case(case, dev, self_counts):
    from otto_amd.covisitation.candidates import candidate_lookup
    mats, aid, typ, off_d, off = device_inputs(case, dev)
    if case.name.startswith('h-'):
        got = lookup_prefilled(aid, typ, off_d, mats, case.recipe, case.n_common, self_counts)
    else:
        got = candidate_lookup(aid, typ, off_d, mats, case.recipe, n_common=case.n_common, self_counts=self_counts)
    compare(case, got, expected(case, self_counts), off, self_counts)
    return got


@pytest.mark.parametrize('self_counts', [False, True], ids=['plain', 'self'])
@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n != 'i-513-events'])
def test_lookup_matches_oracle(gpu_device, name, self_counts):
    run_case(ci.case(name), gpu_device, self_counts)


@pytest.mark.parametrize('self_counts', [False, True], ids=['plain', 'self'])
def test_session_of_513_events_is_refused_and_512_accepted(gpu_device, self_counts):
    """One 513-event session between valid ones: the call raises; the same call with that session cut to 512 events -- the next
    call -- matches the oracle."""
    import torch
    from otto_amd import _lib
    from otto_amd.covisitation.candidates import candidate_lookup
    case = ci.case('i-513-events')
    aid, typ, off = case.events()
    mats = case.device_matrices(gpu_device)
    t = lambda a: torch.from_numpy(a).to(gpu_device)
    with pytest.raises(_lib.OttoError, match='longer than 512 events'):
        candidate_lookup(t(aid.astype(np.int32)), t(typ), t(off), mats, case.recipe, n_common=case.n_common, self_counts=self_counts)
    run_case(case, gpu_device, self_counts)


@pytest.mark.parametrize('n_frequent', [0, 20, 64])
@pytest.mark.parametrize('n_pred', [1, 20, 64])
def test_predictions_around_n_pred(gpu_device, n_pred, n_frequent):
    """``otto_cand_predictions`` on sessions with fewer, exactly and more unique aids than n_pred, rows filled by 0, 20 or 64
    frequent aids (rows are cut at n_pred: include/otto_cand.h)."""
    from otto_amd.covisitation.candidates import predictions
    case = ci.case('j-predictions')
    if (case.name, False) not in _got:
        _got[case.name, False] = run_case(case, gpu_device, False)
    cand, _, n = _got[case.name, False]
    _, aid, _, off_d, off = device_inputs(case, gpu_device)
    frequent = list(range(2900, 2900 + n_frequent))
    pred, n_out = (t.cpu().numpy() for t in predictions(aid, off_d, cand, n, frequent, n_pred=n_pred))
    kinds = set()
    for s, ((aids, _), (wa, _)) in enumerate(zip(case.sessions, expected(case, False))):
        wp = cdo.session_predictions(aids, wa, frequent, n_pred)[:n_pred]
        assert n_out[s] == len(wp) and pred[s, :len(wp)].tolist() == wp and (pred[s, len(wp):] == -1).all(), (s, pred[s].tolist(), wp)
        u = len(set(aids))
        kinds.add('fewer' if u < n_pred else ('exact' if u == n_pred else 'more'))
    assert kinds == ({'exact', 'more'} if n_pred == 1 else {'fewer', 'exact', 'more'})


@pytest.mark.parametrize('name', ['a-short-tot1537-distinct-r2', 'a-long-tot6145-distinct-r3'])
def test_ranker_table_of_split_cases(gpu_device, name):
    """``otto_cand_ranker_table`` over the lookup's output where the candidates come from split partitions."""
    import torch
    from otto_amd.covisitation.candidates import ranker_table
    case = ci.case(name)
    cand, cnt, n = run_case(case, gpu_device, False)
    _, aid, _, off_d, off = device_inputs(case, gpu_device)
    want = expected(case, False)
    lab = [sorted(set(w[0][::7] + aids[:3])) for (aids, _), w in zip(case.sessions, want)]
    l_off = torch.from_numpy(np.r_[0, np.cumsum([len(x) for x in lab])].astype(np.int64)).to(gpu_device)
    l_aid = torch.from_numpy(np.array([a for x in lab for a in x], dtype=np.int32)).to(gpu_device)
    tab = ranker_table(aid, off_d, cand, cnt, n, labels=(l_off, l_aid))
    ro = tab['row_off'].cpu().numpy()
    t_s, t_c, t_w, t_l = (tab[c].cpu().numpy() for c in ('session', 'candidates', 'candidate_scores', 'candidate_labels'))
    for s, ((aids, _), (wa, wc)) in enumerate(zip(case.sessions, want)):
        pred, sc, lb = cdo.session_ranker_rows(aids, wa, wc, lab[s])
        a, b = int(ro[s]), int(ro[s + 1])
        assert b - a == len(pred) and len(wa) == case.n_common
        assert t_c[a:b].tolist() == pred and t_w[a:b].tolist() == [float(v) for v in sc] and (t_s[a:b] == s).all()
        assert t_l[a:b].tolist() == lb and sum(lb) >= 10
    assert int(ro[-1]) == len(t_c)
