"""The interaction features of csrc/otto_inter.hip (include/otto_inter.h) against the pandas restatement
``oracle/inter_oracle.py`` (float64), at candidate counts around the wave width, session lengths at the end of the LDS
buffer, above the session count where the grid-stride loop starts, and with scores that exercise the order-preserving float
image (negative, mixed sign, both zeros) and the atomics (one aid that is a candidate of every session).

Integer columns and score min / max are compared exactly. Float columns keep the project's rtol = 1e-5, atol = 1e-6. The
scores are multiples of 2^-10 (or small integers), so their float64 sums are exact in any order, and they come from the
distributions for which ``tests/test_edge_cases_cpu.py`` shows the float64 one-pass variance to stay within 1e-6 of the two-pass
one: a miss of 1e-5 is then the kernel's, not the formula's."""
import numpy as np
import pytest

import edge_inputs as ei
import inter_oracle as io

pytestmark = pytest.mark.gpu

EXACT = ('session_candidate_score_min', 'session_candidate_score_max', 'aid_candidate_score_max')


def _compare(got, want, ife):
    key = ['session', 'candidates', 'candidate_scores']
    got = got.sort_values(key).reset_index(drop=True)
    want = want.sort_values(key).reset_index(drop=True)
    assert len(got) == len(want) and (got[key].to_numpy() == want[key].to_numpy()).all()
    for col in ife.ROW_COLUMNS + ife.SESSION_COLUMNS + ife.AID_COLUMNS:
        g, w = got[col].to_numpy().astype(np.float64), want[col].to_numpy().astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), col
        ok = ~np.isnan(w)
        if col in EXACT or (col.endswith(('_sum', '_max', '_min', 'occurrence_count', 'cumcount_last')) and 'score' not in col):
            assert np.array_equal(g[ok], w[ok]), col
        else:
            np.testing.assert_allclose(g[ok], w[ok].astype(np.float32), rtol=1e-5, atol=1e-6, err_msg=col)
    return got


def _dense(dev, aid, typ, off, cand, score, n_aids):
    import pandas as pd
    import torch
    from otto_amd.ranker import interaction_feature_engineering as ife
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    row, sf, af = ife.interaction_features(t(aid), t(typ), t(off), t(cand), t(score), n_aids)
    got = ife.to_frame(np.arange(len(off) - 1), t(cand), t(score), row, sf, af)
    keep = cand >= 0
    s_idx, _ = np.nonzero(keep)
    want = io.interaction_features(pd.DataFrame({'session': s_idx.astype(np.int64), 'candidates': cand[keep].astype(np.int64),
                                                 'candidate_scores': score[keep].astype(np.float64)}), ei.events_frame(aid, typ, off))
    return _compare(got, want, ife), sf.cpu().numpy(), af.cpu().numpy()


def _dense_case(C, S, lengths, n_aids, kind, seed, hot=None):
    rng = np.random.default_rng(seed)
    aid, typ, off = ei.inter_sessions(lengths, n_aids, seed)
    cand = np.full((S, C), -1, dtype=np.int32)
    score = np.zeros((S, C), dtype=np.float32)
    for s in range(S):
        n = C if s % 3 == 0 else int(rng.integers(0, C + 1))
        if hot is not None:
            n = max(n, 1)
        pick = ei.unique_candidates(rng, aid[off[s]:off[s + 1]], n_aids, n)
        if hot is not None and hot not in pick:
            pick[0] = hot
        cand[s, :n] = pick
        score[s, :n] = ei.inter_scores(kind, n, rng)
    return aid, typ, off, cand, score


@pytest.mark.parametrize('C,kind', [(1, 'mixed'), (63, 'fractional'), (64, 'negative'), (65, 'mixed'), (100, 'counts'), (128, 'mixed')])
def test_dense_candidate_counts_around_the_wave_width(gpu_device, C, kind):
    """Dense rows of C candidates (full rows, partly filled rows, empty rows); aid 0 is a candidate of every non-empty
    row (atomics under contention); one row lists an aid twice with different scores; one row holds +0.0 and -0.0."""
    S, n_aids = 400, 700
    lengths = np.random.default_rng(C).integers(1, 50, S)
    aid, typ, off, cand, score = _dense_case(C, S, lengths, n_aids, kind, seed=C, hot=0)
    if C >= 3:
        a, b = (1, 2) if cand[0, 1] != 0 else (2, 1)          # keep the hot aid in the row
        cand[0, a] = cand[0, b]
        score[0, a] = score[0, b] + 1
        score[3, 0], score[3, 1] = 0.0, -0.0
        if kind in ('negative', 'fractional'):      # both zeros are the extreme of the row on one side
            assert np.signbit(score[3, 1]) and not np.signbit(score[3, 0])
    got, sf, af = _dense(gpu_device, aid, typ, off, cand, score, n_aids)
    assert (got['session_candidate_occurrence_count'] > 0).any()
    assert (cand == 0).sum() >= S and not np.isnan(af[0]).any()


def test_grid_stride_loop_and_sessions_at_the_end_of_the_lds_buffer(gpu_device):
    """20,000 sessions: the launch is capped at 16,384, so every wave takes a second session and reuses its LDS rows. Lengths
    cycle through 1, 3, 4, 5, 509, 510, 511, 512; a wave's second session is 4096 x 4 = 16,384 further on, the same position of
    the cycle (16,384 mod 8 = 0) -- so the cycle is rotated by 3 in the second half and a short session follows a long
    one on the same wave: events of the long session left in LDS beyond ``n`` would be counted if the ``i0 + e < n`` guard
    were wrong, since the candidates of a short session are drawn from the aids of the long session before it."""
    S, n_aids, C = 20_000, 3000, 6
    cyc = np.array(ei.INTER_LONG_CYCLE)
    lengths = np.r_[cyc[np.arange(16_384) % 8], cyc[(np.arange(S - 16_384) + 3) % 8]]
    aid, typ, off = ei.inter_sessions(lengths, n_aids, seed=4)
    rng = np.random.default_rng(5)
    cand = np.full((S, C), -1, dtype=np.int32)
    score = ei.inter_scores('fractional', (S, C), rng)
    n_stale = 0
    for s in range(S):
        prev = s - 16_384 if s >= 16_384 else s           # the session the same wave held before (second half), or itself
        src = aid[off[prev]:off[prev + 1]]
        own = aid[off[s]:off[s + 1]]
        # what the previous session left in LDS between n and the end of the last 4-wide read of this one
        stale = np.setdiff1d(src[len(own):(len(own) + 3) // 4 * 4], own) if s >= 16_384 else np.zeros(0, dtype=np.int32)
        pick = np.unique(np.r_[7, stale, own[:2]])[:C]      # aid 7 is a candidate of every session
        cand[s, :len(pick)] = pick
        n_stale += len(stale)
    assert n_stale > 1000
    assert (lengths[:16_384][:S - 16_384] > lengths[16_384:]).sum() > 1000
    got, sf, af = _dense(gpu_device, aid, typ, off, cand, score, n_aids)
    assert (cand == 7).sum() == S and (got['session_candidate_occurrence_count'] == 0).sum() > 3000


def test_csr_rows_of_0_1_64_65_129_and_600_candidates(gpu_device):
    """The CSR form (the ranker's table): rows of 0, 1, 64, 65, 129 candidates and of 600 (a 500-event session's 500 distinct
    aids followed by 100 others), mixed-sign fractional scores."""
    import pandas as pd
    import torch
    from otto_amd.ranker import interaction_feature_engineering as ife
    n_aids = 2000
    rng = np.random.default_rng(11)
    sizes = [0, 1, 64, 65, 129, 600, 0, 600, 1, 129]
    lengths = [5, 1, 40, 70, 200, 500, 3, 500, 512, 100]
    aid, typ, off = ei.inter_sessions(lengths, n_aids, seed=12)
    cands = []
    for s, n in enumerate(sizes):
        if n == 600:
            aid[off[s]:off[s + 1]] = rng.permutation(n_aids)[:500]          # 500 distinct own aids
            own = aid[off[s]:off[s + 1]]
            cands.append(np.r_[own[::-1], rng.permutation(np.setdiff1d(np.arange(n_aids), own))[:100]].astype(np.int32))
        else:
            cands.append(ei.unique_candidates(rng, aid[off[s]:off[s + 1]], n_aids, n))
    row_off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    cand = np.concatenate(cands).astype(np.int32)
    score = ei.inter_scores('mixed', len(cand), rng)
    s_idx = np.repeat(np.arange(len(sizes)), sizes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    tab = {'candidates': t(cand), 'candidate_scores': t(score), 'row_off': t(row_off), 'session': t(s_idx.astype(np.int64))}
    row, sf, af = ife.interaction_features_rows(t(aid), t(typ), t(off), tab, n_aids)
    got = ife.table_to_frame(tab, row, sf, af)
    want = io.interaction_features(pd.DataFrame({'session': s_idx.astype(np.int64), 'candidates': cand.astype(np.int64),
                                                 'candidate_scores': score.astype(np.float64)}), ei.events_frame(aid, typ, off))
    got = _compare(got, want, ife)
    assert np.isnan(sf.cpu().numpy()[0]).all() and np.isnan(sf.cpu().numpy()[1][1])     # no rows: all null; one row: std null
    assert (got['session_candidate_occurrence_count'] > 0).sum() >= 1000


def test_too_long_session_and_out_of_range_candidate_are_errors(gpu_device):
    import torch
    from otto_amd import _lib
    from otto_amd.ranker import interaction_feature_engineering as ife
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    n_aids = 50
    aid, typ, off = ei.inter_sessions([4, 513, 2], n_aids, seed=1)
    cand = np.array([[1, 2], [3, -1], [4, 5]], dtype=np.int32)
    score = np.ones((3, 2), dtype=np.float32)
    with pytest.raises(_lib.OttoError, match='1 sessions longer than 512 events or candidates outside'):
        ife.interaction_features(t(aid), t(typ), t(off), t(cand), t(score), n_aids)
    aid, typ, off = ei.inter_sessions([4, 512, 2], n_aids, seed=1)
    ife.interaction_features(t(aid), t(typ), t(off), t(cand), t(score), n_aids)            # 512 is the limit, not beyond it
    cand[2, 1] = n_aids
    with pytest.raises(_lib.OttoError, match='1 sessions longer than 512 events or candidates outside'):
        ife.interaction_features(t(aid), t(typ), t(off), t(cand), t(score), n_aids)


VARIANCE_CASES = {
    # name: (base, step count, step, rows per aid, inside the candidate generators' range)
    'offset_1000_fractional': (1000.0, 1024, 2.0 ** -10, 4000, False),
    'counts_near_65535': (65_534.0, 2, 1.0, 5000, True),
    'recency_weights_near_4': (4.0 - 2.0 ** -6, 17, 2.0 ** -10, 5000, True),
}


@pytest.mark.parametrize('name', sorted(VARIANCE_CASES))
def test_variance_of_large_mean_small_spread_scores(gpu_device, name, capsys):
    """MEASUREMENT, outside the capped set of ``test_edge_cases_cpu``: the one-pass variance (sum_sq - n mean^2, float64)
    on scores of large mean and small spread, thousands of rows per aid and 100 per session. Prints the observed relative
    error of the aid and session std columns. Scores 1000 + multiples of 2^-10 are outside what the candidate generators
    produce (integer counts up to 65,535, recency weights in (0, 4]) and are only measured; the two cases inside that
    range must meet the project's 1e-5.

    Measured on an MI355X (max relative error of std, aid / session columns):
        plain one-pass sums     offset_1000_fractional 5.1e-08 / 5.9e-08   recency_weights_near_4 4.8e-08 / 5.6e-08
                                counts_near_65535      3.6e-04 / 6.7e-06   (aid column beyond 1e-5: the bug)
        shifted sums (now)      counts_near_65535      3.3e-08 / 1.5e-08   the other two unchanged"""
    base, steps, step, rows, in_range = VARIANCE_CASES[name]
    C, n_aids = 100, 100
    rng = np.random.default_rng(3)
    S = rows
    aid, typ, off = ei.inter_sessions(np.full(S, 2), n_aids, seed=2)
    cand = np.tile(np.arange(C, dtype=np.int32), (S, 1))
    score = (base + rng.integers(0, steps, (S, C)) * step).astype(np.float32)
    if name == 'counts_near_65535':                       # one row of every aid one count lower: the smallest spread there is
        score[:] = 65_535.0
        score[rng.integers(0, S, C), np.arange(C)] = 65_534.0
    import torch
    from otto_amd.ranker import interaction_feature_engineering as ife
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    _, sf, af = ife.interaction_features(t(aid), t(typ), t(off), t(cand), t(score), n_aids)
    s64 = score.astype(np.float64)
    want_aid, want_sess = s64.std(axis=0, ddof=1), s64.std(axis=1, ddof=1)
    ok = want_sess > 0
    err_aid = np.abs(af.cpu().numpy()[:, 1].astype(np.float64) - want_aid) / want_aid
    err_sess = np.abs(sf.cpu().numpy()[:, 1].astype(np.float64)[ok] - want_sess[ok]) / want_sess[ok]
    with capsys.disabled():
        print(f'\nvariance measurement {name}: aid std rel err max {err_aid.max():.3e}, session std rel err max {err_sess.max():.3e}')
    assert np.isfinite(err_aid).all() and np.isfinite(err_sess).all()
    if in_range:
        assert err_aid.max() <= 1e-5 and err_sess.max() <= 1e-5, (err_aid.max(), err_sess.max())
