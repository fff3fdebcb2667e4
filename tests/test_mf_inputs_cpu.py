"""Every builder of ``tests/mf_inputs.py`` has the property its name claims, for every case tests/test_mf_edges_gpu.py uses
(no GPU needed). If a batch lost its edge -- a duplicate too few, a sample inside the threshold band, a gradient row that
cancels, a prefix shorter than a wave -- the GPU tests would still pass and prove nothing."""
import numpy as np
import pytest

import edge_inputs as ei
import mf_inputs as mi
import mf_oracle as mo


def test_batch_sizes_follow_the_block_geometry():
    for d in mi.D_ALL:
        g = 1024 // d
        want = [1, g - 1, g, g + 1, 3 * g + 2] + ([2048 * g + 1] if d in (64, 128, 256) else [])
        assert mi.batch_sizes(d) == want and len(set(want)) == len(want) and min(want) == 1
        assert max(want) <= 32769
    assert [mi.two_trip(d) for d in (64, 128, 256)] == [32769, 16385, 8193]
    assert all(mi.two_trip(d) is None and 2048 * mi.gpb(d) + 1 > 32769 for d in (4, 8, 16, 32))


def _mf_grid(B, G):
    # static int mf_grid(int64_t B, int G) of csrc/otto_mf.hip, restated line by line
    gpb = 256 // G
    g = (B + gpb - 1) // gpb
    cap = 256 * 8
    return 1 if g < 1 else (cap if g > cap else g)


@pytest.mark.parametrize('d', [64, 128, 256])
def test_two_trip_size_gives_block_zero_a_second_partly_filled_trip(d):
    G, B = d // 4, mi.two_trip(d)
    assert all(mi.mf_grid(n, d) == _mf_grid(n, G) for n in (1, mi.gpb(d), mi.gpb(d) + 1, B - 1, B, 2 * B, 3 * B))
    assert _mf_grid(B, G) == 2048 and _mf_grid(B - 1, G) == 2048
    t = mi.trips(B, d)
    assert t.shape == (2048, 256 // G) and t.sum() == B
    assert t[0, 0] == 2 and (t.ravel()[1:] == 1).all()          # block 0 group 0 loops twice, every other group once
    assert (mi.trips(B - 1, d) == 1).all()                      # one sample fewer: a single full trip
    # the kernel's own loop, walked for block 0
    gpb, grid = 256 // G, 2048
    for group in range(gpb):
        b, n = 0 * gpb + group, 0
        while b < B:
            n += 1
            b += grid * gpb
        assert n == t[0, group]
    groups_per_wave = 64 // G
    if d == 128:       # the last live wave of the second trip: group 0 live, group 1 (same wave) has left the loop
        assert groups_per_wave == 2 and t[0, 0] == 2 and t[0, 1] == 1
    if d == 256:
        assert groups_per_wave == 1
    if d == 64:
        assert groups_per_wave == 4 and t[0, :4].tolist() == [2, 1, 1, 1]


def _hist(i1, i2, n1, n2, shared):
    if shared:
        return [np.bincount(np.r_[i1, i2], minlength=n1)]
    return [np.bincount(i1, minlength=n1), np.bincount(i2, minlength=n2)]


def _check_structure(dup, B, shared, n1, n2, i1, i2):
    assert len(i1) == len(i2) == B and i1.dtype == i2.dtype == np.int64
    assert i1.min() >= 0 and i2.min() >= 0 and i1.max() < n1 and i2.max() < n2 and (not shared or n1 == n2)
    hs = _hist(i1, i2, n1, n2, shared)
    if dup == 'none':
        assert all(h.max() == 1 for h in hs) and n1 >= B and n2 >= B
    elif dup == 'pairs':
        for h in hs:
            occ = np.sort(h[h > 0])
            odd = 0 if shared else B % 2
            assert (occ[:len(occ) - odd] == 2).all() and (occ[len(occ) - odd:] == 3).all() and len(occ) >= 1
    elif dup == 'one_row':
        assert len(set(zip(i1.tolist(), i2.tolist()))) == 1 and i1[0] != i2[0]
        assert sorted(np.concatenate([h[h > 0] for h in hs]).tolist()) == [B, B]
        assert all((h == 0).sum() >= 3 for h in hs)               # rows outside the batch exist
    elif dup == 'zipf':
        assert (n1, n2) == ((97, 97) if shared else (97, 53))
        if B >= 64:
            assert all(h.max() >= B // 8 for h in hs), 'no heavy row'
    elif dup == 'self':
        assert shared and n1 == 97
        same = np.flatnonzero(i1 == i2)
        assert len(same) >= min(B, 8)
        assert any(hs[0][i1[b]] == 2 for b in same), 'no self sample whose row occurs nowhere else'
        if B > 8:
            assert any(hs[0][i1[b]] > 2 for b in same), 'no self sample on a row that others use too'


@pytest.mark.parametrize('d', mi.D_ALL)
def test_step_cases_have_their_duplicate_structure_and_no_near_cancelled_row(d):
    worst = np.inf
    for B in mi.batch_sizes(d):
        for dup in mi.DUPS:
            for shared in (False, True):
                if (dup == 'self' and not shared) or (dup == 'pairs' and B < 2 and not shared):
                    continue
                for kind in mi.KINDS if B <= 3 * mi.gpb(d) + 2 else mi.KINDS[:1]:
                    rng = np.random.default_rng([d, B, mi.DUPS.index(dup), int(shared)])
                    n1, n2, E1, E2, i1, i2, tg = mi.step_case(d, B, dup, shared, rng, kind)
                    _check_structure(dup, B, shared, n1, n2, i1, i2)
                    assert E1.shape == (n1, d) and E2.shape == (n2, d) and E1.dtype == np.float32 and (E2 is E1) == shared
                    assert 0.2 < E1.std() < 0.4 or n1 * d < 64
                    assert set(np.unique(tg)) <= ({0, 1, 2} if kind == 'MSELoss' else {0, 1})
                    r = mi.smallest_row_ratio(E1, E2, i1, i2, tg, kind, shared)
                    assert r >= mi.NEAR_CANCELLED, (B, dup, shared, kind, r)
                    assert mi.loss_condition(E1, E2, i1, i2, tg, kind) <= mi.LOSS_CONDITION
                    assert max(E1.nbytes, E2.nbytes) <= 64 << 20
                    worst = min(worst, r)
    print(f'd={d}: smallest gradient row ratio {worst:.3g}')


def _check_sequence(s, plan):
    assert len(s.steps) == len(s.want) == len(plan)
    for k, ((B, dup), (i1, i2, tg), (E1, E2)) in enumerate(zip(plan, s.steps, s.before)):
        _check_structure(dup, B, s.shared, s.n1, s.n2, i1, i2)
        assert mi.smallest_row_ratio(E1, E2, i1, i2, tg, s.kind, s.shared) >= mi.NEAR_CANCELLED
        assert mi.loss_condition(E1, E2, i1, i2, tg, s.kind) <= mi.LOSS_CONDITION
        after = s.want[k]
        assert mi.loss_condition(after[1], after[4], i1, i2, tg, s.kind) <= mi.LOSS_CONDITION     # eval of the same ids
        assert np.isfinite(after[0]) and all(np.isfinite(x).all() for x in after[1:])
        assert (after[4] is after[1]) == s.shared
    assert np.array_equal(s.before[0][0], s.E1) and (s.E2 is s.E1) == s.shared


def test_every_gpu_step_sequence_is_well_conditioned_at_every_step():
    for d, kind, shared, dup in mi.MATRIX_CASES:
        plan = mi.matrix_plan(d, dup)
        assert plan[2][0] < plan[0][0] and plan[2][0] == mi.gpb(d) + 1     # the third step is smaller than max_batch
        _check_sequence(mi.matrix_seq(d, kind, shared, dup), plan)
    for d, B, dup in mi.EDGE_CASES:
        _check_sequence(mi.edge_seq(d, B, dup), ((B, dup),))
    for d, B in mi.IDENTICAL_CASES:                     # run twice and compared with each other: the structure is what counts
        s = mi.edge_seq(d, B, 'none')
        _check_structure('none', B, False, s.n1, s.n2, *s.steps[0][:2])
    for dup, d, shared in mi.DUP_CASES:
        _check_sequence(mi.dup_seq(dup, d, shared), ((mi.gpb(d) + 1, dup),) * 2)
    assert {c[0] for c in mi.MATRIX_CASES} == set(mi.D_ALL) and len(mi.MATRIX_CASES) == 7 * 2 * 3
    assert {(d, B) for d, B, dup in mi.EDGE_CASES if dup == 'zipf'} == {(d, B) for d in mi.D_ALL for B in mi.batch_sizes(d)}


@pytest.mark.parametrize('d,kind,shared', mi.SUMS_CASES)
def test_no_validation_sample_lies_inside_the_threshold_band(d, kind, shared):
    s = mi.sums_case(d, kind, shared)
    assert [len(b[0]) for b in s.batches[:3]] == [1, mi.gpb(d) + 1, mi.two_trip(d) or 3 * mi.gpb(d) + 2]
    assert (s.E2 is s.E1) == shared
    for i1, i2, tg in s.batches:
        dist, band = mi.threshold_margin(s.E1, s.E2, i1, i2, kind)
        assert (dist > band).all() and (band > 0).all()
        # the band is the project's dot-product bound (edge_inputs.dot_bound), at the kernel's threshold
        thr = 0.5 if kind == 'MSELoss' else 0.0
        if len(i1) <= 300:
            S, bound = ei.dot_bound(s.E1[i1], s.E2[i2])
            np.testing.assert_allclose(dist, np.abs(np.diag(S) - thr), rtol=0, atol=1e-14)
            assert (band >= np.diag(bound) * (1 - 1e-12)).all()
        assert mi.loss_condition(s.E1, s.E2, i1, i2, tg, kind) <= mi.LOSS_CONDITION
        # so a float32 forward in any order decides every hit as float64 does
        o32 = mo.forward(s.E1, s.E2, i1, i2)
        o64 = (s.E1[i1].astype(np.float64) * s.E2[i2].astype(np.float64)).sum(1)
        assert np.array_equal(o32 >= thr, o64 >= thr)
        hits = mo.eval_sums(s.E1, s.E2, i1, i2, tg, kind)[2]
        assert 0 <= hits <= len(i1) and (len(i1) < 100 or 0 < hits < len(i1))


def test_sampler_fallback_rows_are_pinned():
    found = mi.bpr_fallback_rows(1, 0, 20000)
    assert found == [(6543, 1), (13119, 1), (18167, 1)] and tuple(r for r, _ in found) == mi.FALLBACK_ROWS
    for row, v in found:
        assert mo.bpr_negative(1, 0, row, 1, 2) == 0                       # the fallback (1 + 1) % 2
        assert mo.bpr_negative(1, 0, row, 1, 2, attempts=True) == (0, 16)
        assert mo.bpr_negative(1, 0, row, 0, 2) == 1
        assert mo.bpr_negative(1, 0, row, 0, 2, attempts=True) == (1, 0)
    # the GPU test's window: row0 = 6543 - 100, 256 rows, positives all 1: exactly one row falls back
    used = [mo.bpr_negative(1, 0, 6443 + b, 1, 2, attempts=True)[1] for b in range(256)]
    assert used[100] == 16 and sorted(used)[-2] < 16


def test_last_attempt_row_is_accepted_on_the_sixteenth_draw():
    row, pos, neg = mi.LAST_ATTEMPT
    assert mo.bpr_negative(1, 0, row, pos, 3, attempts=True) == (neg, 15)
    assert neg != pos and neg != (pos + 1) % 3, 'giving up one attempt early must change the answer'


@pytest.mark.parametrize('d', mi.D_ALL)
def test_race_free_prefix_is_longer_than_a_wave_of_groups(d):
    U, V, u, i, j = mi.race_free_triplets(d, 1, mi.race_rng())
    keep = len(u)
    assert keep >= 65 and len(i) == len(j) == keep
    assert len(set(u.tolist())) == keep and len(set(i.tolist()) | set(j.tolist())) == 2 * keep
    assert np.array_equal(j, mo.bpr_negatives(1, 0, 0, i, V.shape[0]))
    assert max(U.nbytes, V.nbytes) <= 64 << 20 and U.shape[1] == V.shape[1] == d


def test_bpr_batch_cases_cover_every_factor_size():
    assert {d for d, _ in mi.BPR_BATCH_CASES} == set(mi.D_ALL)
    assert {B for d, B in mi.BPR_BATCH_CASES if d == 64} == {1, 17, 32769}
    for d, B in mi.BPR_BATCH_CASES:
        U, V, u, i = mi.bpr_case(d, B, np.random.default_rng([5, d, B]))
        assert u.max() < U.shape[0] and i.max() < V.shape[0] and len(u) == len(i) == B
        if B > 1000:
            assert np.bincount(i).max() > B // 8
