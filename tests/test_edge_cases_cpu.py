"""The generators of ``tests/edge_inputs.py`` hold what their names claim (no GPU needed). The edge-shape GPU tests
(test_events_sort_gpu, test_pairs_gpu, test_inter_gpu, test_score_gpu) compare kernels with references on these inputs; if
an input lost its edge, those tests would still pass and prove nothing. Also here: the float64 one-pass variance cap that
picks the score distributions of test_inter_gpu, and the dot-product bound of test_score_gpu on a NumPy float32 product."""
import numpy as np
import pytest

import edge_inputs as ei
import mf_oracle as mo
import pairs_oracle as po

BIG = ei.SORT_PATTERN_SIZES[1]


# ---- 1. sort inputs ---------------------------------------------------------------------------------------------------

def test_sort_sizes_sit_on_and_next_to_every_unit_of_the_kernel():
    s = set(ei.SORT_SIZES)
    for unit in (ei.WAVE, ei.BLOCK, 1024, ei.TILE, ei.SPAN):
        assert {unit - 1, unit, unit + 1} <= s
    assert {1, 2, 3 * ei.SPAN + 1, 65536 + 17} <= s
    assert ei.SORT_PATTERN_SIZES[0] < ei.TILE and ei.SORT_PATTERN_SIZES[1] > 4 * ei.SPAN


@pytest.mark.parametrize('pattern,bytes_', [('all_equal', []), ('bit0', [0]), ('bit30', [3]), ('bit63', [7]), ('bytes05', [0, 5]),
                                            ('tile_one_digit', [0, 1])])
@pytest.mark.parametrize('n', ei.SORT_PATTERN_SIZES)
def test_sort_patterns_vary_exactly_the_bytes_they_name(pattern, bytes_, n):
    sess, ts, div = ei.sort_case(pattern, n)
    var = ei.key_bytes_varying(sess, ts, div)
    assert np.flatnonzero(var).tolist() == bytes_
    key = (sess.astype(np.uint64) << np.uint64(32)) | (ts // div).astype(np.uint64)
    if pattern.startswith('bit'):
        bit = int(pattern[3:])
        x = int(np.bitwise_or.reduce(key) ^ np.bitwise_and.reduce(key))
        assert x == 1 << bit and len(np.unique(key)) == 2


def test_sort_patterns_hold_the_ties_ranges_and_orders_they_name():
    for n in ei.SORT_PATTERN_SIZES:
        sess, ts, div = ei.sort_case('ties3', n)
        assert len(np.unique(sess.astype(np.int64) * (1 << 32) + ts)) == 3
        sess, ts, div = ei.sort_case('high_sessions', n)
        assert sess.dtype == np.uint32 and sess.max() == 2 ** 32 - 1 and (sess >= 2 ** 31).sum() > n // 4 and (sess < 50).sum() > n // 4
        sess, ts, div = ei.sort_case('ts_extremes', n)
        assert ts.min() == 0 and ts.max() == 2 ** 31 - 1 and div == 1
        for pattern, sign in (('descending', -1), ('sorted', 1)):
            sess, ts, div = ei.sort_case(pattern, n)
            key = sess.astype(np.int64) * (1 << 32) + ts
            assert (np.diff(key) * sign > 0).all()
            order = ei.sort_reference(sess, ts, div)[0]
            assert np.array_equal(order, np.arange(n) if sign > 0 else np.arange(n)[::-1])
        # millisecond remainders: sorting by the raw stamps would order ties differently from sorting by seconds
        sess, ts, div = ei.sort_case('ms_remainders', n)
        assert div == 1000 and not np.array_equal(np.lexsort((ts, sess)), np.lexsort((ts // div, sess)))
        sess, ts, div = ei.sort_case('generic', n)
        assert div == 1000 and (ts % 1000 != 0).any() and ei.key_bytes_varying(sess, ts, div)[[0, 1, 4]].all()
        assert ei.sort_case('seconds_div1', n)[2] == 1


def test_tile_one_digit_fills_one_digit_per_tile_in_pass_zero():
    sess, ts, div = ei.sort_case('tile_one_digit', BIG)
    b0 = (ts & 255)[:BIG // ei.TILE * ei.TILE].reshape(-1, ei.TILE)
    assert (b0 == b0[:, :1]).all() and len(np.unique(b0[:, 0])) == BIG // ei.TILE      # 1024 per wave, positions to 4095
    sess, ts, div = ei.sort_case('tile_one_digit', ei.SORT_PATTERN_SIZES[0])
    assert len(np.unique((ts & 255)[:-1])) == 1 and (ts[-1] & 255) != (ts[0] & 255)


def test_sort_reference_is_the_stable_order_with_its_csr():
    sess = np.array([9, 5, 9, 5, 5], dtype=np.uint32)
    ts = np.array([1999, 2000, 1000, 2999, 1000], dtype=np.int64)
    order, sec, ids, off = ei.sort_reference(sess, ts, 1000)
    assert order.tolist() == [4, 1, 3, 0, 2] and sec.tolist() == [1, 2, 2, 1, 1] and ids.tolist() == [5, 9] and off.tolist() == [0, 3, 5]
    order, sec, ids, off = ei.sort_reference(sess[:0], ts[:0], 1)
    assert len(order) == 0 and off.tolist() == [0]


# ---- 2. pair inputs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hours', [1, 24, 0.5])
def test_time_edge_stream_holds_its_edges_in_the_oracles_output(hours):
    max_dt = int(round(hours * 3600))
    sessions = ei.time_edge_sessions(max_dt)
    aid, ts, off, fr = ei.stream_to_frame(sessions)
    n = np.diff(off)
    assert n[0] == 0 and n[-1] == 0 and n[2] == 0 and n[4] == 0 and n[5] == 0 and (n == 0).sum() == 5
    assert {1, 2, 3, 64, 65, 300} <= set(n.tolist()) and len(fr) == off[-1] and fr['session'].nunique() == (n > 0).sum()
    for s, (a, t) in enumerate(sessions):                       # rows are mapped by position
        assert sorted(aid[off[s]:off[s + 1]].tolist()) == sorted(np.asarray(a, dtype=np.int64).tolist())
        assert (np.diff(ts[off[s]:off[s + 1]]) >= 0).all()
    mean = {(r.x1, r.x2): r.target for r in po.pairs_time(fr, hour_difference=hours, target_aggregation='mean').itertuples()}
    mx = {(r.x1, r.x2): r.target for r in po.pairs_time(fr, hour_difference=hours, target_aggregation='max').itertuples()}
    each = lambda q: (ei.AID_DT_EACH + 2 * q, ei.AID_DT_EACH + 2 * q + 1)
    want = [1, 0, 0, 0, int(86_400 <= max_dt), 0]               # dt = max_dt, max_dt + 1, 0, -1, 86400, 90000
    assert [mean[each(q)] for q in range(6)] == want and [mx[each(q)] for q in range(6)] == want
    assert mx[each(3)[::-1]] == 1                                # dt = -1 seen from the other aid is +1
    assert mx[ei.AID_DT_SHARED] == 1 and mean[ei.AID_DT_SHARED] == 0
    assert mean[ei.AID_HALF] == 1 and mean[ei.AID_BELOW_HALF] == 0 and mx[ei.AID_BELOW_HALF] == 1
    assert mean[(0, ei.MAX_AID)] == 1 and mean[(ei.MAX_AID, 0)] == 0
    assert (44, 44) not in mean and mean[(44, 45)] == 0          # equal aids dropped; equal stamps: dt = 0


def test_time_size_case_and_sampled_case_have_the_shape_they_claim():
    aid, ts, off, fr = ei.stream_to_frame(ei.random_sessions(**ei.TIME_BIG))
    raw = ei.raw_time_slots(off)
    assert raw > 2 ** 22 and raw // ei.SPAN > 250 and np.diff(off).max() == 60 and len(off) - 1 == 40_000
    a = aid.astype(np.int64)
    assert sum(int((np.bincount(a[off[s]:off[s + 1]]) ** 2).sum()) - int(off[s + 1] - off[s]) for s in range(2000)) > 0   # PAIR_NONE slots
    # a 15 % sample of short sessions leaves sessions empty
    aid, ts, off, fr = ei.stream_to_frame(ei.random_sessions(3000, 400, 40, 0.15, seed=5))
    keep = np.random.default_rng(0).random(len(aid)) < 0.15
    assert (np.add.reduceat(np.r_[keep, False].astype(np.int64), off[:-1]) == 0).sum() > 300


def test_diff_edge_stream_holds_its_edges():
    sessions, keys = ei.diff_edge_stream()
    aid, ts, off, fr = ei.stream_to_frame(sessions)
    assert len(keys) == len(aid) and {1, 2, 3} <= set(np.diff(off).tolist()) and keys.min() == 0 and keys.max() == 2 ** 31 - 1
    s = fr['session'].to_numpy()
    x1 = aid.astype(np.int64)
    x3 = x1[np.lexsort((keys, s))]
    has_next = np.r_[s[1:] == s[:-1], False]
    x2 = np.r_[x1[1:], -1]
    assert (has_next & (x2 == x3)).any() and (has_next & (x1 == x3) & (x1 != x2)).any()
    pos = set(zip(x1[has_next & (x2 != x3) & (x1 != x2) & (x1 != x3)].tolist(), x2[has_next & (x2 != x3) & (x1 != x2) & (x1 != x3)].tolist()))
    neg = set(zip(x1[has_next & (x2 != x3) & (x1 != x3)].tolist(), x3[has_next & (x2 != x3) & (x1 != x3)].tolist()))
    assert (10, 11) in pos and (10, 11) in neg
    out = po.pairs_diff(fr, shuffle_keys=keys)
    rows = ei.pair_rows([out['x1'].to_numpy(), out['x2'].to_numpy(), out['target'].to_numpy()]).tolist()
    assert [10, 11, 1] in rows and [10, 11, 0] not in rows and not any(r[0] == 33 for r in rows)
    assert len(po.pairs_diff(fr, shuffle_keys=np.full(len(aid), 9))) == 0          # identity permutation: x3 == x1 everywhere


# ---- 3. interaction feature inputs ------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ei.SCORE_KINDS)
def test_one_pass_variance_cap_admits_the_score_distributions_in_use(kind):
    """The kernels' variance formula, evaluated in float64 NumPy over several summation orders, stays within 1e-6 relative of
    the two-pass float64 std for every score distribution test_inter_gpu compares at 1e-5 -- at 2, 100 and 20,000 rows."""
    rng = np.random.default_rng(1)
    for n in (2, 100, 20_000):
        x = ei.inter_scores(kind, n, rng)
        if np.std(x.astype(np.float64)) == 0:
            continue
        assert ei.one_pass_error(x) <= 1e-6, (kind, n)
        assert (x.astype(np.float64) * 1024 == np.round(x.astype(np.float64) * 1024)).all()       # multiples of 2^-10: exact sums
    x = ei.inter_scores(kind, 1000, rng)
    assert {'fractional': x.min() > 0 and x.max() <= 4, 'negative': x.max() < 0, 'mixed': x.min() < 0 < x.max(),
            'counts': (x == np.round(x)).all()}[kind]


def test_one_pass_variance_cap_rejects_large_mean_small_spread():
    """... and the emulation does see the cancellation: scores of large mean and small spread fall outside the cap, so they
    are measured in test_inter_gpu rather than used for the 1e-5 comparisons."""
    x = np.full(5000, 65_535.0)
    x[17] = 65_534.0
    assert ei.one_pass_error(x) > 1e-5
    rng = np.random.default_rng(2)
    assert ei.one_pass_error(1.0e6 + rng.integers(0, 1024, 4000) / 1024.0) > 1e-6


def test_inter_long_cycle_ends_on_the_lds_buffer():
    assert ei.INTER_LONG_CYCLE[-4:] == (509, 510, 511, 512) and {1, 3, 4, 5} <= set(ei.INTER_LONG_CYCLE)
    rng = np.random.default_rng(0)
    own = np.array([5, 5, 9, 11])
    c = ei.unique_candidates(rng, own, 50, 30)
    assert len(np.unique(c)) == 30 and np.isin(c, own).any() and (~np.isin(c, own)).any()


# ---- 4. scoring inputs ------------------------------------------------------------------------------------------------

def test_score_split_restates_the_kernels_split():
    assert ei.score_split(1, 1) == (1, 32) and ei.score_split(300, 1024) == (1, 1024)
    assert ei.score_split(300, 1025) == (2, 544) and ei.score_split(1, 40_000) == (40, 1024)
    assert ei.score_split(4096, 1_855_604) == (32, 58_016)        # 32 row tiles: 32 splits of 1813 item tiles


def test_score_cases_cover_every_pair_and_every_pad_sits_where_it_says():
    cases = ei.score_cases()
    assert cases == ei.score_cases() and len(cases) < 200
    have = set()
    for c in cases:
        have |= {(i, c[i], j, c[j]) for i in range(5) for j in range(i + 1, 5)}
    axes = (ei.SCORE_D, ei.SCORE_K, ei.SCORE_B, ei.SCORE_N, ei.SCORE_PAD)
    for i in range(5):
        for j in range(i + 1, 5):
            for a in axes[i]:
                for b in axes[j]:
                    if i == 3 and a <= 1024 and b == 'split':
                        continue                                  # one split only: no boundary to sit on
                    assert (i, a, j, b) in have, (i, a, j, b)
    for d in ei.SCORE_D:
        assert {k for dd, k, *_ in cases if dd == d} == set(ei.SCORE_K)
        assert any(dd == d and N > 1024 for dd, _, _, N, _ in cases)
        assert any(dd == d and p == 'split' for dd, *_, p in cases)
    for N in (1025, 2049, 40_000):
        assert (3, N, 4, 'split') in have
    for d, k, B, N, kind in cases:
        pad = ei.pad_col_of(kind, B, N)
        ns, per = ei.score_split(B, N)
        assert per % 32 == 0 and (ns - 1) * per < N <= ns * per
        if kind == 'none':
            assert pad == -1
        elif kind == 'first':
            assert pad == 0
        elif kind == 'last':
            assert pad == N - 1
        elif kind == 'split':
            assert ns > 1 and pad == per and pad % per == 0 and 0 < pad < N
        else:
            assert 0 <= pad < N and (N < 64 or (pad % 32 not in (0, 31) and 32 <= pad < N - 32))
    for kind in ei.SCORE_PAD:
        assert ei.pad_col_of('split', 8, 1024) is None


def test_exact_inputs_are_exact_in_fp32_and_tie_at_the_kth_place():
    for d in ei.SCORE_D:
        U, V = ei.exact_inputs(64, 2049, d, seed=1)
        assert U.dtype == np.float32 and (U == np.round(U)).all() and np.abs(U).max() == 4 and np.abs(V).max() == 4
        assert (np.abs(U.astype(np.float64)) @ np.abs(V.astype(np.float64)).T).max() < 2 ** 24
        S = U.astype(np.float64) @ V.astype(np.float64).T
        # fp32 in two different summation orders gives the float64 result
        assert np.array_equal((U @ V.T).astype(np.float64), S) and np.array_equal((U[:, ::-1] @ V[:, ::-1].T).astype(np.float64), S)
        for k in (1, 20, 32):
            srt = -np.sort(-S, axis=1)
            tied = srt[:, k - 1] == srt[:, k]
            assert tied.mean() > 0.5, (d, k, tied.mean())


def test_dot_bound_holds_for_a_numpy_float32_product():
    for d in ei.SCORE_D:
        U, V = ei.float_inputs(33, 1025, d, seed=3)
        S64, bound = ei.dot_bound(U, V)
        err = np.abs((U @ V.T).astype(np.float64) - S64)
        assert (err <= bound).all() and (bound > 0).all()
        naive = np.zeros((33, 1025), dtype=np.float32)              # strictly sequential fp32 accumulation
        for i in range(d):
            naive += U[:, i:i + 1] * V[:, i][None, :]
        assert (np.abs(naive.astype(np.float64) - S64) <= bound).all()
        assert np.median(bound / np.maximum(np.abs(S64), 1e-30)) < 1e-3


def test_topk_padded_and_merge_reference():
    U, V = ei.exact_inputs(3, 5, 8, seed=0)
    ids, sc = ei.topk_padded(mo.score_topk, U, V, 8, 2)
    wi, ws = mo.score_topk(U, V, k=5, pad_col=2)
    assert np.array_equal(ids[:, :4], wi[:, :4]) and (ids[:, 4:] == -1).all() and np.isneginf(sc[:, 4:]).all()
    ids, sc = ei.topk_padded(mo.score_topk, U, V, 3, -1)           # N >= k: the oracle's own output
    wi, ws = mo.score_topk(U, V, k=3)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    for n_lists in (1, 2, 5):
        ps, pi = ei.merge_lists(n_lists, 130, 20, seed=4)
        empty = (pi == -1) | (pi == 0x7FFFFFFF)
        assert np.isneginf(ps[empty]).all() and np.isfinite(ps[~empty]).all() and empty.any()
        if n_lists > 1:
            assert (pi == -1).any() and (pi == 0x7FFFFFFF).any()
            ties = sum(len(np.intersect1d(ps[0, b][~empty[0, b]], ps[1, b][~empty[1, b]])) > 0 for b in range(130))
            assert ties > 50                                       # equal scores, different ids, across lists
        for b in range(130):
            i = pi[:, b][~empty[:, b]]
            assert len(np.unique(i)) == len(i)
        wi, ws = ei.merge_reference(ps, pi, 20)
        assert (wi[np.isneginf(ws)] == -1).all() and (ws[:, 1:] <= ws[:, :-1]).all()
        assert ((wi == -1).sum(axis=1) > 0).any()
