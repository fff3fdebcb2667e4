"""The inputs of tests/test_sgns_hogwild_gpu.py reach what they claim (tests/sgns_hogwild_inputs.py): the duplicate patterns,
the 64-pair chain, the race-free launch lengths; what a float32 run of the restatement leaves of the band (the noise
floor), and that each planted defect leaves the band by two orders of magnitude on the case aimed at it."""
import numpy as np
import pytest

import sgns_hogwild_inputs as hi
import sgns_hs_restatement as hr
import sgns_restatement as sr

LR = 0.05


@pytest.fixture(scope='module')
def tiny():
    return hi.tiny_vocab()


@pytest.fixture(scope='module')
def chain():
    return hi.long_chain()


# ---------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------
def test_tiny_vocab_is_what_the_module_says(tiny):
    w = tiny['weight'].astype(np.int64)
    assert tiny['n_aids'] == 7 and np.diff(tiny['sess_off']).tolist() == [9, 3, 2] and tiny['ws'] == 3
    assert (w == 0).sum() == 1 and w.max() > 0.6 * w.sum() and (tiny['keep_q'] == hi.U32).all()
    assert any(tiny['aid'][e] == tiny['aid'][e + 1] for s in range(3) for e in range(tiny['sess_off'][s], tiny['sess_off'][s + 1] - 1))
    for p in tiny['plans']:
        assert len(p['tok_aid']) == 14                        # t = 0: every event is a token
        assert np.diff(p['pair_off']).max() >= 4              # ws = 3 reaches beyond one pair on each side


@pytest.mark.parametrize('neg', [n for n in hi.NEGS if n >= 3])
def test_tiny_vocab_shows_every_duplicate_pattern(tiny, neg):
    seen = set()
    for ep, p in enumerate(tiny['plans']):
        T = len(p['tok_aid'])
        ctx, negs = sr.negatives(p, tiny['cum'], tiny['seed'], ep, neg, 0, T, tiny['n_aids'])
        seen |= hi.duplicate_patterns(p, ctx, negs, 0, T)
    possible = hi.possible_patterns(neg)
    assert possible <= seen, possible - seen
    # what a short target list cannot show (possible_patterns says why) is shown by the long ones
    if neg >= 7:
        assert possible == set(hi.PATTERNS)
    assert {('four', 1, 2), ('four', 2, 3), 'three_in_a_four', 'negative_is_centre', 'context_is_centre'} <= possible
    assert ('across_fours' in possible) == (neg >= 4) and (('four', 0, 1) in possible) == (neg >= 5)


def test_long_chain_holds_a_centre_with_64_pairs(chain):
    p = chain['plan']
    assert len(p['tok_aid']) == hi.CHAIN_TOKENS >= 70 and chain['ws'] == 32 and chain['neg'] == 64 and chain['n_aids'] == 400
    npairs = np.diff(p['pair_off'])
    c0, c1, c2 = chain['centres']
    assert (c0, c1) == (0, len(npairs) - 1) and npairs[c2] == 64 and p['tok_left'][c2] == 32
    assert npairs[c0] >= 2 and npairs[c1] >= 2 and p['tok_left'][c0] == 0 and p['tok_left'][c1] == npairs[c1]


@pytest.mark.parametrize('neg', hi.WIDE_NEGS)
@pytest.mark.parametrize('d', hi.DIMS)
def test_wide_vocab_cut_is_race_free_and_long_enough(d, neg):
    w = hi.wide_vocab(d, neg)
    p, sp = w['plan'], w['sparse']
    T = len(p['tok_aid'])
    assert w['n_aids'] * d <= 1 << 24 and len(np.unique(w['aid'])) == T and (w['weight'] == w['weight'][0]).all()
    lens = np.diff(w['sess_off'])
    assert set(lens.tolist()) == set(range(2, 8))
    assert (np.add.reduceat(w['active'].astype(np.int64), w['sess_off'][:-1]) == 1).all()      # one centre per session
    kept = np.diff(sp['pair_off'])
    assert np.array_equal(kept[w['active']], np.diff(p['pair_off'])[w['active']]) and not kept[~w['active']].any()
    assert set(kept[w['active']].tolist()) == set(range(1, 7))
    cut = w['cut']
    assert cut[0][0] == 0 and cut[-1][1] == T and all(a[1] == b[0] for a, b in zip(cut, cut[1:]))
    need = 2 * hi.gpb(d) + 1
    assert need == {4: 129, 8: 129, 16: 129, 32: 65, 64: 33, 128: 17}[d]
    assert max(hi.active_in(sp, t0, t1) for t0, t1 in cut) >= need
    for i, (t0, t1) in enumerate(cut):
        rows_in, rows_out = [], []
        for c in range(t0, t1):
            lo, hi_ = int(sp['pair_off'][c]), int(sp['pair_off'][c + 1])
            if hi_ > lo:
                rows_in.append(int(sp['tok_aid'][c]))
                rows_out.append(set(w['ctx'][lo:hi_].tolist()) | set(w['negs'][lo:hi_].ravel().tolist()))
        assert len(set(rows_in)) == len(rows_in)
        assert sum(len(r) for r in rows_out) == len(set().union(*rows_out))              # pairwise disjoint
        if t1 < T:                                          # maximal: the next centre does collide
            lo, hi_ = int(sp['pair_off'][t1]), int(sp['pair_off'][t1 + 1])
            nxt = set(w['ctx'][lo:hi_].tolist()) | set(w['negs'][lo:hi_].ravel().tolist())
            assert (nxt & set().union(*rows_out)) or int(sp['tok_aid'][t1]) in rows_in
        if t1 - t0 >= 64:
            # one wave at d = 4 is 64 centres: they leave the pair loop at different times
            assert len(set(kept[t0:t0 + 64].tolist()) - {0}) >= 3, (i, t0)


@pytest.mark.parametrize('d', hi.PERM_DIMS)
def test_permutation_closed_form_equals_the_restatement(d):
    pm = hi.permutation(d)
    T = pm['T']
    assert T == {128: 16395, 16: 131139}[d] and T > hi.SG_GRID * hi.gpb(d) and len(np.unique(pm['aid'])) == T == pm['n_aids']
    n = 1000
    head = pm['sess_off'][:n // 2 + 1]
    want_plan = sr.plan(pm['aid'][:n], head, pm['keep_q'], pm['seed'], 0, 1)
    got_plan = hi.permutation_plan(pm, n)
    for k in want_plan:
        assert got_plan[k].dtype == want_plan[k].dtype and np.array_equal(got_plan[k], want_plan[k]), k
    full = hi.permutation_plan(pm)
    assert full['pair_off'][-1] == T - 1 and full['tok_off'][-1] == T and full['tok_off'][-2] == T - 1
    cum = sr.cum_table(pm['weight'])
    for step in (sr.step_sequential, sr.step_batch):
        In, Out = hi.tables(T, d, 1), hi.tables(T, d, 2)
        In_w, Out_w = In.copy(), Out.copy()
        loss, ctx = hi.permutation_step(pm, In, Out, hi.PERM_LR, n)
        want = step(want_plan, cum, In_w, Out_w, pm['seed'], 0, 0, hi.PERM_LR, 0, n)
        assert np.array_equal(ctx, sr.negatives(want_plan, cum, pm['seed'], 0, 0, 0, n, T)[0])
        assert abs(loss - want) <= 1e-12 * want
        # the same float64 expression per row up to the order of the dot's additions: the stored float32 may differ in
        # its last bit
        np.testing.assert_allclose(In, In_w, rtol=2.5e-7, atol=0)
        np.testing.assert_allclose(Out, Out_w, rtol=2.5e-7, atol=0)
        assert not np.array_equal(In_w, hi.tables(T, d, 1))


# ---------------------------------------------------------------------------
# noise floor: a float32 run of the restatement against the float64 run, through the band
# ---------------------------------------------------------------------------
def _tiny_run(tiny, d, neg, hs, dtype):
    """tiny_vocab over two epochs, the state after every centre (what the GPU test compares after every launch)"""
    In, Out = hi.tables(7, d, 1), hi.tables(7, d, 2)
    tree = hr.huffman(tiny['count'], 1) if hs else None
    Syn = hi.tables(tree['n_inner'], d, 3) if hs else None
    states = []
    for ep, p in enumerate(tiny['plans']):
        for c in range(len(p['tok_aid'])):
            if hs:
                loss = hr.step_sequential_hs(p, tiny['cum'], In, Out, Syn, tree, tiny['seed'], ep, neg, LR, c, c + 1, dtype=dtype)
            else:
                loss = sr.step_sequential(p, tiny['cum'], In, Out, tiny['seed'], ep, neg, LR, c, c + 1, dtype=dtype)
            states.append((In.copy(), Out.copy(), None if Syn is None else Syn.copy(), loss))
    return states


def _worst(a_states, b_states):
    worst = 0.0
    for a, b in zip(a_states, b_states):
        for x, y in zip(a[:3], b[:3]):
            if x is not None:
                worst = max(worst, hi.band_ratio(x, y))
        worst = max(worst, abs(a[3] - b[3]) / (hi.ATOL + hi.RTOL * abs(b[3])))
    return worst


NOISE_BOUND = 0.25


@pytest.mark.parametrize('hs', [False, True])
@pytest.mark.parametrize('d', hi.DIMS)
def test_noise_floor_of_tiny_vocab(tiny, d, hs):
    for neg in hi.NEGS:
        ratio = _worst(_tiny_run(tiny, d, neg, hs, np.float32), _tiny_run(tiny, d, neg, hs, np.float64))
        print(f'tiny_vocab d {d} neg {neg} hs {hs}: float32 run / band = {ratio:.3f}')
        assert ratio <= NOISE_BOUND, (d, neg, hs, ratio)


def _chain_run(chain, d, dtype):
    In, Out = hi.tables(400, d, 1), hi.tables(400, d, 2)
    states = []
    for c in chain['centres']:
        loss = sr.step_sequential(chain['plan'], chain['cum'], In, Out, chain['seed'], 0, chain['neg'], LR, c, c + 1, dtype=dtype)
        states.append((In.copy(), Out.copy(), None, loss))
    return states


@pytest.mark.parametrize('d', [4, 32, 128])
def test_noise_floor_of_long_chain(chain, d):
    ratio = _worst(_chain_run(chain, d, np.float32), _chain_run(chain, d, np.float64))
    print(f'long_chain d {d}: float32 run / band = {ratio:.3f}')
    assert ratio <= NOISE_BOUND, (d, ratio)


def test_dtype_default_is_the_float64_loop(tiny):
    a, b = _tiny_run(tiny, 8, 5, True, np.float64), _tiny_run(tiny, 8, 5, True, np.float32)
    p, tree = tiny['plans'][0], hr.huffman(tiny['count'], 1)
    In, Out, Syn = hi.tables(7, 8, 1), hi.tables(7, 8, 2), hi.tables(tree['n_inner'], 8, 3)
    loss = hr.step_sequential_hs(p, tiny['cum'], In, Out, Syn, tree, tiny['seed'], 0, 5, LR, 0, 1)       # no dtype given
    assert np.array_equal(In, a[0][0]) and np.array_equal(Out, a[0][1]) and np.array_equal(Syn, a[0][2]) and loss == a[0][3]
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(a, b))         # and float32 arithmetic is a different run


# ---------------------------------------------------------------------------
# sensitivity: the band catches the bugs the GPU tests are aimed at
# ---------------------------------------------------------------------------
def _defect_ratio(data, plans, centres, d, neg, flags):
    """the largest band ratio of one launch of the wrong loop, started from the right loop's state"""
    n = data['n_aids']
    In, Out = hi.tables(n, d, 1), hi.tables(n, d, 2)
    worst = 0.0
    for ep, p in enumerate(plans):
        for c in (range(len(p['tok_aid'])) if centres is None else centres):
            In_b, Out_b = In.copy(), Out.copy()
            sr.step_sequential(p, data['cum'], In, Out, data['seed'], ep, neg, LR, c, c + 1)
            hi.step_variant(p, data['cum'], In_b, Out_b, data['seed'], ep, neg, LR, c, c + 1, **flags)
            worst = max(worst, hi.band_ratio(In_b, In), hi.band_ratio(Out_b, Out))
    return worst


def test_step_variant_without_a_defect_is_the_sequential_loop(tiny):
    for neg in (0, 5, 40):
        assert _defect_ratio(tiny, tiny['plans'], None, 16, neg, {}) == 0.0


@pytest.mark.parametrize('d', [4, 32, 128])
def test_the_band_catches_each_planted_defect(tiny, chain, d):
    bad = hi.planted_defects
    assert set(bad) == {'stale duplicate', 'no carry', 'dropped tail'}
    got = {}
    for neg in (3, 4, 5, 40, 64):
        got['stale duplicate', neg] = _defect_ratio(tiny, tiny['plans'], None, d, neg, bad['stale duplicate'])
    got['no carry', 5] = _defect_ratio(tiny, tiny['plans'], None, d, 5, bad['no carry'])
    for neg in (1, 4, 40):
        got['dropped tail', neg] = _defect_ratio(tiny, tiny['plans'], None, d, neg, bad['dropped tail'])
    full = chain['centres'][2:]
    got['stale duplicate', 'chain'] = _defect_ratio(chain, [chain['plan']], full, d, 64, bad['stale duplicate'])
    got['no carry', 'chain'] = _defect_ratio(chain, [chain['plan']], full, d, 64, bad['no carry'])
    for k, v in got.items():
        print(f'd {d} {k}: {v:.3g} x the band')
    assert min(got.values()) >= 100.0, got
    # neg = 0 leaves the carry as the only thing a centre's pairs share, and there its loss is of second order in lr (54 x
    # the band at d = 4, about 600 x at d = 32 and 128). A kernel with the bug stays within the band of the wrong loop, so it is
    # caught wherever the wrong loop is more than two bands from the right one.
    alone = _defect_ratio(tiny, tiny['plans'], None, d, 0, bad['no carry'])
    print(f'd {d} no carry at neg 0: {alone:.3g} x the band')
    assert alone >= 2.0
