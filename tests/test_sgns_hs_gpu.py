"""SPEC-SGNS-HS on the device (otto_sgns_step_hs, include/otto_sgns.h) against tests/sgns_hs_restatement.py: the batch step
on shallow and 64-deep paths, the entry with empty paths against otto_sgns_step, the hogwild step one centre at a time,
what hogwild with hs learns, the driver's switch and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import sgns_hs_restatement as hr
import sgns_inputs as si
import sgns_restatement as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6             # test_sgns_gpu.py's band
N_STEP_AIDS = 400


def _sg():
    from otto_amd.gensim_fasttext import skipgram
    return skipgram


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _close(got, want, what):
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=RTOL, atol=ATOL, err_msg=what)


class _Tables:
    """the restatement's tables in the shape SkipGramEngine(hs=...) takes"""

    def __init__(self, h):
        self.V, self.n_inner, self.max_len = h['V'], h['n_inner'], h['max_len']
        self.path_off, self.path_node = h['path_off'], h['path_node']
        self.code = np.array(h['code'], dtype=np.uint64)


# ---------------------------------------------------------------------------
# 1. batch step
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def step_data():
    # the sessions of test_sgns_gpu.py's step_data: 16 sessions, 400 aids, rows repeat heavily
    rng = np.random.default_rng(8)
    lens = [9, 1, 2, 9, 5, 9, 3, 9, 9, 9, 4, 9, 9, 6, 9, 9]
    sess_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    aid = np.minimum(rng.zipf(1.2, sess_off[-1]) - 1, N_STEP_AIDS - 1).astype(np.int32)
    count, keep_q, weight = _sg().vocab_tables(aid, N_STEP_AIDS, 1, 0.05, 0.5)
    plans = [sr.plan(aid, sess_off, keep_q, 6, ep, 3) for ep in (0, 1)]
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight), plans=plans,
                hs=hr.huffman(count, 1))


def _tables(d, n_inner, seed=1):
    rng = np.random.default_rng(seed)
    In = rng.uniform(-0.5, 0.5, (N_STEP_AIDS, d)).astype(np.float32)
    Out = rng.uniform(-0.5, 0.5, (N_STEP_AIDS, d)).astype(np.float32)
    Syn1 = rng.uniform(-0.5, 0.5, (n_inner, d)).astype(np.float32)
    return In, Out, Syn1


def _run_cut(gpu_device, sd, hs, d, neg, cut, epochs=(0, 1)):
    """consecutive epochs in launches of `cut` tokens, each launch against the restatement cut the same way; hs = None
    runs otto_sgns_step against tests/sgns_restatement.py"""
    import torch
    sg = _sg()
    eng = sg.SkipGramEngine(N_STEP_AIDS, d, 3, neg, sd['keep_q'], sd['weight'], seed=6, device=gpu_device,
                            hs=None if hs is None else _Tables(hs))
    In_h, Out_h, Syn_h = _tables(d, 1 if hs is None else hs['n_inner'])
    In, Out, Syn1 = _dev(In_h, gpu_device), _dev(Out_h, gpu_device), _dev(Syn_h, gpu_device)
    d_aid, d_off = _dev(sd['aid'], gpu_device), _dev(sd['sess_off'], gpu_device)
    inside_session, seen_ctx = False, set()
    for ep in epochs:
        p = sd['plans'][ep]
        plan = eng.plan(d_aid, d_off, ep)
        T = plan.T
        assert T == len(p['tok_aid']) and np.array_equal(plan.pair_off.cpu().numpy(), p['pair_off'])
        step = T if cut is None else cut
        for t0 in range(0, T, step):
            t1 = min(t0 + step, T)
            inside_session |= t1 < T and t1 not in set(p['tok_off'].tolist())
            npair = int(p['pair_off'][t1] - p['pair_off'][t0])
            ctx = torch.full((max(npair, 1),), -7, dtype=torch.int32, device=gpu_device)
            ngo = torch.full((max(npair, 1), max(neg, 1)), -7, dtype=torch.int32, device=gpu_device)
            lr = 0.05 * (1 - 0.1 * ep)
            if hs is None:
                loss = eng.step(plan, t0, t1, In, Out, lr, sg.BATCH, ctx_out=ctx, neg_out=ngo if neg else None)
                want = sr.step_batch(p, sd['cum'], In_h, Out_h, 6, ep, neg, lr, t0, t1)
            else:
                loss = eng.step(plan, t0, t1, In, Out, lr, sg.BATCH, ctx_out=ctx, neg_out=ngo if neg else None, Syn1=Syn1)
                want = hr.step_batch_hs(p, sd['cum'], In_h, Out_h, Syn_h, hs, 6, ep, neg, lr, t0, t1)
            wc, wn = sr.negatives(p, sd['cum'], 6, ep, neg, t0, t1, N_STEP_AIDS)
            seen_ctx |= set(wc.tolist())
            assert np.array_equal(ctx.cpu().numpy()[:npair], wc)                 # bit for bit: the same draws, the same keys
            if neg:
                assert np.array_equal(ngo.cpu().numpy()[:npair, :neg], wn)
            print(f'd {d} neg {neg} cut {cut} epoch {ep} [{t0}, {t1}): loss {loss.item():.9g} want {want:.9g}')
            assert abs(loss.item() - want) <= RTOL * abs(want) + ATOL
            _close(In, In_h, 'In')
            _close(Out, Out_h, 'Out')
            if hs is not None:
                _close(Syn1, Syn_h, 'Syn1')
    if hs is None:
        assert eng.Syn1 is None and np.array_equal(Syn1.cpu().numpy(), Syn_h)
    else:
        assert not bool(eng._gsyn1.any())
    assert not bool(eng._grads[0].any()) and not bool(eng._grads[1].any())      # the workspaces are zero again
    return inside_session, seen_ctx


@pytest.mark.parametrize('neg', [0, 1, 5, 40])
@pytest.mark.parametrize('d', [4, 32, 64, 128])
def test_batch_step_matches_the_restatement(gpu_device, step_data, d, neg):
    hs = step_data['hs']
    assert hs['V'] > 20 and hs['lens'].max() > 4 and (hs['lens'] == 0).any()     # out-of-vocabulary aids keep empty rows
    _run_cut(gpu_device, step_data, hs, d, neg, None)


@pytest.mark.parametrize('cut', [1, 7])
def test_batch_step_cut_into_launches(gpu_device, step_data, cut):
    inside, _ = _run_cut(gpu_device, step_data, step_data['hs'], 32, 5, cut)
    assert inside                       # a launch boundary fell inside a session


@pytest.fixture(scope='module')
def deep_data():
    # Fibonacci counts on 65 of the 400 aids: paths of 1 to 64 nodes, n_inner = 64; aid i has the i-th Fibonacci count, so
    # aids 0 and 1 are the deepest leaves and aid 64 the shallowest. Aids 65.. occur as events with empty paths.
    hs = hr.huffman(_fib_counts(), 1)
    rng = np.random.default_rng(12)
    lens = [5, 9, 2, 7, 9, 1, 9, 6]
    sess_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    aid = rng.integers(0, 80, sess_off[-1]).astype(np.int32)
    aid[1:4] = [0, 64, 1]                                        # deepest, shallowest, deepest, in one session
    _, keep_q, weight = _sg().vocab_tables(aid, N_STEP_AIDS, 1, 0.0, 0.5)
    return dict(aid=aid, sess_off=sess_off, keep_q=keep_q, weight=weight, cum=sr.cum_table(weight),
                plans=[sr.plan(aid, sess_off, keep_q, 6, 0, 3)], hs=hs)


@pytest.mark.parametrize('d', [4, 128])                          # 64 lane groups per workgroup, and 8
def test_deep_and_shallow_paths_in_one_launch(gpu_device, deep_data, d):
    sg = _sg()
    hs = deep_data['hs']
    assert hs['n_inner'] == 64 and hs['max_len'] == 64 and sorted(set(hs['lens'][:65].tolist())) == list(range(1, 65))
    assert hs['lens'][0] == 64 and hs['lens'][1] == 64 and hs['lens'][64] == 1
    assert {hs['code'][0] >> 63, hs['code'][1] >> 63} == {0, 1}                  # bit 63 of a code word is in use
    lib = sg.huffman_tables(_fib_counts(), 1)
    assert np.array_equal(lib.path_node, hs['path_node']) and lib.code.tolist() == hs['code']
    _, seen = _run_cut(gpu_device, deep_data, hs, d, 2, None, epochs=(0,))
    assert {0, 64} <= seen and (seen & set(range(65, 80)))       # the deepest, the shallowest and an empty path were contexts


def _fib_counts():
    fib = [1, 1]
    while len(fib) < 65:
        fib.append(fib[-1] + fib[-2])
    count = np.zeros(N_STEP_AIDS, dtype=np.int64)
    count[:65] = fib
    return count


def test_ns_entry_is_unchanged_around_an_hs_engine(gpu_device, step_data):
    # otto_sgns_step through an engine without tables, before and after otto_sgns_step_hs ran on the same device: the two
    # entries share the error word, the loss partials and the apply kernel
    _run_cut(gpu_device, step_data, None, 32, 5, None)
    _run_cut(gpu_device, step_data, step_data['hs'], 32, 5, None)
    _run_cut(gpu_device, step_data, None, 32, 5, None)


# ---------------------------------------------------------------------------
# 2. hogwild
# ---------------------------------------------------------------------------
N_RF_AIDS, N_RF_CHECK = 200000, 96


def _race_free_prefix(seed, aid, sess_off, keep_q, cum, neg):
    # test_sgns_gpu.py's construction: the leading sessions whose rows (contexts and negatives) are pairwise distinct
    head_off = sess_off[:N_RF_CHECK + 1]
    p = sr.plan(aid[:head_off[-1]], head_off, keep_q, seed, 0, 1)
    ctx, ng = sr.negatives(p, cum, seed, 0, neg, 0, len(p['tok_aid']), N_RF_AIDS)
    seen, k = set(), 0
    for s in range(N_RF_CHECK):
        rows = [int(x) for q in (2 * s, 2 * s + 1) for x in [ctx[q], *ng[q]]]
        if len(set(rows)) < len(rows) or seen & set(rows):
            break
        seen |= set(rows)
        k += 1
    return k, p


def test_empty_paths_equal_the_ns_entry_bit_for_bit(gpu_device):
    sg = _sg()
    neg, d = 2, 32
    perm = np.random.default_rng(1).permutation(N_RF_AIDS).astype(np.int32)       # every aid once: In rows never repeat
    aid, sess_off = perm, np.arange(0, N_RF_AIDS + 1, 2, dtype=np.int64)
    _, keep_q, weight = sg.vocab_tables(aid, N_RF_AIDS, 1, 0.0, 0.5)
    cum = sr.cum_table(weight)
    for seed in range(20):
        k, p = _race_free_prefix(seed, aid, sess_off, keep_q, cum, neg)
        if k >= 32:
            break
    assert k >= 32, 'no seed gives 32 sessions with pairwise distinct rows'
    one = np.zeros(N_RF_AIDS, dtype=np.int64)
    one[7] = 3
    tables = sg.huffman_tables(one, 1)                          # V = 1: every path empty, n_inner clamped to 1
    assert (tables.V, tables.n_inner, tables.path_node.size) == (1, 1, 0) and not tables.path_off.any()
    rng = np.random.default_rng(2)
    In_h = rng.uniform(-0.5, 0.5, (N_RF_AIDS, d)).astype(np.float32)
    Out_h = rng.uniform(-0.5, 0.5, (N_RF_AIDS, d)).astype(np.float32)
    d_aid, d_off = _dev(aid, gpu_device), _dev(sess_off, gpu_device)
    res = []
    for hs in (None, tables):
        eng = sg.SkipGramEngine(N_RF_AIDS, d, 1, neg, keep_q, weight, seed=seed, device=gpu_device, hs=hs)
        plan = eng.plan(d_aid, d_off, 0)
        In, Out = _dev(In_h, gpu_device), _dev(Out_h, gpu_device)
        Syn1 = _dev(np.full((1, d), 0.25, dtype=np.float32), gpu_device)
        loss = eng.step(plan, 0, 2 * k, In, Out, 0.05, sg.HOGWILD, **({} if hs is None else dict(Syn1=Syn1)))
        assert bool((Syn1 == 0.25).all())
        res.append((In.cpu().numpy(), Out.cpu().numpy(), loss.item()))
    assert not np.array_equal(res[0][0], In_h) and not np.array_equal(res[0][1], Out_h)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] and res[0][2] > 0


N_ONE_AIDS = 4000


def test_hogwild_equals_the_sequential_loop_one_centre_at_a_time(gpu_device):
    # every aid once, two-token sessions, ws = 1: the two centres of a session always share the root's row, so each runs as
    # its own launch; after each the three tables equal the sequential loop's
    sg = _sg()
    neg, d, seed = 2, 32, 3
    aid = np.random.default_rng(1).permutation(N_ONE_AIDS).astype(np.int32)
    sess_off = np.arange(0, N_ONE_AIDS + 1, 2, dtype=np.int64)
    count, keep_q, weight = sg.vocab_tables(aid, N_ONE_AIDS, 1, 0.0, 0.5)
    cum = sr.cum_table(weight)
    hs = hr.huffman(count, 1)
    assert hs['V'] == N_ONE_AIDS and hs['lens'].min() >= 11
    head = sess_off[:33]
    p = sr.plan(aid[:head[-1]], head, keep_q, seed, 0, 1)
    for s in range(32):                                          # the paths of a session's two contexts do meet
        a, b = (set(hs['path_node'][hs['path_off'][x]:hs['path_off'][x + 1]].tolist()) for x in aid[2 * s:2 * s + 2])
        assert a & b
    eng = sg.SkipGramEngine(N_ONE_AIDS, d, 1, neg, keep_q, weight, seed=seed, device=gpu_device, hs=_Tables(hs))
    plan = eng.plan(_dev(aid, gpu_device), _dev(sess_off, gpu_device), 0)
    assert plan.T == N_ONE_AIDS and np.array_equal(plan.tok_aid[:64].cpu().numpy(), p['tok_aid'])
    rng = np.random.default_rng(2)
    In_h, Out_h = (rng.uniform(-0.5, 0.5, (N_ONE_AIDS, d)).astype(np.float32) for _ in range(2))
    Syn_h = rng.uniform(-0.5, 0.5, (hs['n_inner'], d)).astype(np.float32)
    In, Out, Syn1 = _dev(In_h, gpu_device), _dev(Out_h, gpu_device), _dev(Syn_h, gpu_device)
    for c in range(64):
        loss = eng.step(plan, c, c + 1, In, Out, 0.05, sg.HOGWILD, Syn1=Syn1)
        want = hr.step_sequential_hs(p, cum, In_h, Out_h, Syn_h, hs, seed, 0, neg, 0.05, c, c + 1)
        assert abs(loss.item() - want) <= RTOL * want
        _close(In, In_h, f'In after centre {c}')
        _close(Out, Out_h, f'Out after centre {c}')
        _close(Syn1, Syn_h, f'Syn1 after centre {c}')


def test_hogwild_centre_with_two_pairs_walks_the_shared_rows_in_order(gpu_device):
    # the middle token of a three-token session has two pairs whose paths share the root: the second pair sees the first
    # pair's update of it and the h the first pair left, as in the sequential loop
    sg = _sg()
    n, d, neg, seed = 50, 64, 1, 5
    aid, sess_off = np.array([3, 9, 4], dtype=np.int32), np.array([0, 3], dtype=np.int64)
    count = np.arange(n, dtype=np.int64) % 7 + 1
    _, keep_q, weight = sg.vocab_tables(np.repeat(np.arange(n), count), n, 1, 0.0, 0.5)
    hs = hr.huffman(count, 1)
    eng = sg.SkipGramEngine(n, d, 1, neg, keep_q, weight, seed=seed, device=gpu_device, hs=_Tables(hs))
    plan = eng.plan(_dev(aid, gpu_device), _dev(sess_off, gpu_device), 0)
    p = sr.plan(aid, sess_off, keep_q, seed, 0, 1)
    assert p['pair_off'].tolist() == [0, 1, 3, 4]
    rng = np.random.default_rng(4)
    In_h, Out_h = (rng.uniform(-0.5, 0.5, (n, d)).astype(np.float32) for _ in range(2))
    Syn_h = rng.uniform(-0.5, 0.5, (hs['n_inner'], d)).astype(np.float32)
    In, Out, Syn1 = _dev(In_h, gpu_device), _dev(Out_h, gpu_device), _dev(Syn_h, gpu_device)
    loss = eng.step(plan, 1, 2, In, Out, 0.25, sg.HOGWILD, Syn1=Syn1)
    want = hr.step_sequential_hs(p, sr.cum_table(weight), In_h, Out_h, Syn_h, hs, seed, 0, neg, 0.25, 1, 2)
    assert abs(loss.item() - want) <= RTOL * want
    _close(In, In_h, 'In')
    _close(Out, Out_h, 'Out')
    _close(Syn1, Syn_h, 'Syn1')


# ---------------------------------------------------------------------------
# 3. hogwild with hs learns; the driver
# ---------------------------------------------------------------------------
def test_hogwild_with_hs_learns_the_planted_clusters(gpu_device):
    import torch
    from otto_amd.matrix_factorization.neighbours import neighbour_table
    sg = _sg()
    g = np.load(os.path.join(GOLDEN, 'sgns_hs_golden.npz'))
    recorded = g['purity']
    assert len(recorded) == 5 and recorded.min() >= 0.5          # chance is 1/12
    aid, sess_off, cluster = si.planted_sessions()
    In, Out, losses, Syn1 = sg.train(_dev(aid, gpu_device), _dev(sess_off, gpu_device), si.N_AIDS, dim=si.DIM, ws=si.WS,
                                     neg=si.NEG, epochs=si.EPOCHS, lr=si.LR, t=si.T, min_count=si.MIN_COUNT,
                                     ns_exponent=si.NS_EXPONENT, seed=int(si.GOLDEN_SEEDS[0]), mode=sg.HOGWILD,
                                     tokens_per_launch=si.TOKENS_PER_LAUNCH, hs=True)
    assert losses[0] > losses[1] > losses[2], losses
    assert all(bool(torch.isfinite(M).all()) for M in (In, Out, Syn1))
    assert tuple(Syn1.shape) == (si.N_AIDS - 1, si.DIM) and bool((Syn1 != 0).any(dim=1).all())    # every inner node was trained
    ids, _, _ = neighbour_table(In, k=10, metric='euclidean')
    purity = si.purity_from_ids(ids.cpu().numpy(), cluster)
    bound = recorded.min() - (recorded.max() - recorded.min())
    print(f'purity {purity:.4f}, recorded {recorded}, bound {bound:.4f}, losses {losses}, restatement losses {g["losses"][0]}')
    assert purity >= bound, (purity, recorded)


def test_driver_trains_the_path_half_when_the_config_asks(gpu_device, tmp_path, monkeypatch):
    import pandas as pd
    from otto_amd import settings
    from otto_amd.gensim_fasttext import trainer
    sg = _sg()
    aid, sess_off, _ = si.planted_sessions()
    session = np.repeat(np.arange(len(sess_off) - 1), np.diff(sess_off))
    df = pd.DataFrame({'session': session.astype(np.int32), 'aid': aid, 'ts': np.arange(len(aid), dtype=np.int64) + 1_600_000_000,
                       'type': np.zeros(len(aid), dtype=np.uint8)})
    monkeypatch.setattr(settings, 'MODELS', tmp_path / 'models')
    args = dict(vector_size=32, alpha=0.025, window=3, min_count=1, sample=0.003, seed=42, workers=32, min_alpha=0.0001, sg=1,
                negative=5, ns_exponent=0.75, epochs=1)
    out = {}
    for hs in (1, 0):
        config = {'model': {'model_name': 'Word2Vec', 'model_args': {**args, 'hs': hs}},
                  'persistence': {'model_directory': f'word2vec_hs{hs}'}}
        In, losses, root = trainer.run(config, df=df, device=str(gpu_device), n_aids=si.N_AIDS, tokens_per_launch=1000)
        assert root == tmp_path / 'models' / f'word2vec_hs{hs}' and len(losses) == 1 and np.isfinite(losses[0])
        saved = np.load(root / 'aid_embeddings.npy')
        assert saved.dtype == np.float32 and saved.shape == (si.N_AIDS, 32) and np.array_equal(saved, In)
        aids, vec = sg.load_vec(root / 'aid_embeddings.vec')
        assert len(aids) == si.N_AIDS
        np.testing.assert_allclose(vec, In[aids], rtol=5e-6, atol=0)
        out[hs] = In
    assert np.isfinite(out[1]).all() and not np.array_equal(out[1], out[0])      # the switch reaches the kernel


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_tables_unwritten(gpu_device, step_data):
    import torch
    from otto_amd import _lib
    sg = _sg()
    sd, hs, d, neg = step_data, step_data['hs'], 32, 5
    eng = sg.SkipGramEngine(N_STEP_AIDS, d, 3, neg, sd['keep_q'], sd['weight'], seed=6, device=gpu_device, hs=_Tables(hs))
    plan = eng.plan(_dev(sd['aid'], gpu_device), _dev(sd['sess_off'], gpu_device), 0)
    In_h, Out_h, Syn_h = _tables(d, hs['n_inner'])
    In, Out, Syn1 = _dev(In_h, gpu_device), _dev(Out_h, gpu_device), _dev(Syn_h, gpu_device)
    gin, gout, gsyn = (torch.zeros(M.shape, dtype=torch.float64, device=gpu_device) for M in (In, Out, Syn1))
    loss = torch.zeros(1, dtype=torch.float64, device=gpu_device)

    def call(mode, syn1, n_inner, gsyn1):
        eng._call('otto_sgns_step_hs', plan.tok_aid, plan.tok_src, plan.tok_left, plan.pair_off, plan.T, 0, plan.T, In, Out, d, neg,
                  0.05, mode, 6, 0, C.byref(eng.table), loss, None, None, 0, gin, gout, eng._path_off, eng._path_node, eng._code,
                  syn1, n_inner, gsyn1)

    for bad in (lambda: call(sg.HOGWILD, None, hs['n_inner'], None),             # null Syn1
                lambda: call(sg.HOGWILD, Syn1, 0, None),                        # n_inner = 0
                lambda: call(sg.BATCH, Syn1, hs['n_inner'], None),              # BATCH without gsyn1
                lambda: eng.step(plan, 0, plan.T, In, Out, 0.05, sg.HOGWILD)):  # the wrapper passes the null Syn1 on
        with pytest.raises(_lib.OttoError, match=r'code -22'):
            bad()
    short = _Tables(hs)
    short.path_off = hs['path_off'][:-1]
    with pytest.raises(ValueError, match='path_off'):
        sg.SkipGramEngine(N_STEP_AIDS, d, 3, neg, sd['keep_q'], sd['weight'], seed=6, device=gpu_device, hs=short)
    with pytest.raises(ValueError, match='Syn1'):
        eng.step(plan, 0, plan.T, In, Out, 0.05, sg.HOGWILD, Syn1=Syn1[:-1].contiguous())
    plain = sg.SkipGramEngine(N_STEP_AIDS, d, 3, neg, sd['keep_q'], sd['weight'], seed=6, device=gpu_device)
    with pytest.raises(ValueError, match='Syn1'):
        plain.step(plan, 0, plan.T, In, Out, 0.05, sg.HOGWILD, Syn1=Syn1)
    for M, M_h in ((In, In_h), (Out, Out_h), (Syn1, Syn_h)):
        assert np.array_equal(M.cpu().numpy(), M_h)
    assert not bool(gin.any()) and not bool(gout.any()) and not bool(gsyn.any())
    call(sg.BATCH, Syn1, hs['n_inner'], gsyn)                                   # and the same call with everything in place runs
    assert not np.array_equal(Syn1.cpu().numpy(), Syn_h) and not bool(gsyn.any())
