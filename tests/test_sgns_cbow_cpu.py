"""SPEC-CBOW and SPEC-DOC2VEC on the host: the restatement (tests/sgns_cbow_restatement.py) against the hand-worked case and
against the skip-gram HS restatement where the two coincide, the config mapping `resolve` and its refusals, the independence
of the launch cut, the properties of the edge input, and the layout of the job record."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sgns_cbow_inputs as ci
import sgns_cbow_restatement as cr
import sgns_hogwild_inputs as hi
import sgns_hs_restatement as hr
import sgns_restatement as sr
from conftest import GOLDEN
from otto_amd.gensim_fasttext import skipgram as sg


# ---------------------------------------------------------------------------
# the hand case
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'sgns_cbow_hand.json')) as fh:
        return json.load(fh)


@pytest.mark.parametrize('which', ['sequential', 'batch'])
@pytest.mark.parametrize('variant', ['sum', 'mean', 'fasttext'])
def test_restatement_matches_the_hand_case(hand, variant, which):
    keep_q = np.full(5, ci.U32, dtype=np.uint32)
    p = sr.plan(np.array(hand['aid'], dtype=np.int32), np.array(hand['sess_off'], dtype=np.int64), keep_q, hand['seed'], hand['epoch'],
                hand['ws'])
    assert p['tok_left'].tolist() == [0, 1, 1] and p['pair_off'].tolist() == [0, 1, 3, 4] and p['tok_off'].tolist() == [0, 3]
    hs = dict(path_off=np.array(hand['path_off']), path_node=np.array(hand['path_node'], dtype=np.int32), code=hand['code'])
    lib = hr.huffman(hand['count'], hand['min_count'])
    assert lib['path_node'].tolist() == hand['path_node'] and lib['code'] == hand['code'] and lib['n_inner'] == hand['n_inner']
    tabs = {k: np.array(hand[k], dtype=np.float32) for k in ('In', 'Out', 'Syn1', 'Doc')}
    fn = cr.step_sequential if which == 'sequential' else cr.step_batch
    loss = fn(p, None, tabs, hs, hand['seed'], hand['epoch'], 0, hand['lr'], hand['t0'], hand['t1'], cr.PVDM,
              dict(sum=cr.SUM, mean=cr.MEAN, fasttext=cr.FASTTEXT)[variant])
    want = hand['after'][variant]
    assert abs(loss - want['loss']) <= 1e-12 * want['loss']
    for k in tabs:
        np.testing.assert_allclose(tabs[k], np.array(want[k], dtype=np.float32), rtol=1.5e-7, atol=1e-9, err_msg=k)
    for k, rows in (('In', [0, 2]), ('Doc', [0]), ('Out', [1]), ('Syn1', [0, 1, 2, 3])):       # exactly these rows moved
        moved = np.flatnonzero((tabs[k] != np.array(hand[k], dtype=np.float32)).any(axis=1)).tolist()
        assert moved == rows, (k, moved)


def test_the_three_variants_of_the_hand_case_differ(hand):
    a = hand['after']
    assert a['sum']['loss'] != a['mean']['loss'] == a['fasttext']['loss']        # FASTTEXT shares the mean's h
    assert a['mean']['In'] != a['fasttext']['In'] and a['mean']['Syn1'] == a['fasttext']['Syn1']


# ---------------------------------------------------------------------------
# where CBOW and skip-gram coincide
# ---------------------------------------------------------------------------
def test_sum_variant_equals_the_skipgram_hs_step_on_two_token_sessions():
    # sessions (a, b) over a permutation, neg = 0, HS: the CBOW centre a reads h = In[b] and walks the path of a; the
    # skip-gram centre b reads h = In[b] and walks the path of its context a. The same hidden row meets the same path, the
    # same Out row, and In[b] takes the same gradient.
    n, d = 64, 8
    aid = np.random.default_rng(5).permutation(n).astype(np.int32)
    sess_off = np.arange(0, n + 1, 2, dtype=np.int64)
    keep_q = np.full(n, ci.U32, dtype=np.uint32)
    hs = hr.huffman(np.arange(n) % 5 + 1, 1)
    assert hs['V'] == n and hs['lens'].min() >= 3
    p = sr.plan(aid, sess_off, keep_q, 7, 0, 1)
    assert np.array_equal(np.diff(p['pair_off']), np.ones(n))
    rng = np.random.default_rng(6)
    In, Out = (rng.uniform(-0.5, 0.5, (n, d)).astype(np.float32) for _ in range(2))
    Syn1 = rng.uniform(-0.5, 0.5, (hs['n_inner'], d)).astype(np.float32)
    tabs = dict(In=In.copy(), Out=Out.copy(), Syn1=Syn1.copy())
    loss = cr.step_batch(p, None, tabs, hs, 7, 0, 0, 0.05, 0, n, cr.CBOW, cr.SUM)
    want = hr.step_batch_hs(p, None, In, Out, Syn1, hs, 7, 0, 0, 0.05, 0, n)
    assert abs(loss - want) <= 1e-12 * want
    for k, M in (('In', In), ('Out', Out), ('Syn1', Syn1)):
        np.testing.assert_allclose(tabs[k], M, rtol=2e-7, atol=1e-9, err_msg=k)       # float64 sums in another order
    assert not np.array_equal(tabs['Syn1'], np.random.default_rng(6).uniform(-0.5, 0.5, (n, d)))


# ---------------------------------------------------------------------------
# resolve
# ---------------------------------------------------------------------------
FASTTEXT_ARGS = dict(model='cbow', lr=0.05, dim=32, ws=10, epoch=5, minCount=1, minn=0, maxn=0, neg=40, wordNgrams=1, loss='ns',
                     bucket=2000000, thread=32, lrUpdateRate=100, t=0.0001, verbose=2)
GENSIM_ARGS = dict(vector_size=32, alpha=0.025, window=12, min_count=1, sample=0.003, seed=42, workers=32, min_alpha=0.0001,
                   negative=40, ns_exponent=0.75, epochs=5)
GENSIM_KW = dict(dim=32, ws=12, neg=40, epochs=5, lr=0.025, t=0.003, min_count=1, ns_exponent=0.75, seed=42)


def _cfg(name, args):
    return {'model': {'model_name': name, 'model_args': args}}


def test_resolve_mappings():
    from otto_amd.gensim_fasttext import trainer
    arch, kw = trainer.resolve(_cfg('FastText', FASTTEXT_ARGS))
    assert arch == 'cbow' and kw == dict(dim=32, ws=10, neg=40, epochs=5, lr=0.05, t=1e-4, min_count=1, ns_exponent=0.5, seed=0, hs=False,
                                         variant=sg.CBOW_FASTTEXT)
    for mean, variant in ((1, sg.CBOW_MEAN), (0, sg.CBOW_SUM)):
        arch, kw = trainer.resolve(_cfg('Word2Vec', {**GENSIM_ARGS, 'sg': 0, 'cbow_mean': mean}))
        assert arch == 'cbow' and kw == dict(GENSIM_KW, hs=False, variant=variant)
    assert trainer.resolve(_cfg('Word2Vec', {**GENSIM_ARGS, 'sg': 0}))[1]['variant'] == sg.CBOW_MEAN      # gensim's default
    arch, kw = trainer.resolve(_cfg('Word2Vec', {**GENSIM_ARGS, 'sg': 0, 'hs': 1, 'negative': 0}))       # hs alone
    assert arch == 'cbow' and kw['hs'] is True and kw['neg'] == 0
    for args, dm, dm_mean in ((dict(dm=1, dm_mean=1), 1, 1), (dict(dm=1, dm_mean=0), 1, 0), (dict(dm=1), 1, 1),
                              (dict(dm=1, dm_mean=None), 1, 1), (dict(dm=0), 0, 1), ({}, 1, 1)):
        arch, kw = trainer.resolve(_cfg('Doc2Vec', {**GENSIM_ARGS, **args}))
        assert arch == 'doc2vec' and kw == dict(GENSIM_KW, hs=False, dm=dm, dm_mean=dm_mean), args
    arch, kw = trainer.resolve(_cfg('Doc2Vec', {**GENSIM_ARGS, 'dm': 0, 'hs': 1, 'negative': 0}))
    assert arch == 'doc2vec' and kw['hs'] is True and kw['neg'] == 0 and kw['dm'] == 0
    # the skip-gram configs go where they went
    arch, kw = trainer.resolve(_cfg('FastText', {**FASTTEXT_ARGS, 'model': 'skipgram'}))
    assert arch == 'skipgram' and kw == dict(trainer.fasttext_args({**FASTTEXT_ARGS, 'model': 'skipgram'}), hs=False)
    arch, kw = trainer.resolve(_cfg('Word2Vec', {**GENSIM_ARGS, 'sg': 1, 'hs': 1}))
    assert arch == 'skipgram' and kw == dict(GENSIM_KW, hs=True)
    # and the keywords are the trainers' own
    import inspect
    for fn, cfg in ((sg.train_cbow, _cfg('FastText', FASTTEXT_ARGS)), (sg.train_doc2vec, _cfg('Doc2Vec', GENSIM_ARGS)),
                    (sg.train, _cfg('Word2Vec', {**GENSIM_ARGS, 'sg': 1}))):
        assert set(trainer.resolve(cfg)[1]) <= set(inspect.signature(fn).parameters)


def test_resolve_refusals():
    from otto_amd.gensim_fasttext import trainer
    bad = [('FastText', {**FASTTEXT_ARGS, 'loss': 'hs'}), ('FastText', {**FASTTEXT_ARGS, 'loss': 'softmax'}),
           ('FastText', {**FASTTEXT_ARGS, 'minn': 3, 'maxn': 6}), ('FastText', {**FASTTEXT_ARGS, 'maxn': 6}),
           ('FastText', {**FASTTEXT_ARGS, 'model': 'supervised'}), ('FastText', {**FASTTEXT_ARGS, 'neg': 0}),
           ('Word2Vec', {**GENSIM_ARGS, 'sg': 0, 'negative': 0}), ('Word2Vec', {**GENSIM_ARGS, 'sg': 1, 'negative': 0, 'hs': 1}),
           ('Doc2Vec', {**GENSIM_ARGS, 'dm_concat': 1}), ('Doc2Vec', {**GENSIM_ARGS, 'dbow_words': 1}),
           ('Doc2Vec', {**GENSIM_ARGS, 'dm_tag_count': 2}), ('Doc2Vec', {**GENSIM_ARGS, 'negative': 0}), ('GloVe', {})]
    for name, args in bad:
        with pytest.raises(ValueError):
            trainer.resolve(_cfg(name, args))
    with pytest.raises(ValueError):                              # run refuses before any file or device is touched
        trainer.run({**_cfg('Doc2Vec', {**GENSIM_ARGS, 'dm_concat': 1}), 'persistence': {'model_directory': 'x'}}, df=object())


def test_trainers_refuse_no_objective_before_touching_a_device():
    for fn in (sg.train_cbow, sg.train_doc2vec):
        with pytest.raises(ValueError, match='nothing to train'):
            fn(None, None, 10, neg=0, hs=False, device='cpu')
    D0, D1 = sg.init_doc(7, 8, seed=3), sg.init_doc(7, 8, seed=4)
    assert D0.dtype == np.float32 and D0.shape == (7, 8) and np.abs(D0).max() <= 1 / 8 and not np.array_equal(D0, D1)
    assert np.array_equal(D0, np.random.default_rng([3, 1]).uniform(-1 / 8, 1 / 8, (7, 8)).astype(np.float32))


# ---------------------------------------------------------------------------
# the edge input; the launch cut
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def edge():
    return ci.edge_input()


def test_edge_input_has_its_edges(edge):
    count, keep_q, weight = sg.vocab_tables(edge['aid'], ci.EDGE_AIDS, ci.EDGE_MIN_COUNT, 0.0, 0.5)
    assert np.array_equal(count, edge['count']) and np.array_equal(keep_q, edge['keep_q']) and np.array_equal(weight, edge['weight'])
    assert (count[:30] >= 2).all() and (count[30:36] == 1).all() and not count[36:].any()
    assert not keep_q[30:].any() and not weight[30:].any()       # singletons are dropped and never drawn
    for p in edge['plans']:
        assert tuple(np.diff(p['tok_off'])) == ci.EDGE_KEPT and (p['tok_aid'] < 30).all()
        npairs = np.diff(p['pair_off'])
        assert npairs[0] == 0                                    # the one-token session: a CBOW centre that is skipped
        assert p['tok_aid'][3:6].tolist() == [4, 4, 9] and cr.context_aids(p, 3) [:1] == [4]      # a context equal to its centre's aid
    p = edge['plans'][0]
    npairs = np.diff(p['pair_off'])
    assert npairs.max() == 2 * ci.EDGE_WS == 64                  # OTTO_SGNS_MAX_WS on both sides
    assert cr.context_aids(p, 5) == [4, 4]                       # a window holding one aid twice
    full = int(np.argmax(npairs))
    ctx = cr.context_aids(p, full)
    assert len(ctx) == 64 and len(set(ctx)) < 64 and int(p['tok_aid'][full]) in ctx
    assert edge['hs']['V'] == 30 and (edge['hs']['lens'][30:] == 0).all() and edge['hs']['lens'][:30].min() >= 3


def _edge_tables(edge, d=8, seed=1):
    rng = np.random.default_rng(seed)
    S = len(edge['sess_off']) - 1
    return dict(In=rng.uniform(-0.5, 0.5, (ci.EDGE_AIDS, d)).astype(np.float32), Out=rng.uniform(-0.5, 0.5, (ci.EDGE_AIDS, d)).astype(np.float32),
                Syn1=rng.uniform(-0.5, 0.5, (edge['hs']['n_inner'], d)).astype(np.float32), Doc=rng.uniform(-0.5, 0.5, (S, d)).astype(np.float32))


@pytest.mark.parametrize('name,arch,variant', ci.ARCHS, ids=[a[0] for a in ci.ARCHS])
def test_the_launch_cut_changes_nothing(edge, name, arch, variant):
    p, neg = edge['plans'][0], 3
    T = len(p['tok_aid'])
    whole = cr.negatives(p, edge['cum'], ci.EDGE_SEED, 0, neg, 0, T, ci.EDGE_AIDS)
    assert (whole != p['tok_aid'][:, None]).all() and (whole < 30).all() and len(np.unique(whole)) > 10
    ref = _edge_tables(edge)
    want = cr.step_sequential(p, edge['cum'], ref, edge['hs'], ci.EDGE_SEED, 0, neg, 0.05, 0, T, arch, variant)
    for cut in (1, 7):
        tabs = _edge_tables(edge)
        loss = 0.0
        for t0 in range(0, T, cut):
            t1 = min(t0 + cut, T)
            assert np.array_equal(cr.negatives(p, edge['cum'], ci.EDGE_SEED, 0, neg, t0, t1, ci.EDGE_AIDS), whole[t0:t1])
            loss += cr.step_sequential(p, edge['cum'], tabs, edge['hs'], ci.EDGE_SEED, 0, neg, 0.05, t0, t1, arch, variant)
        if arch == cr.DBOW:
            # a cut inside a session stores the doc row as float32 and reads it back: float32 rounding, nothing more
            assert hi.band_ratio(loss, want) <= 1 and all(hi.band_ratio(tabs[k], ref[k]) <= 1 for k in tabs)
            assert np.array_equal(tabs['In'], _edge_tables(edge)['In'])          # DBOW never touches In
        else:
            assert abs(loss - want) <= 1e-12 * want and all(np.array_equal(tabs[k], ref[k]) for k in tabs), cut
    # and the draws of stream 4 are not the skip-gram draws of stream 3
    _, sg_negs = sr.negatives(p, edge['cum'], ci.EDGE_SEED, 0, neg, 0, T, ci.EDGE_AIDS)
    first_pair = p['pair_off'][:-1][np.diff(p['pair_off']) > 0]
    assert not np.array_equal(sg_negs[first_pair], whole[np.diff(p['pair_off']) > 0])


def test_batch_and_sequential_agree_where_no_row_is_shared():
    pm = dict(aid=np.random.default_rng(2).permutation(40).astype(np.int32), sess_off=np.arange(0, 41, 2, dtype=np.int64), T=40)
    p = hi.permutation_plan(pm)
    for fn in (cr.step_sequential, cr.step_batch):
        tabs, want = ci.permutation_tables(pm, 8), ci.permutation_tables(pm, 8)
        wl = ci.permutation_cbow_step(pm, want, 0.05)
        loss = fn(p, None, tabs, None, 9, 0, 0, 0.05, 0, 40, cr.CBOW, cr.MEAN)
        assert abs(loss - wl) <= 1e-12 * wl and all(np.array_equal(tabs[k], want[k]) for k in tabs)


def test_target_counts():
    e = ci.edge_input()
    p, hs = e['plans'][0], e['hs']
    T = len(p['tok_aid'])
    paths = int(hs['lens'][p['tok_aid']].sum())
    assert cr.count_targets(p, None, 3, 0, T, cr.DBOW) == 4 * T == cr.count_targets(p, None, 3, 0, T, cr.PVDM)
    assert cr.count_targets(p, None, 3, 0, T, cr.CBOW) == 4 * (T - 1)            # the one-token session trains nothing
    assert cr.count_targets(p, hs, 0, 0, T, cr.PVDM) == T + paths


# ---------------------------------------------------------------------------
# the job record
# ---------------------------------------------------------------------------
def test_job_record_layout_is_the_header_s():
    from otto_amd import _lib
    J = _lib.SgnsCbowJob
    # include/otto_sgns.h, field by field on an LP64 target: 5 pointers, 4 int64, 4 pointers, 2 int64, d, neg, lr, arch,
    # variant, mode (4 bytes each), seed, epoch, the table (44 bytes padded to 48), 3 + 2 + 4 pointers, the stream
    assert C.sizeof(_lib.SgnsTable) == 48 and C.sizeof(J) == 288
    want = dict(d_tok_aid=0, d_tok_off=32, T=40, t0=56, d_In=72, d_Doc=96, n_aids=104, d=120, neg=124, lr=128, arch=132, variant=136,
                mode=140, seed=144, epoch=152, table=160, d_path_off=208, d_loss_sum=232, d_neg_out=240, d_gin=248, d_gdoc=272, stream=280)
    assert {k: getattr(J, k).offset for k in want} == want
    assert _lib.SIGNATURES['otto_sgns_cbow_step'][1][0]._type_ is J and len(_lib.SIGNATURES['otto_sgns_cbow_step'][1]) == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'otto_sgns.h')).read()
    body = header[header.index('typedef struct otto_sgns_cbow_job {'):header.index('} otto_sgns_cbow_job;')]
    import re
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split('{', 1)[1].split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
    assert names == [f[0] for f in J._fields_]                   # the same fields in the same order
    for word in ('SPEC-CBOW', 'SPEC-DOC2VEC', 'OTTO_SGNS_CBOW_FASTTEXT', 'dm_mean'):
        assert word in header
