"""SPEC-SGNS-HS on the host: otto_sgns_hs_tree (a host function of the library) against the restatement array for array,
the prefix-code properties of the restatement itself, the 64-bit depth cap, the hand-worked case and the driver's switch."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import sgns_hs_restatement as hr
import sgns_inputs as si
import sgns_restatement as sr
from conftest import GOLDEN
from otto_amd import _lib
from otto_amd.gensim_fasttext import skipgram as sg
from test_sgns_cpu import FASTTEXT_ARGS, WORD2VEC_ARGS


def _fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _counts(case):
    rng = np.random.default_rng(11)
    if case.startswith('equal'):
        return [7] * int(case[5:]), 1
    if case == 'zipf5000':
        # V = 5,000 in-vocabulary aids between aids without an event and aids below min_count
        c = np.zeros(6500, dtype=np.int64)
        c[rng.permutation(6500)[:5000]] = 3 + np.minimum(rng.zipf(1.3, 5000), 10**6)
        low = np.flatnonzero(c == 0)
        c[low[::2]] = rng.integers(1, 3, len(low[::2]))
        assert int((c >= 3).sum()) == 5000 and (c == 0).any() and ((c > 0) & (c < 3)).any()
        return c.tolist(), 3
    if case == 'V0':
        return [0, 0, 2, 0], 3
    if case == 'V1':
        return [0, 5, 0, 1], 2
    if case == 'planted':
        aid, _, _ = si.planted_sessions()
        return np.bincount(aid, minlength=si.N_AIDS).tolist(), si.MIN_COUNT
    raise AssertionError(case)


CASES = ['equal2', 'equal3', 'equal64', 'equal65', 'equal1000', 'zipf5000', 'V0', 'V1', 'planted']


def _same(got, want):
    assert (got.V, got.n_inner, got.max_len) == (want['V'], want['n_inner'], want['max_len'])
    for k in ('path_off', 'path_node'):
        g = getattr(got, k)
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k
    assert got.code.dtype == np.uint64 and got.code.tolist() == want['code']


@pytest.mark.parametrize('case', CASES)
def test_library_tree_equals_the_restatement(case):
    count, min_count = _counts(case)
    want = hr.huffman(count, min_count)
    if case in ('V0', 'V1'):
        assert want['V'] == int(case[1]) and want['max_len'] == 0 and not want['path_off'].any()
    if case == 'planted':
        assert want['V'] == si.N_AIDS and want['lens'].min() >= 2
    _same(sg.huffman_tables(np.array(count), min_count), want)


@pytest.mark.parametrize('case', [c for c in CASES if c not in ('V0', 'V1')])
def test_restatement_is_a_prefix_code(case):
    count, min_count = _counts(case)
    h = hr.huffman(count, min_count)
    V = h['V']
    vocab = [a for a in range(len(count)) if count[a] >= max(min_count, 1)]
    assert len(vocab) == V and all(h['lens'][a] == 0 for a in range(len(count)) if a not in set(vocab))
    assert set(h['path_node'].tolist()) == set(range(V - 1))                   # every inner id appears
    words = sorted(format(h['code'][a], 'b').zfill(int(h['lens'][a]))[::-1] if h['lens'][a] else '' for a in vocab)
    assert all(len(w) > 0 for w in words)
    for a, b in zip(words, words[1:]):                                         # sorted: a prefix sits next to its extension
        assert not b.startswith(a), (a, b)
    assert sum(Fraction(1, 2 ** int(h['lens'][a])) for a in vocab) == 1        # Kraft, exactly
    assert sum(int(h['lens'][a]) * int(count[a]) for a in vocab) == sum(h['inner_count'])
    for a in vocab:                                                            # every path starts at the root V - 2
        assert h['path_node'][h['path_off'][a]] == V - 2


def test_depth_cap_at_64_bits():
    f65, f66 = _fibonacci(65), _fibonacci(66)
    w65, w66 = hr.huffman(f65), hr.huffman(f66)
    assert w65['max_len'] == 64 and w66['max_len'] == 65
    got = sg.huffman_tables(np.array(f65, dtype=np.int64))
    _same(got, w65)
    deepest = int(np.argmax(got.lengths()))
    assert got.max_len == 64 and got.lengths()[deepest] == 64 and w65['code'][deepest] >> 63 == 1
    assert int(got.code[deepest]) >> 63 == 1                                   # the bit in position 63 is set
    # 66 aids: sizes still answers (so the caller can see why), the fill refuses and writes nothing
    count = np.array(f66, dtype=np.int64)
    sizes = np.zeros(3, dtype=np.int64)
    _lib.call('otto_sgns_hs_tree_sizes', None, count, 66, 1, sizes.ctypes.data_as(C.POINTER(C.c_int64)), stream=False)
    assert sizes.tolist() == [66, int(w66['lens'].sum()), 65]
    path_off = np.full(67, 0x55, dtype=np.int64)
    path_node = np.full(int(sizes[1]), 0x55, dtype=np.int32)
    code = np.full(66, 0x55, dtype=np.uint64)
    with pytest.raises(_lib.OttoError, match=r'code -22'):
        _lib.call('otto_sgns_hs_tree', None, count, 66, 1, path_off, path_node, path_node.size, code, stream=False)
    assert (path_off == 0x55).all() and (path_node == 0x55).all() and (code == 0x55).all()
    with pytest.raises(_lib.OttoError, match=r'code -22'):
        sg.huffman_tables(count)
    # too little room for the ids is refused the same way
    with pytest.raises(_lib.OttoError, match=r'code -22'):
        _lib.call('otto_sgns_hs_tree', None, np.array(f65, dtype=np.int64), 65, 1, path_off, path_node, got.path_node.size - 1, code,
                  stream=False)
    assert (path_off == 0x55).all() and (path_node == 0x55).all() and (code == 0x55).all()
    with pytest.raises(_lib.OttoError, match=r'code -22'):
        sg.huffman_tables(np.array([3, -1, 2]))


def test_hs_requested():
    from otto_amd.gensim_fasttext import trainer
    cfg = lambda name, args: {'model': {'model_name': name, 'model_args': args}}
    assert trainer.hs_requested(cfg('Word2Vec', WORD2VEC_ARGS)) is True
    assert trainer.hs_requested(cfg('FastText', FASTTEXT_ARGS)) is False
    assert trainer.hs_requested(cfg('Word2Vec', {**WORD2VEC_ARGS, 'hs': 0})) is False
    assert trainer.hs_requested(cfg('Word2Vec', {k: v for k, v in WORD2VEC_ARGS.items() if k != 'hs'})) is False
    assert trainer.hs_requested(cfg('FastText', {**FASTTEXT_ARGS, 'hs': 1})) is False


def test_warning_says_what_is_trained(caplog):
    from otto_amd.gensim_fasttext import trainer
    trainer._HS_WARNED = False
    with caplog.at_level('WARNING'):
        trainer.word2vec_args(WORD2VEC_ARGS)
        trainer.word2vec_args(WORD2VEC_ARGS)
    msgs = [r.message for r in caplog.records if 'hierarchical softmax' in r.message]
    assert len(msgs) == 1 and 'not built' not in msgs[0] and 'word2vec.c' in msgs[0] and 'negative-sampling' in msgs[0]
    assert all(r.levelname == 'WARNING' for r in caplog.records if 'hierarchical softmax' in r.message)


@pytest.fixture(scope='module')
def hand():
    with open(os.path.join(GOLDEN, 'sgns_hs_hand.json')) as fh:
        return json.load(fh)


def test_tree_of_the_hand_case(hand):
    w = hr.huffman(hand['count'], hand['min_count'])
    for k in ('V', 'n_inner', 'max_len', 'code', 'inner_count'):
        assert w[k] == hand[k], k
    assert w['path_off'].tolist() == hand['path_off'] and w['path_node'].tolist() == hand['path_node']
    _same(sg.huffman_tables(np.array(hand['count']), hand['min_count']), w)


@pytest.mark.parametrize('which', ['sequential', 'batch'])
def test_restatement_steps_match_the_hand_case(hand, which):
    hs = hr.huffman(hand['count'], hand['min_count'])
    keep_q = np.full(len(hand['count']), 2**32 - 1, dtype=np.uint32)
    p = sr.plan(np.array(hand['aid'], dtype=np.int32), np.array(hand['sess_off'], dtype=np.int64), keep_q, hand['seed'],
                hand['epoch'], hand['ws'])
    assert p['tok_aid'].tolist() == hand['aid'] and p['pair_off'].tolist() == [0, 1, 2]
    cum = sr.cum_table(np.ones(len(hand['count']), dtype=np.uint32))
    In, Out, Syn1 = (np.array(hand[k], dtype=np.float32) for k in ('In', 'Out', 'Syn1'))
    fn = hr.step_sequential_hs if which == 'sequential' else hr.step_batch_hs
    loss = fn(p, cum, In, Out, Syn1, hs, hand['seed'], hand['epoch'], hand['neg'], hand['lr'], hand['t0'], hand['t1'])
    # float64 arithmetic rounded to float32 once per stored row on both sides: the last float32 bit may differ
    for k, M in (('In', In), ('Out', Out), ('Syn1', Syn1)):
        np.testing.assert_allclose(M, np.array(hand['after'][k], dtype=np.float32), rtol=2.5e-7, atol=0, err_msg=k)
        assert not np.array_equal(M, np.array(hand[k], dtype=np.float32)), k          # the step wrote the table
    assert abs(loss - hand['after']['loss']) <= 1e-12 * hand['after']['loss']
