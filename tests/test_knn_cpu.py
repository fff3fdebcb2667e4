"""SPEC-KNN without a GPU: the float64 restatement against a hand-computed fixture, the fourth candidate generator
against the reference loop restated here, argument validation, the rank split, and the check that the inputs of the
GPU parity tests keep the restatement's own near-tie share under 1 %."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import knn_restatement as kr


def _hand():
    with open(os.path.join(GOLDEN, 'knn_hand.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('case', range(4))
def test_restatement_matches_hand_computed_fixture(case):
    h = _hand()
    c = h['cases'][case]
    E = np.array(h['points'], dtype=np.float32)
    valid = np.array(h['valid'], dtype=np.uint8)
    ids, value, n, keys, _ = kr.knn(E, c['k'], c['metric'], valid=valid, rows=np.array(c['rows']))
    want_key = np.array([[np.inf if v is None else v for v in row] for row in c['key']], dtype=np.float64)
    assert ids.tolist() == c['ids'], c['name']
    assert n.tolist() == c['n']
    assert np.allclose(keys, want_key, rtol=0, atol=1e-12), c['name']
    fin = np.isfinite(want_key)
    want_value = -want_key if c['metric'] == 'dot' else np.sqrt(np.where(fin, want_key, 0.0))
    assert np.allclose(value[fin], want_value[fin], rtol=0, atol=1e-12)
    assert np.all(np.isinf(value[~fin])) and np.all(ids[~fin] == -1)


def test_restatement_fixture_covers_what_it_claims():
    h = _hand()
    E = np.array(h['points'], dtype=np.float32)
    valid = np.array(h['valid'], dtype=np.uint8)
    ids, value, n, _, _ = kr.knn(E, 3, 'euclidean', valid=valid)          # rows = None: all aids, in order
    sub = kr.knn(E, 3, 'euclidean', valid=valid, rows=np.array([0, 3, 4, 5, 9]))
    assert np.array_equal(ids[[0, 3, 4, 5, 9]], sub[0]) and np.array_equal(n[[0, 3, 4, 5, 9]], sub[2])
    assert ids[3, 0] == 4 and ids[4, 0] == 3 and value[3, 0] == 0 and value[4, 0] == 0      # twins list each other first
    assert all(a not in ids[a] for a in range(len(E)))                                       # nobody lists itself
    assert not (ids == 5).any() and n[5] == 0                                                # the invalid aid
    assert n.tolist() == [3] * 5 + [0] + [3] * 6


# ---- the fourth candidate generator -----------------------------------------------------------------------------------

def _reference_loop(session_aids, table, n_candidates, labels, session_ids):
    """src/ranker/fasttext_candidate_generator.py:75-98,118-136 restated: per session the neighbours of the LAST aid
    (the index's first hit, the item itself, is already absent from our table), their distances as scores, one label per
    candidate = membership in the session's ground truth of the type; exploded, sessions without candidates dropped."""
    ids, dist, n = table
    rows = []
    for s, aids in enumerate(session_aids):
        if not len(aids):
            continue
        last = aids[-1]
        sorted_aids = [int(a) for a in ids[last][:n[last]][:n_candidates]]
        sorted_dist = [float(x) for x in dist[last][:n[last]][:n_candidates]]
        for a, x in zip(sorted_aids, sorted_dist):
            row = [session_ids[s] if session_ids is not None else s, a, x]
            if labels is not None:
                row.append(int(a in labels[s]))
            rows.append(row)
    return rows


def _toy():
    import torch
    rng = np.random.default_rng(5)
    N, k = 30, 8
    ids = np.full((N, k), -1, dtype=np.int32)
    dist = np.full((N, k), np.inf, dtype=np.float32)
    n = rng.integers(0, k + 1, N).astype(np.int32)
    n[7] = 0                                   # an aid with an empty row
    for a in range(N):
        ids[a, :n[a]] = rng.choice(np.setdiff1d(np.arange(N), [a]), size=n[a], replace=False)
        dist[a, :n[a]] = np.sort(rng.random(n[a])).astype(np.float32)
    sessions = [list(rng.integers(0, N, rng.integers(1, 6))) for _ in range(12)]
    sessions[3][-1] = 7                        # ends on the aid with the empty row -> no rows
    sessions[5] = []                           # no events -> no rows
    sessions[8][-1] = sessions[8][0]
    labels = [set(int(x) for x in rng.integers(0, N, rng.integers(0, 6))) for _ in sessions]
    for s, aids in enumerate(sessions):        # at least one positive label, on the nearest neighbour
        if len(aids) and n[aids[-1]] > 0:
            labels[s].add(int(ids[aids[-1], 0]))
            break
    aid = torch.tensor([a for s in sessions for a in s], dtype=torch.int32)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in sessions])]), dtype=torch.int64)
    l_off = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in labels])]), dtype=torch.int64)
    l_aid = torch.tensor([a for x in labels for a in sorted(x)], dtype=torch.int32)
    sid = torch.tensor(1000 + 3 * np.arange(len(sessions)), dtype=torch.int64)
    return (ids, dist, n), sessions, labels, aid, off, (l_off, l_aid), sid


@pytest.mark.parametrize('with_labels', [True, False])
@pytest.mark.parametrize('n_candidates', [1, 5, 8])
def test_neighbour_candidates_frame_matches_reference_loop(with_labels, n_candidates):
    import torch
    from otto_amd.matrix_factorization.neighbours import neighbour_candidates_frame
    table, sessions, labels, aid, off, csr, sid = _toy()
    t_table = tuple(torch.from_numpy(x) for x in table)
    df = neighbour_candidates_frame(aid, off, t_table, n_candidates=n_candidates, labels=csr if with_labels else None,
                                    session_ids=sid)
    want = _reference_loop(sessions, table, n_candidates, labels if with_labels else None, sid.tolist())
    cols = ['session', 'candidates', 'candidate_scores'] + (['candidate_labels'] if with_labels else [])
    assert list(df.columns) == cols
    assert df['candidates'].dtype == np.uint64 and df['candidate_scores'].dtype == np.float32
    assert df['session'].dtype == np.int64
    if with_labels:
        assert df['candidate_labels'].dtype == np.uint8
        assert df['candidate_labels'].sum() > 0
    assert len(df) == len(want) and len(want) > 0
    got = [list(r) for r in df.itertuples(index=False)]
    assert [[int(r[0]), int(r[1]), float(r[2])] + [int(x) for x in r[3:]] for r in got] == want
    assert sid[3].item() not in set(df['session']) and sid[5].item() not in set(df['session'])


def test_neighbour_candidates_without_session_ids_uses_the_index():
    import torch
    from otto_amd.matrix_factorization.neighbours import neighbour_candidates
    table, sessions, labels, aid, off, csr, sid = _toy()
    out = neighbour_candidates(aid, off, tuple(torch.from_numpy(x) for x in table), n_candidates=5)
    want = _reference_loop(sessions, table, 5, None, None)
    assert out['candidate_labels'] is None
    assert out['session'].tolist() == [r[0] for r in want] and out['candidates'].tolist() == [r[1] for r in want]
    assert out['row_off'][-1].item() == len(want) and out['row_off'].numel() == len(sessions) + 1


# ---- validation, refusal, rank split ------------------------------------------------------------------------------------

def test_bad_arguments_raise_value_error_before_the_library_is_touched(monkeypatch):
    import torch
    from otto_amd import _lib
    from otto_amd.matrix_factorization.neighbours import neighbour_table

    def boom():
        raise AssertionError('the library must not be touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    E = torch.zeros((10, 32), dtype=torch.float32)
    for kw in ({'k': 0}, {'k': 65}, {'metric': 'manhattan'}):
        with pytest.raises(ValueError):
            neighbour_table(E, **kw)
    with pytest.raises(ValueError):
        neighbour_table(torch.zeros((10, 24), dtype=torch.float32))            # unsupported d
    with pytest.raises(ValueError):
        neighbour_table(E.double())                                             # dtype
    with pytest.raises(ValueError):
        neighbour_table(torch.zeros((10, 64), dtype=torch.float32)[:, ::2])     # not contiguous
    with pytest.raises(ValueError):
        neighbour_table(E, rows=torch.arange(3))                                # int64 rows
    with pytest.raises(ValueError):
        neighbour_table(E, valid=torch.ones(9, dtype=torch.uint8))              # wrong length


def test_cpu_tensors_are_refused():
    import torch
    from otto_amd import _lib
    from otto_amd.matrix_factorization.neighbours import neighbour_table, neighbour_table_from_model
    with pytest.raises(_lib.OttoError, match='no CPU fallback'):
        neighbour_table(torch.zeros((10, 32), dtype=torch.float32))
    with pytest.raises(_lib.OttoError, match='no CPU fallback'):
        neighbour_table_from_model({'aid_embeddings.weight': torch.zeros((10, 32)), 'session_embeddings.weight': torch.zeros((4, 32))})


def test_item_table_picks_the_item_embeddings_of_every_model():
    import torch
    from otto_amd.matrix_factorization.neighbours import item_table
    from otto_amd.matrix_factorization.torch_modules import CollaborativeFiltering, MatrixFactorization
    cf = CollaborativeFiltering(n_embeddings=7, n_factors=8)
    mf = MatrixFactorization(n_sessions=5, n_aids=7, n_factors=8)
    assert item_table(cf).data_ptr() == cf.embeddings.weight.data_ptr()
    assert item_table(mf.state_dict()).shape == (7, 8)
    assert item_table({'user_embedding.weight': torch.zeros(3, 8), 'item_embedding.weight': torch.ones(7, 8)}).sum() == 56
    with pytest.raises(ValueError):
        item_table({'something.else': torch.zeros(1)})


@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_rank_split_covers_every_query_aid_once(world):
    import torch
    from otto_amd.matrix_factorization.neighbours import split_rows
    for n_aids in (1, 5, 8, 1001):
        parts = [split_rows(n_aids, r, world) for r in range(world)]
        assert all(p.dtype == torch.int32 for p in parts)
        assert torch.cat(parts).tolist() == list(range(n_aids))
        assert max(p.numel() for p in parts) - min(p.numel() for p in parts) <= 1
    rows = torch.tensor([9, 2, 7, 7, 0, 4, 11], dtype=torch.int32)
    assert torch.cat([split_rows(12, r, world, rows=rows) for r in range(world)]).tolist() == rows.tolist()
    with pytest.raises(ValueError):
        split_rows(10, world, world)


# ---- the inputs of the GPU parity tests ----------------------------------------------------------------------------------

@pytest.mark.parametrize('d,N,ks,mode', list(kr.parity_cases()))
def test_restatement_near_tie_share_of_the_gpu_inputs(d, N, ks, mode):
    """Consecutive float64 keys of the restatement's own top k + 1 closer than tau: at most 1 % of the positions of
    every GPU parity input, so the parity test cannot pass by hiding behind its band."""
    E, valid, rows = kr.parity_case(d, N, mode)
    q = np.arange(N) if rows is None else rows
    for metric in kr.METRIC_NAMES:
        _, _, _, keys, ids_x = kr.knn(E, max(ks), metric, valid=valid, rows=rows, extra=1)
        for k in ks:
            share = kr.close_positions(E, metric, q, ids_x, keys, k).mean()
            print(f'd={d} N={N} {mode} {metric} k={k}: near-tie share {100 * share:.3f} %')
            assert share <= kr.MAX_NEAR_TIE_SHARE, (metric, k, share)
