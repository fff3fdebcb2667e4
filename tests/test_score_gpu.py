"""Full-sort scoring + top-k (``otto_mf_score_topk``) and the list merge (``otto_mf_topk_merge``) of csrc/otto_mf.hip over a
pairwise cover of d x k x B x N x pad_col (``edge_inputs.score_cases``), with two kinds of input:

* exact-arithmetic inputs (integers in [-4, 4]): fp32 is exact in any order, scores tie massively, and ids AND scores must
  equal ``mf_oracle.score_topk`` bit for bit -- this pins (score desc, id asc) across item tiles, lane halves, splits and the
  merge at every d;
* random float inputs: no tolerance constant; every returned score is within the forward error bound of an fp32 dot product
  of its float64 value, and no item left out could have belonged in the list by more than the two bounds involved.
"""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as ei
import mf_oracle as mo

pytestmark = pytest.mark.gpu

CASES = ei.score_cases()
SHORT = [(8, 32, 33, 1, 'none'), (16, 2, 5, 1, 'last'), (32, 20, 129, 19, 'none'), (64, 20, 32, 20, 'first'), (128, 32, 31, 31, 'mid'),
         (16, 32, 128, 32, 'last'), (16, 31, 1, 33, 'none')]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, U, V, k, pad):
    from otto_amd.matrix_factorization.engine import score_topk
    ids, sc = score_topk(_t(U, dev), _t(V, dev), k=k, pad_col=pad)
    return ids.cpu().numpy(), sc.cpu().numpy()


def _id(c):
    return 'd{}-k{}-B{}-N{}-{}'.format(*c)


def _exact(dev, d, k, B, N, padkind):
    pad = ei.pad_col_of(padkind, B, N)
    U, V = ei.exact_inputs(B, N, d, seed=1)
    ids, sc = _run(dev, U, V, k, pad)
    wi, ws = ei.topk_padded(mo.score_topk, U, V, k, pad)
    assert np.array_equal(ids, wi), 'ids differ from the oracle'
    assert np.array_equal(sc.astype(np.float64), ws), 'scores differ from the oracle'
    return ids, sc


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_exact_arithmetic_inputs_equal_the_oracle_bit_for_bit(gpu_device, case):
    _exact(gpu_device, *case)


@pytest.mark.parametrize('case', SHORT, ids=_id)
def test_rows_with_fewer_than_k_valid_items_end_in_minus_one_and_minus_inf(gpu_device, case):
    """N < k, N = 1, N = k - 1, N = k with a masked column: the tail of the row holds id -1 and score -inf
    (include/otto_mf.h). The oracle cannot express this; ``edge_inputs.topk_padded`` pads its output."""
    d, k, B, N, padkind = case
    ids, sc = _exact(gpu_device, *case)
    valid = N - (ei.pad_col_of(padkind, B, N) >= 0)
    if valid < k:
        assert (ids[:, valid:] == -1).all() and np.isneginf(sc[:, valid:]).all() and (ids[:, :valid] >= 0).all()
    U, V = ei.float_inputs(B, N, d, seed=2)
    _check_float(U, V, k, ei.pad_col_of(padkind, B, N), *_run(gpu_device, U, V, k, ei.pad_col_of(padkind, B, N)))


def _check_float(U, V, k, pad, ids, sc):
    B, N = U.shape[0], V.shape[0]
    S64, bound = ei.dot_bound(U, V)
    valid = np.ones(N, dtype=bool)
    if pad >= 0:
        valid[pad] = False
    n_valid = min(k, int(valid.sum()))
    assert (ids[:, n_valid:] == -1).all() and np.isneginf(sc[:, n_valid:]).all()
    ids, sc = ids[:, :n_valid], sc[:, :n_valid].astype(np.float64)
    if n_valid == 0:
        return
    assert (ids >= 0).all() and (ids < N).all() and (ids != pad).all()
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), 'an id is returned twice'
    assert (sc[:, 1:] <= sc[:, :-1]).all(), 'scores increase along a row'
    rows = np.arange(B)[:, None]
    err = np.abs(sc - S64[rows, ids])
    over = err - bound[rows, ids]
    assert (over <= 0).all(), f'score off by {err.max():.3e}, {over.max():.3e} beyond the dot-product bound'
    # selection: nothing left out beats the weakest returned item by more than the two bounds
    floor = (S64[rows, ids] + bound[rows, ids]).min(axis=1)
    out = np.broadcast_to(valid, (B, N)).copy()
    out[rows, ids] = False
    excess = np.where(out, S64 - bound - floor[:, None], -np.inf)
    assert (excess <= 0).all(), f'an item left out beats the list by {excess.max():.3e} beyond the bounds'


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_random_float_inputs_within_the_dot_product_bound(gpu_device, case):
    d, k, B, N, padkind = case
    pad = ei.pad_col_of(padkind, B, N)
    U, V = ei.float_inputs(B, N, d, seed=3)
    _check_float(U, V, k, pad, *_run(gpu_device, U, V, k, pad))


@pytest.mark.parametrize('k', [1, 20, 32])
@pytest.mark.parametrize('B', [1, 130])
@pytest.mark.parametrize('n_lists', [1, 2, 5])
def test_topk_merge_against_a_lexsort_of_the_union(gpu_device, n_lists, B, k):
    """Lists with empty slots written both ways the header allows (-1 and 0x7FFFFFFF), wholly empty lists, equal scores
    with different ids across lists."""
    from otto_amd.matrix_factorization.engine import topk_merge
    ps, pi = ei.merge_lists(n_lists, B, k, seed=4)
    ids, sc = topk_merge(_t(ps, gpu_device), _t(pi, gpu_device), k)
    wi, ws = ei.merge_reference(ps, pi, k)
    assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(sc.cpu().numpy(), ws)


def test_scoring_argument_errors(gpu_device):
    import torch
    from otto_amd import _lib
    lib = _lib.lib()
    B, N = 8, 64
    U = torch.zeros((B, 256), dtype=torch.float32, device=gpu_device)
    V = torch.zeros((N, 256), dtype=torch.float32, device=gpu_device)
    ids = torch.empty((B, 64), dtype=torch.int32, device=gpu_device)
    sc = torch.empty((B, 64), dtype=torch.float32, device=gpu_device)
    ws_b = int(lib.otto_mf_score_workspace(B, N, 32))
    ws = torch.empty(ws_b, dtype=torch.uint8, device=gpu_device)
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)

    def call(d, k, ws_bytes):
        with torch.cuda.device(gpu_device):
            _lib.check(lib.otto_mf_score_topk(p(U), p(V), B, N, d, k, -1, p(ids), p(sc), p(ws), ws_bytes, stream), 'otto_mf_score_topk')
    for d in (4, 256):                  # valid for the trainer, refused here
        with pytest.raises(_lib.OttoError, match='scoring supports d in'):
            call(d, 20, ws_b)
    for k in (0, 33):
        with pytest.raises(_lib.OttoError, match='k must be in \\[1, 32\\]'):
            call(32, k, ws_b)
    with pytest.raises(_lib.OttoError, match='workspace too small'):
        call(32, 20, int(lib.otto_mf_score_workspace(B, N, 20)) - 1)
    call(32, 20, int(lib.otto_mf_score_workspace(B, N, 20)))
