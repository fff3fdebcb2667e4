"""Label assembly on the device (SPEC-LABELS, include/otto_labels.h; otto_amd/ranker/evaluate.py): ``assemble_labels`` against
the NumPy restatement (tests/pqlist_restatement.py) at every session-list size around the 64-lane waves, its refusals naming
the smallest offending row, ``read_labels`` end to end against the pandas chain of the reference on a ``DataFrame.to_parquet``
file in the shape of ``val_labels.parquet``, the same recall through ``evaluate.evaluate`` as host-built lists, and the calling
contract (side stream with late inputs, reused scratch after a larger job)."""
import numpy as np
import pytest
import torch

import pqlist_inputs as I
import pqlist_restatement as R
from test_labels_cpu import SIZES, csr, refusal_edits

pytestmark = pytest.mark.gpu
N_AIDS = 5000


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _inputs(S, seed=None, keep_every=1):
    ids, sess, typ, lists = I.label_rows(S, seed=S if seed is None else seed)
    return (sess, typ, *csr(lists)), ids[::keep_every].astype(np.int32), (sess, typ, lists)


def _run(dev, rows, ids, n_aids=N_AIDS, work=None):
    from otto_amd.ranker import evaluate
    sess, typ, off, value, null = rows
    return evaluate.assemble_labels(_dev(sess, dev), _dev(typ, dev), _dev(off, dev), _dev(value, dev), _dev(null, dev), _dev(ids, dev),
                                    n_aids, work=work)


def _same(got, want):
    labels, dropped = got
    assert dropped == want[1]
    for name, (wo, wa) in zip(('clicks', 'carts', 'orders'), want[0]):
        go, ga = labels[name]
        assert go.dtype == torch.int64 and ga.dtype == torch.int32
        assert np.array_equal(go.cpu().numpy(), wo) and np.array_equal(ga.cpu().numpy(), wa), name


@pytest.mark.parametrize('S', SIZES)
def test_assemble_equals_the_restatement(gpu_device, S):
    for keep_every in (1, 2):
        rows, ids, _ = _inputs(S, keep_every=keep_every)
        want = R.labels_assemble(*rows, ids, N_AIDS)
        assert keep_every == 1 or S < 2 or want[1] > 0                         # rows of sessions outside the list: dropped and counted
        _same(_run(gpu_device, rows, ids), want)


def test_null_empty_and_missing_rows(gpu_device):
    sess = np.array([5, 5, 7, 9], dtype=np.int64)
    typ = np.array([0, 1, 1, 2], dtype=np.uint8)
    off = np.array([0, 1, 1, 1, 3], dtype=np.int64)
    value = np.array([4, 8, 8], dtype=np.int64)
    null = np.array([0, 1, 0, 0], dtype=np.uint8)
    for ids in ([5, 6, 7], [9], [], [1, 2, 3]):
        ids = np.array(ids, dtype=np.int32)
        _same(_run(gpu_device, (sess, typ, off, value, null), ids, 10), R.labels_assemble(sess, typ, off, value, null, ids, 10))
    none = (sess[:0], typ[:0], off[:1], value[:0], null[:0])
    _same(_run(gpu_device, none, np.array([1, 2], dtype=np.int32), 10), R.labels_assemble(*none, [1, 2], 10))


def test_refusals_name_the_smallest_offending_row(gpu_device):
    from otto_amd import _lib
    rows, ids, _ = _inputs(65, seed=1)
    sess, typ, off, value, null = rows
    for name, edit, row, code in refusal_edits(sess, typ, off, value):
        s, t, v = sess.copy(), typ.copy(), value.copy()
        edit(s, t, v)
        with pytest.raises(_lib.OttoError) as e:
            _run(gpu_device, (s, t, off, v, null), ids)
        assert f'row {row}: {R.LABEL_REASONS[code]}' in str(e.value), (name, str(e.value))
    _same(_run(gpu_device, rows, ids), R.labels_assemble(*rows, ids, N_AIDS))    # the clean rows still pass
    with pytest.raises(_lib.OttoError, match='ROCm'):
        from otto_amd.ranker import evaluate
        evaluate.assemble_labels(*[torch.from_numpy(a) for a in rows], torch.from_numpy(ids), N_AIDS)


@pytest.fixture(scope='module')
def label_file(tmp_path_factory):
    ids, sess, typ, lists = I.label_rows(3000, seed=11, n_aids=N_AIDS)
    frame = I.label_frame(sess, typ, lists)
    path = str(tmp_path_factory.mktemp('labels') / 'val_labels.parquet')
    frame.to_parquet(path)
    return path, frame, ids


def test_read_labels_equals_the_pandas_chain(gpu_device, label_file):
    from otto_amd import _lib
    from otto_amd.ranker import evaluate
    path, frame, ids = label_file
    present = np.unique(frame['session'].to_numpy())
    session, labels, dropped = evaluate.read_labels(path, gpu_device)
    assert session.dtype == torch.int32 and np.array_equal(session.cpu().numpy(), present) and dropped == 0
    _same((labels, dropped), (R.labels_reference(frame, present), 0))
    keep = ids[::3].astype(np.int32)                                             # the caller's own session list, with sessions the file lacks
    session, labels, dropped = evaluate.read_labels(path, gpu_device, session=_dev(keep, gpu_device), n_aids=N_AIDS)
    _same((labels, dropped), (R.labels_reference(frame, keep), int((~np.isin(frame['session'].to_numpy(), keep)).sum())))
    with pytest.raises(_lib.OttoError, match=r'a value outside \[0, n_aids\)'):
        evaluate.read_labels(path, gpu_device, n_aids=10)


def test_recall_through_evaluate_equals_host_built_lists(gpu_device, label_file):
    """the chain: read_labels -> evaluate.evaluate gives the recall of label lists built on the host with np.cumsum"""
    from otto_amd.ranker import evaluate
    path, frame, ids = label_file
    present = np.unique(frame['session'].to_numpy())
    session, labels, _ = evaluate.read_labels(path, gpu_device)
    host = {name: (_dev(o, gpu_device), _dev(a, gpu_device)) for name, (o, a) in zip(evaluate.TYPES, R.labels_reference(frame, present))}
    rng = np.random.default_rng(0)
    preds = {}
    for name in evaluate.TYPES:                                                   # half the rows hold one of the session's labels
        p = rng.integers(0, N_AIDS, size=(len(present), 20)).astype(np.int32)
        o, a = host[name][0].cpu().numpy(), host[name][1].cpu().numpy()
        for s in range(0, len(present), 2):
            if o[s + 1] > o[s]:
                p[s, 3] = a[o[s]]
        preds[name] = _dev(p, gpu_device)
    got = evaluate.evaluate(preds, labels, label_session=session)
    want = evaluate.evaluate(preds, host, label_session=_dev(present.astype(np.int32), gpu_device))
    assert got == want
    # the comparison is over something: every second session has its one click label among its predictions, chance adds 20 / N_AIDS
    assert 0.4 < got['clicks'] < 0.6 and 0 < got['carts'] < 1 and 0 < got['orders'] < 1


# ---- the calling contract -------------------------------------------------------------------------------------------------------
def test_reused_scratch_after_a_larger_job(gpu_device):
    (real, ids, _), (decoy, ids_d, _), (large, ids_l, _) = _inputs(1000, seed=1), _inputs(1000, seed=2), _inputs(2500, seed=3)
    want = R.labels_assemble(*real, ids, N_AIDS)
    work = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    for rows, i, w in ((real, ids, want), (real, ids, want), (decoy, ids_d, None), (real, ids, want), (large, ids_l, None), (real, ids, want)):
        _same(_run(gpu_device, rows, i, work=work), w or R.labels_assemble(*rows, i, N_AIDS))


def test_side_stream_with_late_inputs(gpu_device):
    """The inputs hold a decoy; on a side stream a delay is followed by the copies of the real rows and by the call."""
    from otto_amd.ranker import evaluate
    dev = gpu_device
    real, ids, _ = _inputs(1000, seed=1)
    n, v = len(real[0]), len(real[3])
    rng = np.random.default_rng(9)
    decoy = (rng.permutation(real[0]), real[1], np.r_[0, np.sort(rng.integers(0, v + 1, size=n - 1)), v].astype(np.int64),
             rng.integers(0, N_AIDS, size=v), real[4])
    want = R.labels_assemble(*real, ids, N_AIDS)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(20_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(30.0 * 20_000_000 / t0.elapsed_time(t1))                         # about 30 ms
    d_in = [_dev(a, dev) for a in decoy]
    d_ids = _dev(ids, dev)
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in real]
    work = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record(side)
        torch.cuda._sleep(cycles)
        e1.record(side)
        for t, p in zip(d_in, pinned):
            t.copy_(p, non_blocking=True)
        got = evaluate.assemble_labels(*d_in, d_ids, N_AIDS, work=work)
    side.synchronize()
    assert e0.elapsed_time(e1) >= 10.0
    _same(got, want)
