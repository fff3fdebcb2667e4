"""TF-IDF bag-of-aids vectors of the sessions and the cosine top-k between sparse rows, on the device (SPEC-TFIDF,
``include/otto_tfidf.h``).

Reference code replaced: ``TfidfVectorizer().fit_transform`` over ``' '.join(str(aid))`` and
``cosine_similarity(dense_output=False)`` with its per-row ``argsort`` (``src/tfidf/inference.py:33-37,89-91``). Nothing of
size S x S is ever materialised: a query's similarities are summed, ranked and dropped again inside one kernel.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _lib

MAX_K = 64                                   # OTTO_TFIDF_MAX_K
SMALL_CAP = 512                              # OTTO_TFIDF_SMALL_CAP: the candidate bound up to which a query runs in the LDS tier
MAX_GROUPS = 128                             # OTTO_TFIDF_MAX_GROUPS
SMALL_GRID = 1024                            # OTTO_TFIDF_SMALL_GRID: workgroups of four queries the small tier launches at most
SKLEARN_MIN_AID = 10                         # the default token_pattern drops one-character tokens: aids 0..9

# TfidfVectorizer arguments and the only value of each that is built
_VECTORIZER_DEFAULTS = {'sublinear_tf': False, 'norm': 'l2', 'use_idf': True, 'smooth_idf': True, 'max_df': 1.0, 'min_df': 1,
                        'max_features': None, 'ngram_range': (1, 1), 'binary': False, 'analyzer': 'word', 'vocabulary': None,
                        'stop_words': None}


def resolve_vectorizer(params=None):
    """``TfidfVectorizer`` keyword arguments -> ``min_aid``. Every argument that changes the arithmetic must have
    scikit-learn's default (``ValueError`` naming it otherwise): ``sublinear_tf``, ``norm='l1'``, ``use_idf=False``,
    ``max_df`` / ``min_df`` / ``max_features`` and n-grams are not built. ``token_pattern``: the default drops aids 0..9
    (``min_aid = 10``); ``r'(?u)\\b\\w+\\b'`` keeps every aid (``min_aid = 0``)."""
    params = dict(params or {})
    pattern = params.pop('token_pattern', r'(?u)\b\w\w+\b')
    if pattern == r'(?u)\b\w\w+\b':
        min_aid = SKLEARN_MIN_AID
    elif pattern == r'(?u)\b\w+\b':
        min_aid = 0
    else:
        raise ValueError(f'token_pattern = {pattern!r} is not built')
    for key, val in params.items():
        if key not in _VECTORIZER_DEFAULTS:
            raise ValueError(f'{key}: unknown TfidfVectorizer argument')
        want = _VECTORIZER_DEFAULTS[key]
        if (tuple(val) if key == 'ngram_range' else val) != want:
            raise ValueError(f'{key} = {val!r} is not built (only {want!r})')
    return min_aid


@dataclass
class TfidfMatrix:
    """CSR float64 matrix on the device: ``row_off`` int64 [n_rows + 1], ``col`` int32 [nnz] ascending inside each row,
    ``val`` float64 [nnz]. ``tf`` int32 [nnz], ``df`` int32 [n_cols] and ``idf`` float64 [n_cols] are those of the fit
    (None on a transpose)."""
    row_off: object
    col: object
    val: object
    n_rows: int
    n_cols: int
    tf: object = None
    df: object = None
    idf: object = None

    @property
    def nnz(self):
        return int(self.col.numel())


def _scratch_for(job, name, dev, work):
    """the scratch of ``job``: sized by entry point ``name``, a fresh tensor unless ``work`` is given"""
    import torch
    need = int(getattr(_lib.lib(), name)(C.byref(job)))
    if need < 0:
        _lib.check(need, name)
    if work is None:
        work = _lib.workspace(need, dev)
    elif _lib.need(work, 'work', torch.uint8, 1, device=dev).numel() < need:
        raise ValueError(f'work: {work.numel()} bytes, {need} are needed')
    job.d_work, job.work_bytes = _lib.ptr(work, dev), int(work.numel())
    return work


def count(aid, sess_off, n_aids, min_aid=SKLEARN_MIN_AID, work=None):
    """SPEC-TFIDF COUNT + FILL: tokens ``aid`` int32 [E] of the documents ``sess_off`` int64 [D + 1] -> ``(row_off int64
    [D + 1], col int32 [nnz], tf int32 [nnz], df int32 [n_aids])``; aids below ``min_aid`` are dropped. ``OttoError`` naming
    the first token whose aid lies outside ``[0, n_aids)``."""
    import torch
    dev = aid.device if isinstance(aid, torch.Tensor) else None
    if dev is None or dev.type != 'cuda':
        raise _lib.OttoError('tfidf.count needs tensors on a ROCm device (no CPU fallback)')
    _lib.need(aid, 'aid', torch.int32, 1, device=dev)
    _lib.need(sess_off, 'sess_off', torch.int64, 1, device=dev)
    n_aids, min_aid = int(n_aids), int(min_aid)
    if sess_off.numel() < 1:
        raise ValueError('sess_off: at least one offset')
    if not 0 <= n_aids < 1 << 31:
        raise ValueError(f'n_aids must be in [0, 2^31) (got {n_aids})')
    if min_aid < 0:
        raise ValueError(f'min_aid must not be negative (got {min_aid})')
    E, D = int(aid.numel()), int(sess_off.numel()) - 1
    with torch.cuda.device(dev):
        row_off = torch.empty(D + 1, dtype=torch.int64, device=dev)
        df = torch.empty(n_aids, dtype=torch.int32, device=dev)
        job = _lib.TfidfFitJob(_lib.ptr(aid, dev), _lib.ptr(sess_off, dev), E, D, n_aids, min_aid, 0, _lib.ptr(row_off, dev),
                               _lib.ptr(df, dev), None, None, 0, None, 0, _lib.stream(dev))
        work = _scratch_for(job, 'otto_tfidf_fit_workspace', dev, work)
        nnz, err = np.zeros(1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
        try:
            _lib.call('otto_tfidf_count', dev, C.byref(job), nnz, err, stream=False)
        except _lib.OttoError:
            if err[0] < 0:
                raise
            raise _lib.OttoError(f'tfidf.count: token {int(err[0])}: aid outside [0, {n_aids})') from None
        col = torch.empty(int(nnz[0]), dtype=torch.int32, device=dev)
        tf = torch.empty(int(nnz[0]), dtype=torch.int32, device=dev)
        job.d_col, job.d_tf, job.nnz = _lib.ptr(col, dev), _lib.ptr(tf, dev), int(nnz[0])
        _lib.call('otto_tfidf_fill', dev, C.byref(job), stream=False)
    return row_off, col, tf, df


def smooth_idf(df, n_docs):
    """``log((1 + D) / (1 + df)) + 1`` in float64 with NumPy on the host (scikit-learn's smooth idf; one libm for the
    product and for the restatement). ``df``: NumPy int array."""
    return np.log((1.0 + n_docs) / (1.0 + df.astype(np.float64))) + 1.0


def _weights(row_off, col, tf, idf, val, n_rows, n_cols, dev):
    import torch
    with torch.cuda.device(dev):
        job = _lib.TfidfWeightsJob(_lib.ptr(row_off, dev), _lib.ptr(col, dev), _lib.ptr(tf, dev), _lib.ptr(idf, dev), _lib.ptr(val, dev),
                                   n_rows, n_cols, _lib.stream(dev))
        _lib.call('otto_tfidf_weights', dev, C.byref(job), stream=False)


def fit_transform(aid, sess_off, n_aids, min_aid=SKLEARN_MIN_AID, work=None):
    """``TfidfVectorizer().fit_transform`` of the sessions: a :class:`TfidfMatrix` (sessions x aids, l2 rows) with its
    ``tf``, ``df`` and ``idf``. ``min_aid``: :func:`resolve_vectorizer`."""
    import torch
    row_off, col, tf, df = count(aid, sess_off, n_aids, min_aid, work=work)
    dev = aid.device
    D = int(sess_off.numel()) - 1
    idf = torch.from_numpy(smooth_idf(df.cpu().numpy(), D)).to(dev)
    val = torch.empty(col.numel(), dtype=torch.float64, device=dev)
    _weights(row_off, col, tf, idf, val, D, int(n_aids), dev)
    return TfidfMatrix(row_off, col, val, D, int(n_aids), tf=tf, df=df, idf=idf)


def _matrix(m, what):
    import torch
    if not isinstance(m, TfidfMatrix):
        raise ValueError(f'{what}: expected a TfidfMatrix')
    dev = m.row_off.device
    _lib.need(m.row_off, f'{what}.row_off', torch.int64, 1, numel=m.n_rows + 1)
    _lib.need(m.col, f'{what}.col', torch.int32, 1, device=dev)
    _lib.need(m.val, f'{what}.val', torch.float64, 1, device=dev, numel=m.col.numel())
    return dev


def transpose(m, work=None):
    """SPEC-TFIDF TRANSPOSE: the CSR of ``m``'s transpose, indices ascending inside each row, values bit-copied."""
    import torch
    dev = _matrix(m, 'm')
    nnz = m.nnz
    with torch.cuda.device(dev):
        t_off = torch.empty(m.n_cols + 1, dtype=torch.int64, device=dev)
        t_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
        t_val = torch.empty(nnz, dtype=torch.float64, device=dev)
        job = _lib.TfidfTransposeJob(_lib.ptr(m.row_off, dev), _lib.ptr(m.col, dev), _lib.ptr(m.val, dev), m.n_rows, m.n_cols, nnz,
                                     _lib.ptr(t_off, dev), _lib.ptr(t_idx, dev), _lib.ptr(t_val, dev), None, 0, _lib.stream(dev))
        work = _scratch_for(job, 'otto_tfidf_transpose_workspace', dev, work)
        err = np.full(1, -1, dtype=np.int64)
        try:
            _lib.call('otto_tfidf_transpose', dev, C.byref(job), err, stream=False)
        except _lib.OttoError:
            if err[0] < 0:
                raise
            raise _lib.OttoError(f'tfidf.transpose: entry {int(err[0])}: index outside [0, {m.n_cols})') from None
    return TfidfMatrix(t_off, t_idx, t_val, m.n_cols, m.n_rows)


def normalize_rows(m):
    """A copy of ``m`` with every row divided by its l2 norm (SPEC-TFIDF WEIGHTS without idf); zero rows stay zero."""
    dev = _matrix(m, 'm')
    val = m.val.clone()
    _weights(m.row_off, None, None, None, val, m.n_rows, m.n_cols, dev)
    return TfidfMatrix(m.row_off, m.col, val, m.n_rows, m.n_cols)


def cosine_topk(a, at, queries, k=49, exclude_self=True, work=None):
    """SPEC-TFIDF COSINE TOP-K: for every row id of ``queries`` (int32) the ``k`` rows of ``a`` with the largest positive
    cosine, ties to the smaller id -> ``(ids int32 [nq, k] padded -1, sim float64 [nq, k] padded 0, n int32 [nq])``.
    ``at``: :func:`transpose` of ``a``. ``OttoError`` naming the first query outside ``[0, a.n_rows)``."""
    import torch
    dev = _matrix(a, 'a')
    if _matrix(at, 'at') != dev:
        raise ValueError('a and at live on different devices')
    if (at.n_rows, at.n_cols) != (a.n_cols, a.n_rows) or at.nnz != a.nnz:
        raise ValueError(f'at is {at.n_rows} x {at.n_cols} with {at.nnz} entries; the transpose of a is {a.n_cols} x {a.n_rows} with {a.nnz}')
    _lib.need(queries, 'queries', torch.int32, 1, device=dev)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    nq = int(queries.numel())
    with torch.cuda.device(dev):
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        sim = torch.empty((nq, k), dtype=torch.float64, device=dev)
        n = torch.empty(nq, dtype=torch.int32, device=dev)
        job = _lib.TfidfCosineJob(_lib.ptr(a.row_off, dev), _lib.ptr(a.col, dev), _lib.ptr(a.val, dev), _lib.ptr(at.row_off, dev),
                                  _lib.ptr(at.col, dev), _lib.ptr(at.val, dev), a.n_rows, a.n_cols, _lib.ptr(queries, dev), nq, k,
                                  1 if exclude_self else 0, _lib.ptr(ids, dev), _lib.ptr(sim, dev), _lib.ptr(n, dev), None, 0,
                                  _lib.stream(dev))
        work = _scratch_for(job, 'otto_tfidf_cosine_workspace', dev, work)
        err = np.full(1, -1, dtype=np.int64)
        try:
            _lib.call('otto_tfidf_cosine_topk', dev, C.byref(job), err, stream=False)
        except _lib.OttoError:
            if err[0] < 0:
                raise
            raise _lib.OttoError(f'tfidf.cosine_topk: query {int(err[0])}: row id outside [0, {a.n_rows})') from None
    return ids, sim, n


def similar_sessions(m, queries, k=49, mt=None):
    """The ``k`` sessions most similar to each session of ``queries`` (``cosine_similarity(X)`` row by row, self excluded).
    ``mt``: ``transpose(m)`` where the caller has it already."""
    return cosine_topk(m, mt if mt is not None else transpose(m), queries, k, exclude_self=True)


def aid_matrices(m):
    """``(A, AT)`` of the aid direction: ``A = normalize_rows(transpose(m))`` (aids x sessions, unit rows -- the columns of
    the session matrix are not unit vectors) and its transpose."""
    a = normalize_rows(transpose(m))
    return a, transpose(a)


def similar_aids(m, aids, k=49, matrices=None):
    """The ``k`` aids most similar to each aid of ``aids`` over the sessions that hold them (``cosine_similarity(X.T)`` row
    by row, self excluded). ``matrices``: :func:`aid_matrices` of ``m`` where the caller has them already."""
    a, at = matrices if matrices is not None else aid_matrices(m)
    return cosine_topk(a, at, aids, k, exclude_self=True)
