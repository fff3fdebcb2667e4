"""NumPy restatement of SPEC-TFIDF (include/otto_tfidf.h): explicit Python loops wherever the order of the floating-point
operations is part of the result. Test infrastructure, not product."""
import numpy as np

MAX_K = 64
RECENCY_CURVE = (0.1, 1.0)
TYPE_COEFFICIENT = {0: 1, 1: 6, 2: 3}


class Refused(Exception):
    def __init__(self, index):
        super().__init__(f'index {index}')
        self.index = index


def count(tok_aid, doc_off, n_aids, min_aid):
    """-> (row_off int64 [D + 1], col int32, tf int32, df int32 [n_aids])"""
    tok_aid = np.asarray(tok_aid)
    bad = np.flatnonzero((tok_aid < 0) | (tok_aid >= n_aids))
    if bad.size:
        raise Refused(int(bad[0]))
    D = len(doc_off) - 1
    row_off, col, tf = [0], [], []
    df = np.zeros(n_aids, dtype=np.int32)
    for d in range(D):
        doc = tok_aid[int(doc_off[d]):int(doc_off[d + 1])]
        aids, counts = np.unique(doc[doc >= min_aid], return_counts=True)
        col += aids.tolist()
        tf += counts.tolist()
        df[aids] += 1
        row_off.append(len(col))
    return np.array(row_off, dtype=np.int64), np.array(col, dtype=np.int32), np.array(tf, dtype=np.int32), df


def smooth_idf(df, n_docs):
    return np.log((1.0 + n_docs) / (1.0 + df.astype(np.float64))) + 1.0


def _normalized(w):
    ss = np.float64(0.0)
    for x in w:                                  # column order
        ss = ss + x * x
    norm = np.sqrt(ss)
    return [x / norm if norm > 0.0 else np.float64(0.0) for x in w]


def weights(row_off, col, tf, idf):
    val = np.zeros(len(col), dtype=np.float64)
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        val[b:e] = _normalized([np.float64(tf[i]) * np.float64(idf[col[i]]) for i in range(b, e)])
    return val


def normalize_rows(row_off, val):
    out = np.zeros(len(val), dtype=np.float64)
    for r in range(len(row_off) - 1):
        b, e = int(row_off[r]), int(row_off[r + 1])
        out[b:e] = _normalized([np.float64(val[i]) for i in range(b, e)])
    return out


def fit_transform(tok_aid, doc_off, n_aids, min_aid=10):
    """-> (row_off, col, val) and the dict of the intermediate arrays"""
    row_off, col, tf, df = count(tok_aid, doc_off, n_aids, min_aid)
    idf = smooth_idf(df, len(doc_off) - 1)
    return (row_off, col, weights(row_off, col, tf, idf)), {'tf': tf, 'df': df, 'idf': idf}


def transpose(off, idx, val, n_cols):
    """CSR of the transpose, indices ascending inside each row, values bit-copied"""
    R = len(off) - 1
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(off))
    order = np.lexsort((rows, idx))              # by column, then by row
    t_off = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(idx, dtype=np.int64), minlength=n_cols), out=t_off[1:])
    return t_off, rows[order].astype(np.int32), np.asarray(val, dtype=np.float64)[order]


def similarities(a, at, q):
    """{j: s(q, j)} over every row j that shares a column with q, summed in ascending column order"""
    a_off, a_idx, a_val = a
    t_off, t_idx, t_val = at
    s = {}
    for p in range(int(a_off[q]), int(a_off[q + 1])):        # q's columns ascend
        c, v = int(a_idx[p]), np.float64(a_val[p])
        for pp in range(int(t_off[c]), int(t_off[c + 1])):
            j = int(t_idx[pp])
            s[j] = s.get(j, np.float64(0.0)) + v * np.float64(t_val[pp])
    return s


def cosine_topk(a, at, queries, k, exclude_self=True):
    """-> (ids int32 [nq, k] padded -1, sim float64 [nq, k] padded 0, n int32 [nq], first refused query position or -1)"""
    assert 1 <= k <= MAX_K
    R = len(a[0]) - 1
    nq = len(queries)
    ids = np.full((nq, k), -1, dtype=np.int32)
    sim = np.zeros((nq, k), dtype=np.float64)
    n = np.zeros(nq, dtype=np.int32)
    refused = -1
    for qi, q in enumerate(queries):
        q = int(q)
        if not 0 <= q < R:
            refused = qi if refused < 0 else refused
            continue
        kept = [(j, s) for j, s in similarities(a, at, q).items() if s > 0.0 and not (exclude_self and j == q)]
        kept.sort(key=lambda e: (-e[1], e[0]))
        kept = kept[:k]
        n[qi] = len(kept)
        ids[qi, :len(kept)] = [j for j, _ in kept]
        sim[qi, :len(kept)] = [s for _, s in kept]
    return ids, sim, n, refused


def aid_matrices(m, n_rows_of_t):
    """(A, AT) of the aid direction from the session matrix m = (row_off, col, val) with n_rows_of_t = n_aids columns"""
    t_off, t_idx, t_val = transpose(*m, n_rows_of_t)
    a = (t_off, t_idx, normalize_rows(t_off, t_val))
    return a, transpose(*a, len(m[0]) - 1)


def recency_list(session_aids, session_types, n_pred):
    """src/tfidf/inference.py:63-75 through the oracle's session_recency (Counter.most_common = the script's stable sort)"""
    import recency_oracle as ro
    (aids, _), = ro.session_recency(session_aids, session_types, curves=(RECENCY_CURVE,), coef=TYPE_COEFFICIENT)
    return aids[:n_pred]


def predictions(aid, typ, sess_off, n_aids, n_similar=49, n_pred=20, min_unique=20, min_aid=10, matrices=None):
    """-> (pred int32 [S, n_pred] padded -1, n int32 [S], recency bool [S]). ``matrices``: the aid direction's (A, AT) to use
    instead of the restated ones (the GPU test feeds the device's)."""
    S = len(sess_off) - 1
    if matrices is None:
        m, _ = fit_transform(aid, sess_off, n_aids, min_aid)
        matrices = aid_matrices(m, n_aids)
    a, at = matrices
    pred = np.full((S, n_pred), -1, dtype=np.int32)
    n = np.zeros(S, dtype=np.int32)
    recency = np.zeros(S, dtype=bool)
    for s in range(S):
        b, e = int(sess_off[s]), int(sess_off[s + 1])
        session_aids = np.asarray(aid[b:e])
        unique = np.unique(session_aids).tolist()
        if len(unique) >= min_unique:
            recency[s] = True
            row = recency_list(session_aids, typ[b:e], n_pred)
        elif e > b:
            ids, _, cnt, _ = cosine_topk(a, at, [int(session_aids[-1])], n_similar, exclude_self=True)
            row = (unique + ids[0, :cnt[0]].tolist())[:n_pred]
        else:
            row = []
        pred[s, :len(row)] = row
        n[s] = len(row)
    return pred, n, recency
