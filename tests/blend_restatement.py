"""Plain NumPy restatement of SPEC-BLEND (include/otto_blend.h) for the tests.

Everything the device computes is exact, so the tests compare bit for bit (zeros sign-blind where the spec says so).
``prediction_fma`` is NOT the spec: it evaluates the weighted sum with a fused multiply-add and exists only to prove that
a test input can tell the two apart.
"""
import numpy as np

TINY = 10 * np.finfo(np.float64).eps
CLICK_WEIGHTS = (0.05, 0.05, 0.70, 0.20)           # gunes lightgbm, gunes xgboost, tetsuro, anil: the join order
CART_WEIGHTS = (0.05, 0.05, 0.05, 0.70, 0.15)


def stat_ranks(nv):
    """The six integer ranks: median low / high, 25th low / high, 75th low / high."""
    nv = int(nv)
    out = [(nv - 1) >> 1, nv >> 1]
    for num in (1, 3):
        p = num * (nv - 1)
        lo = p >> 2
        out += [lo, min(lo + 1, nv - 1)]
    return out


def _lerp(a, b, t):
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    if b == a:
        return a
    d = b - a
    if t >= 0.5:
        return b - d * (np.float64(1.0) - t)
    return a + d * t


def center_scale(nv, stats):
    """center and scale from nv and the six selected values (the host half of robust scaling)."""
    s = [np.float64(v) for v in stats]
    nv = int(nv)
    center = s[1] if nv & 1 else (s[0] + s[1]) / np.float64(2.0)
    q = []
    for i, num in enumerate((1, 3)):
        p = num * (nv - 1)
        q.append(_lerp(s[2 + 2 * i], s[3 + 2 * i], (p & 3) / 4.0))
    scale = q[1] - q[0]
    if scale < TINY:
        scale = np.float64(1.0)
    return np.float64(center), np.float64(scale)


def robust_stats(x):
    """(nv, the six order statistics float64 [6]); ValueError where the spec refuses."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        raise ValueError('empty column')
    if np.isinf(x).any():
        raise ValueError('infinite value')
    v = np.sort(x[~np.isnan(x)])
    if v.size == 0:
        raise ValueError('all NaN')
    return int(v.size), v[np.array(stat_ranks(v.size))]


def robust_scale(x):
    """(scaled float32, center, scale) of a float64 column."""
    x = np.asarray(x, dtype=np.float64)
    nv, stats = robust_stats(x)
    center, scale = center_scale(nv, stats)
    with np.errstate(invalid='ignore'):
        return ((x - center) / scale).astype(np.float32), center, scale


def join(models, left_of_base=None):
    """models: list of (session int32, aid int32, score float32). Returns (session int64 [R], aid int64 [R],
    cols float32 [M, R] zero-filled) in ascending (session, aid) order; ValueError for a negative id or a key twice in
    one model."""
    M = len(models)
    left = [False] * M if left_of_base is None else [bool(f) for f in left_of_base]
    assert not left[0]
    keys = []
    for s, a, _ in models:
        s, a = np.asarray(s, dtype=np.int64), np.asarray(a, dtype=np.int64)
        if (s < 0).any() or (a < 0).any():
            raise ValueError('negative id')
        k = (s << 32) | a
        if np.unique(k).size != k.size:
            raise ValueError('duplicate key inside a model')
        keys.append(k)
    parts = [keys[m] for m in range(M) if not left[m]]
    out = np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
    base = np.isin(out, keys[0])
    cols = np.zeros((M, out.size), dtype=np.float32)
    for m in range(M):
        pos = np.searchsorted(out, keys[m])
        ok = pos < out.size
        ok[ok] = out[pos[ok]] == keys[m][ok]
        if left[m]:
            ok[ok] = base[pos[ok]]
        cols[m, pos[ok]] = np.asarray(models[m][2], dtype=np.float32)[ok]
    return out >> 32, out & 0xFFFFFFFF, cols


def prediction(cols, weights):
    """((s_0 w_0 + s_1 w_1) + s_2 w_2) + ... with every product and every sum rounded to float32."""
    cols = np.asarray(cols, dtype=np.float32)
    w = [np.float32(x) for x in weights]
    with np.errstate(invalid='ignore', over='ignore'):
        p = cols[0] * w[0]
        for m in range(1, len(w)):
            p = (p + (cols[m] * w[m]).astype(np.float32)).astype(np.float32)
    return p.astype(np.float32)


def prediction_fma(cols, weights):
    """NOT the spec: p = fma(s_m, w_m, p), emulated in float64 (the float32 product is exact there; the one float64
    rounding of the sum before the float32 rounding is the emulation's only liberty)."""
    cols = np.asarray(cols, dtype=np.float32)
    w = [np.float32(x) for x in weights]
    p = cols[0] * w[0]
    for m in range(1, len(w)):
        p = (cols[m].astype(np.float64) * np.float64(w[m]) + p.astype(np.float64)).astype(np.float32)
    return p


def sessions_csr(session):
    """(distinct sessions, row_off int64 [S+1]) of an ascending session column."""
    session = np.asarray(session, dtype=np.int64)
    sid, first = np.unique(session, return_index=True)
    return sid, np.concatenate([first, [session.size]]).astype(np.int64)


def blend(models, weights, left_of_base=None):
    """(session_id, row_off, aid, pred float32) of the joined, weighted models (scores already scaled)."""
    s, a, cols = join(models, left_of_base)
    sid, off = sessions_csr(s)
    return sid, off, a, prediction(cols, weights)


def topk(sid, row_off, aid, pred, k):
    """Per session by (pred descending, aid ascending), NaN last, zeros tie: (top_aid int32 [S, k] -1 padded, n)."""
    S = len(sid)
    top = np.full((S, k), -1, dtype=np.int32)
    n = np.zeros(S, dtype=np.int32)
    for j in range(S):
        lo, hi = int(row_off[j]), int(row_off[j + 1])
        p = pred[lo:hi].astype(np.float64)
        nan = np.isnan(p)
        order = np.lexsort((np.arange(hi - lo), np.where(nan, 0.0, -p) + 0.0, nan))
        order = order[:k]
        top[j, :order.size] = aid[lo:hi][order]
        n[j] = order.size
    return top, n


def same_bits(a, b):
    """Bit-equal arrays of one float dtype, except that -0.0 and +0.0 compare equal (NaN equals NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    za, zb = np.where(a == 0, 0, a).astype(a.dtype), np.where(b == 0, 0, b).astype(b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(za.view(u)[~na], zb.view(u)[~nb]))
