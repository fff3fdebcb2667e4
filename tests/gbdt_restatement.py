"""Plain NumPy float64 / integer restatement of SPEC-GBDT (include/otto_gbdt.h) for the tests.

Written for clarity, not speed: a sequential double loop for the objective, a dense histogram by ``np.add.at``, Python
leaf-wise growth. Every float64 operation is a single NumPy / Python operation, so each rounds once, in the order the
spec pins. The tables come from the same NumPy calls the package makes (``gbdt.sigmoid_table``, ``gbdt.discount_table``
are restated here, not imported).
"""
import numpy as np

MAX_QUERY = 1024
MAX_EDGES = 254
NAN_BIN = 255
SIGMOID_BINS = 1 << 20


# ---- binning

def fit_edges(column, max_bin=255):
    """The edges (float32, strictly increasing) of one feature from its sample column."""
    v = np.sort(column[~np.isnan(column)])
    distinct = np.unique(v)
    if distinct.size <= max_bin:
        return distinct[:-1].astype(np.float32)
    m = v.size
    return np.unique(np.array([v[((i + 1) * m) // max_bin - 1] for i in range(max_bin - 1)], dtype=np.float32))


def bin_column(x, edges):
    """bin(x) = the number of edges < x; NaN -> 255."""
    out = np.searchsorted(edges, x, side='left').astype(np.uint8)
    out[np.isnan(x)] = NAN_BIN
    return out


def bin_rows(X, edge_list):
    """uint8 [F, n] from X float32 [n, >= F] and the per-feature edges."""
    return np.stack([bin_column(X[:, f], e) for f, e in enumerate(edge_list)])


# ---- objective

def sigmoid_table(sigma):
    lo, hi = -25.0 / sigma, 25.0 / sigma
    factor = SIGMOID_BINS / (hi - lo)
    i = np.arange(SIGMOID_BINS, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(sigma * (lo + i / factor))), lo, factor


def discount_table():
    return 1.0 / np.log2(2.0 + np.arange(MAX_QUERY, dtype=np.float64))


_TABLE = {}


def _tables(sigma):
    if sigma not in _TABLE:
        _TABLE[sigma] = sigmoid_table(sigma) + (discount_table(),)
    return _TABLE[sigma]


def rank_order(score):
    """Positions by (score descending, position ascending); -0.0 == +0.0, NaN last."""
    return np.argsort(-score, kind='stable')


def valid_query(query_off, q, n):
    lo, hi = int(query_off[q]), int(query_off[q + 1])
    return 0 <= lo <= hi <= n and hi - lo <= MAX_QUERY


def lambdarank(score, label, query_off, sigma=1.0, truncation_level=30, norm=True):
    """(grad, hess, n_invalid_queries): float64 [n]; the rows of a refused query stay zero."""
    score = np.asarray(score, dtype=np.float64)
    table, t_lo, factor, discount = _tables(float(sigma))
    n = score.size
    grad, hess = np.zeros(n), np.zeros(n)
    invalid = 0
    sigma = np.float64(sigma)
    for q in range(len(query_off) - 1):
        if not valid_query(query_off, q, n):
            invalid += 1
            continue
        lo, hi = int(query_off[q]), int(query_off[q + 1])
        cnt = hi - lo
        if cnt == 0:
            continue
        order = rank_order(score[lo:hi])
        s = score[lo:hi][order]
        lab = np.asarray(label[lo:hi])[order].astype(np.int64)
        gain = (2.0 ** lab - 1.0).astype(np.float64)
        max_dcg = np.float64(0.0)
        for r, g in enumerate(np.sort(gain)[::-1][:truncation_level]):
            max_dcg = max_dcg + g * discount[r]
        inv_max_dcg = 1.0 / max_dcg if max_dcg > 0 else np.float64(0.0)
        best, worst = s[0], s[-1]
        g_q, h_q = np.zeros(cnt), np.zeros(cnt)
        sum_lambdas = np.float64(0.0)
        for i in range(min(truncation_level, cnt)):
            for j in range(i + 1, cnt):
                if lab[i] == lab[j]:
                    continue
                high, low = (i, j) if lab[i] > lab[j] else (j, i)
                d = s[high] - s[low]
                delta = (gain[high] - gain[low]) * abs(discount[i] - discount[j]) * inv_max_dcg
                if norm and best != worst:
                    delta = delta / (0.01 + abs(d))
                x = (d - t_lo) * factor
                p = table[int(min(max(x, 0.0), float(SIGMOID_BINS - 1)))]
                lam = -sigma * delta * p
                eta = sigma * sigma * delta * p * (1.0 - p)
                g_q[high] += lam
                g_q[low] -= lam
                h_q[high] += eta
                h_q[low] += eta
                sum_lambdas = sum_lambdas + -2.0 * lam
        if norm and sum_lambdas > 0:
            f = np.log2(1.0 + sum_lambdas) / sum_lambdas
            g_q, h_q = g_q * f, h_q * f
        grad[lo + order], hess[lo + order] = g_q, h_q
    return grad, hess, invalid


def ap_at_k(score, label, query_off, k):
    """(ap float64 [Q], n_invalid): -1 for a query without a positive (and for a refused query)."""
    score = np.asarray(score, dtype=np.float64)
    Q = len(query_off) - 1
    ap = np.full(Q, -1.0)
    invalid = 0
    for q in range(Q):
        if not valid_query(query_off, q, score.size):
            invalid += 1
            continue
        lo, hi = int(query_off[q]), int(query_off[q + 1])
        lab = np.asarray(label[lo:hi])[rank_order(score[lo:hi])]
        n_pos = int((lab > 0).sum())
        if n_pos == 0:
            continue
        total, hits = np.float64(0.0), 0
        for r in range(min(k, hi - lo)):
            if lab[r] > 0:
                hits += 1
                total = total + np.float64(hits) / np.float64(r + 1)
        ap[q] = total / np.float64(min(n_pos, k))
    return ap, invalid


def mean_ap(ap):
    ok = ap >= 0
    return float(np.sum(ap[ok]) / ok.sum()) if ok.any() else float('nan')


# ---- quantisation

def quant_exp(m):
    """e = 30 - x for m = f * 2^x, f in [0.5, 1); 0 for m == 0."""
    if not m > 0:
        return 0
    return 30 - int(np.frexp(np.float64(m))[1])


def quantize(grad, hess):
    """(q int32 [n, 2], (e_g, e_h))."""
    grad, hess = np.asarray(grad, dtype=np.float64), np.asarray(hess, dtype=np.float64)
    mg = float(np.max(np.abs(grad))) if grad.size else 0.0
    mh = max(float(np.max(hess)), 0.0) if hess.size else 0.0
    eg, eh = quant_exp(mg), quant_exp(mh)
    q = np.zeros((grad.size, 2), dtype=np.int32)
    if mg > 0:
        q[:, 0] = np.rint(np.ldexp(grad, eg)).astype(np.int32)      # np.rint rounds half to even
    if mh > 0:
        q[:, 1] = np.rint(np.ldexp(hess, eh)).astype(np.int32)
    return q, (eg, eh)


# ---- histogram, split search, growth

def histogram(bins, q, rows):
    """int64 [3, F, 256] = (sum qg, sum qh, rows) of the rows listed."""
    F = bins.shape[0]
    hist = np.zeros((3, F, 256), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    for f in range(F):
        b = bins[f, rows].astype(np.int64)
        np.add.at(hist[0, f], b, q[rows, 0].astype(np.int64))
        np.add.at(hist[1, f], b, q[rows, 1].astype(np.int64))
        np.add.at(hist[2, f], b, 1)
    return hist


def best_split(hist, n_edges, exps, min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split):
    """None, or dict(feature, bin, default_left, gain, cnt_left, g_left, h_left, cnt, g, h); the parent's sums are those
    of feature 0's 256 bins."""
    eg, eh = int(exps[0]), int(exps[1])
    G = lambda gq: np.ldexp(np.asarray(gq, dtype=np.int64).astype(np.float64), -eg)      # int64 -> float64 rounds to nearest
    H = lambda hq: np.ldexp(np.asarray(hq, dtype=np.int64).astype(np.float64), -eh)
    l2 = np.float64(lambda_l2)
    gP, hP, cP = (int(hist[k, 0].sum()) for k in range(3))
    best = None
    for f in range(hist.shape[1]):
        ne = int(n_edges[f])
        if ne == 0:
            continue
        # one entry per edge b (vectorised over b; every operation is still one float64 operation per element)
        cg, ch, cc = (np.cumsum(hist[k, f])[:ne] for k in range(3))
        for default_left in (0, 1):
            gL, hL, cL = (c + default_left * int(hist[k, f, NAN_BIN]) for k, c in enumerate((cg, ch, cc)))
            gR, hR, cR = gP - gL, hP - hL, cP - cL
            ok = (cL >= min_data_in_leaf) & (cR >= min_data_in_leaf) & (H(hL) >= min_sum_hessian_in_leaf) & \
                 (H(hR) >= min_sum_hessian_in_leaf)
            with np.errstate(divide='ignore', invalid='ignore'):
                gain = (G(gL) * G(gL) / (H(hL) + l2) + G(gR) * G(gR) / (H(hR) + l2)) - G(gP) * G(gP) / (H(hP) + l2)
            ok &= gain > min_gain_to_split
            for b in np.flatnonzero(ok):
                # largest gain; ties: smallest f, then smallest b, then NaN-right
                if best is None or gain[b] > best['gain'] or (gain[b] == best['gain'] and best['feature'] == f and b < best['bin']):
                    best = dict(feature=f, bin=int(b), default_left=default_left, gain=float(gain[b]), cnt_left=int(cL[b]),
                                g_left=int(gL[b]), h_left=int(hL[b]), cnt=cP, g=gP, h=hP)
    return best


def goes_left(bin_values, split_bin, default_left):
    return np.where(bin_values == NAN_BIN, bool(default_left), bin_values.astype(np.int64) <= split_bin)


def partition(bins, rows, feature, split_bin, default_left):
    """(left rows, right rows), each in the order of ``rows``."""
    rows = np.asarray(rows)
    left = goes_left(bins[feature, rows], split_bin, default_left)
    return rows[left], rows[~left]


DEFAULTS = dict(num_leaves=128, min_data_in_leaf=2000, min_sum_hessian_in_leaf=1e-3, lambda_l2=0.01, min_gain_to_split=1e-5,
                learning_rate=0.1, lambdarank_truncation_level=30, lambdarank_norm=True, sigmoid=1.0, eval_at=20)


def grow_tree(bins, q, exps, edge_list, p):
    """dict of the tree's arrays (as a ``gbdt.BinTree`` holds them) plus ``leaf_rows``: the row ids of every leaf."""
    n_edges = [len(e) for e in edge_list]
    args = (p['min_data_in_leaf'], p['min_sum_hessian_in_leaf'], p['lambda_l2'], p['min_gain_to_split'])
    n = bins.shape[1]
    leaf_rows = [np.arange(n)]
    hists = [histogram(bins, q, leaf_rows[0])]
    splits = [best_split(hists[0], n_edges, exps, *args)]
    parent = [(-1, 0)]                                   # (internal node that points at this leaf, side)
    nodes = dict(split_feature=[], split_bin=[], default_left=[], threshold=[], decision_type=[], left_child=[], right_child=[],
                 split_gain=[])
    while len(leaf_rows) < p['num_leaves']:
        best = None
        for i, s in enumerate(splits):
            if s is not None and (best is None or s['gain'] > splits[best]['gain']):
                best = i
        if best is None:
            break
        s, node, right = splits[best], len(nodes['split_feature']), len(leaf_rows)
        nodes['split_feature'].append(s['feature'])
        nodes['split_bin'].append(s['bin'])
        nodes['default_left'].append(s['default_left'])
        nodes['threshold'].append(np.float64(edge_list[s['feature']][s['bin']]))
        nodes['decision_type'].append((2 << 2) | (2 if s['default_left'] else 0))
        nodes['split_gain'].append(s['gain'])
        nodes['left_child'].append(~best)
        nodes['right_child'].append(~right)
        if parent[best][0] >= 0:
            nodes['right_child' if parent[best][1] else 'left_child'][parent[best][0]] = node
        rows_l, rows_r = partition(bins, leaf_rows[best], s['feature'], s['bin'], s['default_left'])
        assert rows_l.size == s['cnt_left']
        hist_l = histogram(bins, q, rows_l)
        hist_r = hists[best] - hist_l                    # exact: integers
        leaf_rows[best], hists[best], parent[best] = rows_l, hist_l, (node, 0)
        leaf_rows.append(rows_r); hists.append(hist_r); parent.append((node, 1))
        splits[best] = best_split(hist_l, n_edges, exps, *args)
        splits.append(best_split(hist_r, n_edges, exps, *args))
    eg, eh = int(exps[0]), int(exps[1])
    leaf_value = []
    for h in hists:
        G = np.ldexp(np.float64(int(h[0, 0].sum())), -eg)
        H = np.ldexp(np.float64(int(h[1, 0].sum())), -eh)
        leaf_value.append(-(G / (H + np.float64(p['lambda_l2']))) * np.float64(p['learning_rate']))
    out = {k: np.array(v, dtype=np.float64 if k in ('threshold', 'split_gain') else np.int8 if k == 'decision_type' else np.int32)
           for k, v in nodes.items()}
    out['leaf_value'] = np.array(leaf_value, dtype=np.float64)
    out['leaf_count'] = np.array([r.size for r in leaf_rows], dtype=np.int64)
    out['leaf_rows'] = leaf_rows
    return out


def route(bins, tree):
    """The leaf of every column of ``bins`` under ``tree`` (bin space)."""
    n = bins.shape[1]
    L = tree['leaf_value'].size
    cur = np.zeros(n, dtype=np.int64) if L > 1 else np.full(n, -1, dtype=np.int64)
    rows = np.arange(n)
    for _ in range(L - 1):
        act = rows[cur >= 0]
        if act.size == 0:
            break
        c = cur[act]
        b = bins[tree['split_feature'][c], act]
        left = np.where(b == NAN_BIN, tree['default_left'][c] != 0, b.astype(np.int64) <= tree['split_bin'][c])
        cur[act] = np.where(left, tree['left_child'][c], tree['right_child'][c])
    assert (cur < 0).all()
    return (~cur).astype(np.int32)


def train(bins, label, query_off, edge_list, params=None, valid=None, num_boost_round=100, early_stopping_rounds=None):
    """dict(trees, best_iteration, history, train_score, train_leaf int32 [n, T]) under SPEC-GBDT's boosting rules."""
    p = dict(DEFAULTS)
    p.update(params or {})
    n = bins.shape[1]
    score = np.zeros(n)
    scores_after = []
    if valid is not None:
        vbins, vlabel, voff = valid
        vscore = np.zeros(vbins.shape[1])
    trees, leaves, history = [], [], []
    best_metric, best_iter = None, 0
    for it in range(num_boost_round):
        grad, hess, invalid = lambdarank(score, label, query_off, p['sigmoid'], p['lambdarank_truncation_level'], p['lambdarank_norm'])
        assert invalid == 0
        q, exps = quantize(grad, hess)
        tree = grow_tree(bins, q, exps, edge_list, p)
        if tree['leaf_value'].size < 2:
            break
        leaf = np.zeros(n, dtype=np.int32)
        for i, r in enumerate(tree['leaf_rows']):
            leaf[r] = i
        trees.append(tree)
        leaves.append(leaf)
        score = score + tree['leaf_value'][leaf]
        scores_after.append(score)
        if valid is not None:
            vscore = vscore + tree['leaf_value'][route(vbins, tree)]
            m = mean_ap(ap_at_k(vscore, vlabel, voff, p['eval_at'])[0])
            history.append(m)
            if best_metric is None or m > best_metric:
                best_metric, best_iter = m, it + 1
            if early_stopping_rounds and it + 1 - best_iter >= early_stopping_rounds:
                break
    if not trees:
        raise ValueError('no tree could be grown')
    if valid is None or not early_stopping_rounds:
        best_iter = len(trees)
    return dict(trees=trees[:best_iter], best_iteration=best_iter, history=history, train_score=scores_after[best_iter - 1],
                train_leaf=np.stack(leaves[:best_iter], axis=1))


def to_forest(trees, n_features):
    """The ``ranker.forest.Forest`` of restated trees."""
    from otto_amd.ranker.forest import Forest
    cat = lambda k, dt: np.concatenate([t[k] for t in trees]).astype(dt)
    node_off = np.concatenate([[0], np.cumsum([t['leaf_value'].size - 1 for t in trees])])
    leaf_off = np.concatenate([[0], np.cumsum([t['leaf_value'].size for t in trees])])
    return Forest(node_off, leaf_off, cat('split_feature', np.int32), cat('threshold', np.float64), cat('decision_type', np.int8),
                  cat('left_child', np.int32), cat('right_child', np.int32), cat('leaf_value', np.float64), n_features)


# ---- seeded data for the device tests

def random_problem(rng, n_queries, F, min_len=5, max_len=45, nan_share=0.10, pos_share=0.15, n_levels=None):
    """(X float32 [n, F], label int32 [n], query_off int64 [Q+1]): the label follows a noisy function of the columns, so
    that trees find real splits. ``n_levels``: round the columns to that many values (few distinct values per feature)."""
    lens = rng.integers(min_len, max_len + 1, n_queries)
    query_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(query_off[-1])
    X = rng.standard_normal((n, F)).astype(np.float32)
    if n_levels:
        X = (np.round(X * n_levels / 4) / (n_levels / 4)).astype(np.float32)
    signal = X[:, 0] - 0.7 * X[:, min(1, F - 1)] + 0.5 * np.abs(X[:, min(2, F - 1)]) + rng.standard_normal(n) * 0.8
    label = (signal > np.quantile(signal, 1 - pos_share)).astype(np.int32)
    X[rng.random((n, F)) < nan_share] = np.nan
    return X, label, query_off
