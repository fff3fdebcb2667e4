"""SPEC-XGB (include/otto_xgb.h) restated in NumPy float64 and Python integers on top of
tests/gbdt_restatement.py and tests/gbdt_sampling_restatement.py: the rank:pairwise objective, depth-wise growth, the
``map`` metric, the boosting loop and the fold loop.

Written from the spec, for clarity: a sequential loop over the pairs of a query in ascending pair index (which adds, to
every row, the pairs it takes part in in that order), a level-by-level growth over Python lists. Every float64 operation
is a single NumPy / Python operation, so each rounds once, in the order the spec pins.
"""
import numpy as np

import gbdt_restatement as gr
import gbdt_sampling_restatement as sr

mix = sr.mix
MAX_QUERY = gr.MAX_QUERY
MAX_LABEL = 31
DEFAULTS = {'max_depth': 6, 'min_child_weight': 1.0, 'lambda': 1.0, 'gamma': 0.0, 'eta': 0.3, 'base_score': 0.5, 'subsample': 1.0,
            'colsample_bytree': 1.0, 'seed': 0, 'eval_metric': 'map'}


def seeds(seed):
    """(objective_seed, bagging_seed, feature_fraction_seed)."""
    return mix(seed, 1), mix(seed, 2), mix(seed, 3)


# ---- objective

def record_order(lab):
    """``rec``: the ranks ordered by (label descending, rank ascending); ``lab`` is by rank."""
    return sorted(range(len(lab)), key=lambda r: (-int(lab[r]), r))


def query_pairs(lab, rows, seed_it):
    """The draws of one query: a list of (pid, high rank, low rank), ascending pid. ``lab``: labels by rank, ``rows``: the
    row index in [0, n) by rank, ``seed_it`` = mix(objective_seed, it)."""
    cnt = len(lab)
    rec = record_order(lab)
    pairs = []
    for pid, r in enumerate(rec):
        i = sum(1 for x in lab if x > lab[r])               # the bucket [i, j) of this row's label
        j = i + sum(1 for x in lab if x == lab[r])
        nleft, nright = i, cnt - j
        m = nleft + nright
        if m == 0:
            continue
        u = mix(seed_it, int(rows[r])) % m
        if u < nleft:
            pairs.append((pid, rec[u], r))
        else:
            pairs.append((pid, r, rec[u + (j - i)]))
    return pairs


def pairwise(score, label, query_off, seed, it, want_pairs=False):
    """(grad, hess, n_invalid_queries, bad_label): float64 [n]; the rows of a refused query stay zero. ``seed``: the
    objective seed. A label outside 0..31 sets ``bad_label`` (the device clamps it and reports the call)."""
    score = np.asarray(score, dtype=np.float64)
    table, t_lo, factor, _ = gr._tables(1.0)
    n = score.size
    grad, hess = np.zeros(n), np.zeros(n)
    invalid, bad_label = 0, False
    seed_it = mix(seed, it)
    top = float(gr.SIGMOID_BINS - 1)
    all_pairs = []
    for q in range(len(query_off) - 1):
        if not gr.valid_query(query_off, q, n):
            invalid += 1
            all_pairs.append(None)
            continue
        lo, hi = int(query_off[q]), int(query_off[q + 1])
        cnt = hi - lo
        order = gr.rank_order(score[lo:hi])
        s = score[lo:hi][order]
        lab = np.asarray(label[lo:hi])[order].astype(np.int64)
        if ((lab < 0) | (lab > MAX_LABEL)).any():
            bad_label = True
            lab = np.clip(lab, 0, MAX_LABEL)
        g_q, h_q = np.zeros(cnt), np.zeros(cnt)
        pairs = query_pairs(lab, lo + order, seed_it)
        all_pairs.append(pairs)
        for _, high, low in pairs:
            d = s[low] - s[high]
            x = (d - t_lo) * factor
            x = x if x > 0.0 else 0.0                       # NaN -> 0
            x = x if x < top else top
            p = table[int(x)]
            g = p - 1.0
            h = p * (1.0 - p)
            h = h if h > 1e-16 else 1e-16
            h2 = 2.0 * h
            g_q[high] = g_q[high] + g
            g_q[low] = g_q[low] - g
            h_q[high] = h_q[high] + h2
            h_q[low] = h_q[low] + h2
        grad[lo + order], hess[lo + order] = g_q, h_q
    if want_pairs:
        return grad, hess, invalid, bad_label, all_pairs
    return grad, hess, invalid, bad_label


# ---- metric

def mean_average_precision(score, label, query_off, minus=False):
    """``map`` / ``map-``: SPEC-GBDT's AP at k = MAX_QUERY; a query without a positive counts 1.0 / 0.0."""
    ap, invalid = gr.ap_at_k(score, label, query_off, MAX_QUERY)
    assert invalid == 0
    ap = np.where(ap < 0, 0.0 if minus else 1.0, ap)
    return float(np.sum(ap) / ap.size) if ap.size else float('nan')


# ---- depth-wise growth

def grow_tree(bins, q, exps, edge_list, p, bag_rows=None, features=None):
    """dict of the tree's arrays (as an ``xgb.XgbTree`` holds them) plus ``leaf_rows`` (in-bag rows per leaf),
    ``hist_rows`` and ``n_levels`` (the levels whose split records were read)."""
    n_edges = [len(e) for e in edge_list]
    lam, eta = np.float64(p['lambda']), np.float64(p['eta'])
    args = (0, p['min_child_weight'], p['lambda'], p['gamma'])
    eg, eh = int(exps[0]), int(exps[1])
    first = int(features[0]) if features is not None else 0
    root = np.arange(bins.shape[1]) if bag_rows is None else np.asarray(bag_rows, dtype=np.int64)
    sums = lambda h: (int(h[0, first].sum()), int(h[1, first].sum()))
    # a live leaf: (leaf index, xgb id, rows, histogram, (parent node, side))
    level = [(0, 0, root, sr.histogram(bins, q, root, features), (-1, 0))]
    leaf_rows, leaf_sums = [root], [sums(level[0][3])]
    hist_rows, n_xgb, n_levels = root.size, 1, 0
    nodes = {k: [] for k in ('split_feature', 'split_bin', 'default_left', 'threshold', 'decision_type', 'left_child', 'right_child',
                             'split_gain', 'cover', 'sum_grad', 'count', 'left_id', 'right_id')}
    for depth in range(p['max_depth']):
        if not level:
            break
        n_levels += 1
        nxt = []
        for leaf, xid, rows, hist, parent in level:         # ascending node id
            s = sr.best_split(hist, n_edges, exps, *args, features=features)
            if s is None:
                continue
            node, right = len(nodes['split_feature']), len(leaf_rows)
            nodes['split_feature'].append(s['feature'])
            nodes['split_bin'].append(s['bin'])
            nodes['default_left'].append(s['default_left'])
            nodes['threshold'].append(np.float64(edge_list[s['feature']][s['bin']]))
            nodes['decision_type'].append((2 << 2) | (2 if s['default_left'] else 0))
            nodes['split_gain'].append(s['gain'])
            nodes['cover'].append(np.ldexp(np.float64(s['h']), -eh))
            nodes['sum_grad'].append(np.ldexp(np.float64(s['g']), -eg))
            nodes['count'].append(s['cnt'])
            nodes['left_child'].append(~leaf)
            nodes['right_child'].append(~right)
            nodes['left_id'].append(n_xgb)
            nodes['right_id'].append(n_xgb + 1)
            if parent[0] >= 0:
                nodes['right_child' if parent[1] else 'left_child'][parent[0]] = node
            rows_l, rows_r = gr.partition(bins, rows, s['feature'], s['bin'], s['default_left'])
            assert rows_l.size == s['cnt_left'] and s['cnt'] == rows.size
            leaf_rows[leaf] = rows_l
            leaf_rows.append(rows_r)
            leaf_sums[leaf] = (s['g_left'], s['h_left'])
            leaf_sums.append((s['g'] - s['g_left'], s['h'] - s['h_left']))
            if depth + 1 < p['max_depth']:                  # the children are searched in turn: the smaller one is built
                hist_l = sr.histogram(bins, q, rows_l, features)
                hist_r = hist - hist_l                      # exact: integers
                assert sums(hist_l) == leaf_sums[leaf] and sums(hist_r) == leaf_sums[right]
                hist_rows += min(rows_l.size, rows_r.size)
                nxt.append((leaf, n_xgb, rows_l, hist_l, (node, 0)))
                nxt.append((right, n_xgb + 1, rows_r, hist_r, (node, 1)))
            n_xgb += 2
        level = nxt
    leaf_value, leaf_cover, leaf_grad = [], [], []
    for gq, hq in leaf_sums:
        G, H = np.ldexp(np.float64(gq), -eg), np.ldexp(np.float64(hq), -eh)
        leaf_value.append(np.float64(np.float32(-(G / (H + lam)) * eta)))
        leaf_cover.append(H)
        leaf_grad.append(G)
    dtype = lambda k: np.float64 if k in ('threshold', 'split_gain', 'cover', 'sum_grad') else np.int8 if k == 'decision_type' \
        else np.int64 if k == 'count' else np.int32
    out = {k: np.array(v, dtype=dtype(k)) for k, v in nodes.items()}
    out['leaf_value'] = np.array(leaf_value, dtype=np.float64)
    out['leaf_cover'] = np.array(leaf_cover, dtype=np.float64)
    out['leaf_sum_grad'] = np.array(leaf_grad, dtype=np.float64)
    out['leaf_count'] = np.array([r.size for r in leaf_rows], dtype=np.int64)
    out['leaf_rows'] = leaf_rows
    out['hist_rows'] = hist_rows
    out['n_levels'] = n_levels
    return out


def feature_importance(trees, F):
    """(gain, weight, cover): mean gain per split, number of splits, mean cover per split; 0 for an unused feature."""
    gain, cover, weight = np.zeros(F), np.zeros(F), np.zeros(F, dtype=np.int64)
    for t in trees:
        for f, g, c in zip(t['split_feature'], t['split_gain'], t['cover']):
            gain[f] += g
            cover[f] += c
            weight[f] += 1
    used = weight > 0
    gain[used] /= weight[used]
    cover[used] /= weight[used]
    return gain, weight, cover


def train(bins, label, query_off, edge_list, params=None, valid=None, num_boost_round=10, early_stopping_rounds=None):
    """dict(trees, best_iteration, history, train_score, margin, base_score, bags, features) under SPEC-XGB's boosting
    rules: the score of an iteration is base_score + margin, margin the leaf values added in tree order from 0.0."""
    p = dict(DEFAULTS)
    p.update(params or {})
    F, n = bins.shape
    base = np.float64(p['base_score'])
    objective_seed, bagging_seed, feature_seed = seeds(p['seed'])
    margin = np.zeros(n)
    margins_after = []
    if valid is not None:
        vbins, vlabel, voff = valid
        vmargin = np.zeros(vbins.shape[1])
    trees, history, bags, lists = [], [], [], []
    best_metric, best_iter = None, 0
    bag_on = p['subsample'] < 1
    m = sr.bag_size(p['subsample'], n) if bag_on else n
    assert m >= 1
    for it in range(num_boost_round):
        grad, hess, invalid, bad_label = pairwise(margin + base, label, query_off, objective_seed, it)
        assert invalid == 0 and not bad_label
        q, exps = gr.quantize(grad, hess)
        bag_rows = sr.bag(n, m, mix(bagging_seed, 2 * it)) if bag_on else None
        features = sr.feature_list(F, p['colsample_bytree'], feature_seed, it) if p['colsample_bytree'] < 1 else None
        tree = grow_tree(bins, q, exps, edge_list, p, bag_rows, features)
        if tree['leaf_value'].size < 2:
            break
        leaf = gr.route(bins, tree)
        for i, r in enumerate(tree['leaf_rows']):
            assert (leaf[r] == i).all()
        trees.append(tree)
        bags.append(bag_rows)
        lists.append(features)
        margin = margin + tree['leaf_value'][leaf]
        margins_after.append(margin)
        if valid is not None:
            vmargin = vmargin + tree['leaf_value'][gr.route(vbins, tree)]
            metric = mean_average_precision(vmargin + base, vlabel, voff, p['eval_metric'] == 'map-')
            history.append(metric)
            if best_metric is None or metric > best_metric:
                best_metric, best_iter = metric, it + 1
            if early_stopping_rounds and it + 1 - best_iter >= early_stopping_rounds:
                break
    if not trees:
        raise ValueError('no tree could be grown')
    if valid is None or not early_stopping_rounds:
        best_iter = len(trees)
    return dict(trees=trees[:best_iter], best_iteration=best_iter, history=history, margin=margins_after[best_iter - 1],
                train_score=margins_after[best_iter - 1] + base, base_score=float(base), bags=bags[:best_iter],
                features=lists[:best_iter], n_grown=len(trees))


def predict_bins(bins, trees, base_score):
    """base_score + the leaf values of the trees added in tree order from 0.0, routing the bins."""
    margin = np.zeros(bins.shape[1])
    for tree in trees:
        margin = margin + tree['leaf_value'][gr.route(bins, tree)]
    return margin + np.float64(base_score)
