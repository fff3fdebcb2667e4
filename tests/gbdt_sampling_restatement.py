"""The sampling of SPEC-GBDT (include/otto_gbdt.h, "Sampling") restated in NumPy and Python integers
on top of tests/gbdt_restatement.py: the sampler, the row bag, the feature list, the histogram and the split search over a
list, the growth of a tree on a bag and a list, and the boosting loop that draws them.

Written for clarity: the bag sorts all n keys, the split search over a list searches the listed features' planes alone and
maps the winner back, the parent sums are read off the first listed plane.
"""
import numpy as np

import folds_restatement as fr
import gbdt_restatement as gr

mix = fr.key_int                                     # mix(s, i) of the spec is the row key of SPEC-FOLDS


def bag_size(fraction, n):
    return int(float(fraction) * int(n))


def bag(n, m, seed):
    """The m rows of [0, n) with the smallest mix(seed, r), ascending. ``seed`` is the mixed mix(bagging_seed, 2 * d)."""
    keys = fr.keys(seed, np.arange(n))
    assert np.unique(keys).size == n                  # distinct rows, distinct keys: exactly m rows pass
    return np.sort(np.argsort(keys, kind='stable')[:m]).astype(np.int32)


def n_used(F, fraction):
    return max(min(2, F), int(np.floor(F * float(fraction) + 0.5)))


def feature_list(F, fraction, seed, it):
    keys = fr.keys(mix(seed, 2 * it + 1), np.arange(F))
    return np.sort(np.argsort(keys, kind='stable')[:n_used(F, fraction)]).astype(np.int32)


def histogram(bins, q, rows, features=None):
    """int64 [3, F, 256]; with a list, the planes of the features outside it are zero."""
    if features is None:
        return gr.histogram(bins, q, rows)
    features = np.asarray(features, dtype=np.int64)
    hist = np.zeros((3, bins.shape[0], 256), dtype=np.int64)
    hist[:, features] = gr.histogram(bins[features], q, rows)
    return hist


def best_split(hist, n_edges, exps, min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split, features=None):
    """As ``gr.best_split``, over the listed features: ties go to the smallest listed feature, the parent's sums are those
    of the first listed feature."""
    if features is None:
        return gr.best_split(hist, n_edges, exps, min_data_in_leaf, min_sum_hessian_in_leaf, lambda_l2, min_gain_to_split)
    features = np.asarray(features, dtype=np.int64)
    best = gr.best_split(hist[:, features], [n_edges[f] for f in features], exps, min_data_in_leaf, min_sum_hessian_in_leaf,
                         lambda_l2, min_gain_to_split)
    if best is not None:
        best['feature'] = int(features[best['feature']])
    return best


def grow_tree(bins, q, exps, edge_list, p, bag_rows=None, features=None):
    """``gr.grow_tree`` with the root's row list set to the bag and every histogram and split search over the list.
    ``leaf_rows`` holds in-bag rows only; ``hist_rows``: the rows the histograms were built from (the root, then the
    smaller child of every split but the last one that fills num_leaves)."""
    n_edges = [len(e) for e in edge_list]
    args = (p['min_data_in_leaf'], p['min_sum_hessian_in_leaf'], p['lambda_l2'], p['min_gain_to_split'])
    first = int(features[0]) if features is not None else 0
    root = np.arange(bins.shape[1]) if bag_rows is None else np.asarray(bag_rows, dtype=np.int64)
    leaf_rows = [root]
    hists = [histogram(bins, q, root, features)]
    hist_rows = root.size
    splits = [best_split(hists[0], n_edges, exps, *args, features=features)]
    parent = [(-1, 0)]
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
        assert features is None or s['feature'] in set(int(f) for f in features)
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
        rows_l, rows_r = gr.partition(bins, leaf_rows[best], s['feature'], s['bin'], s['default_left'])
        assert rows_l.size == s['cnt_left']
        hist_l = histogram(bins, q, rows_l, features)
        hist_r = hists[best] - hist_l
        if right + 1 < p['num_leaves']:                   # the device builds the smaller child, unless the tree is full
            hist_rows += min(rows_l.size, rows_r.size)
        leaf_rows[best], hists[best], parent[best] = rows_l, hist_l, (node, 0)
        leaf_rows.append(rows_r); hists.append(hist_r); parent.append((node, 1))
        splits[best] = best_split(hist_l, n_edges, exps, *args, features=features)
        splits.append(best_split(hist_r, n_edges, exps, *args, features=features))
    eg, eh = int(exps[0]), int(exps[1])
    leaf_value = []
    for h in hists:
        G = np.ldexp(np.float64(int(h[0, first].sum())), -eg)
        H = np.ldexp(np.float64(int(h[1, first].sum())), -eh)
        leaf_value.append(-(G / (H + np.float64(p['lambda_l2']))) * np.float64(p['learning_rate']))
    out = {k: np.array(v, dtype=np.float64 if k in ('threshold', 'split_gain') else np.int8 if k == 'decision_type' else np.int32)
           for k, v in nodes.items()}
    out['leaf_value'] = np.array(leaf_value, dtype=np.float64)
    out['leaf_count'] = np.array([r.size for r in leaf_rows], dtype=np.int64)
    out['leaf_rows'] = leaf_rows
    out['hist_rows'] = hist_rows
    return out


def train(bins, label, query_off, edge_list, params=None, valid=None, num_boost_round=100, early_stopping_rounds=None,
          bagging_fraction=1.0, bagging_freq=0, feature_fraction=1.0, bagging_seed=3, feature_fraction_seed=2):
    """``gr.train`` with the draws of the spec: dict(trees, best_iteration, history, train_score, train_leaf, bags,
    features). The score of every row moves with every tree, whether the row was in the tree's bag or not: the leaf of a
    row comes from routing its bins through the tree."""
    p = dict(gr.DEFAULTS)
    p.update(params or {})
    F, n = bins.shape
    score = np.zeros(n)
    scores_after = []
    if valid is not None:
        vbins, vlabel, voff = valid
        vscore = np.zeros(vbins.shape[1])
    trees, leaves, history, bags, lists = [], [], [], [], []
    best_metric, best_iter = None, 0
    bag_on = bagging_freq > 0 and bagging_fraction < 1
    m = bag_size(bagging_fraction, n) if bag_on else n
    assert m >= 1
    bag_rows = None
    for it in range(num_boost_round):
        grad, hess, invalid = gr.lambdarank(score, label, query_off, p['sigmoid'], p['lambdarank_truncation_level'],
                                            p['lambdarank_norm'])
        assert invalid == 0
        q, exps = gr.quantize(grad, hess)
        if bag_on and it % bagging_freq == 0:
            bag_rows = bag(n, m, mix(bagging_seed, 2 * (it // bagging_freq)))
        features = feature_list(F, feature_fraction, feature_fraction_seed, it) if feature_fraction < 1 else None
        tree = grow_tree(bins, q, exps, edge_list, p, bag_rows, features)
        if tree['leaf_value'].size < 2:
            break
        leaf = gr.route(bins, tree)
        for i, r in enumerate(tree['leaf_rows']):         # the in-bag rows sit where the partition put them
            assert (leaf[r] == i).all()
        trees.append(tree)
        leaves.append(leaf)
        bags.append(bag_rows)
        lists.append(features)
        score = score + tree['leaf_value'][leaf]
        scores_after.append(score)
        if valid is not None:
            vscore = vscore + tree['leaf_value'][gr.route(vbins, tree)]
            metric = gr.mean_ap(gr.ap_at_k(vscore, vlabel, voff, p['eval_at'])[0])
            history.append(metric)
            if best_metric is None or metric > best_metric:
                best_metric, best_iter = metric, it + 1
            if early_stopping_rounds and it + 1 - best_iter >= early_stopping_rounds:
                break
    if not trees:
        raise ValueError('no tree could be grown')
    if valid is None or not early_stopping_rounds:
        best_iter = len(trees)
    return dict(trees=trees[:best_iter], best_iteration=best_iter, history=history, train_score=scores_after[best_iter - 1],
                train_leaf=np.stack(leaves[:best_iter], axis=1), bags=bags[:best_iter], features=lists[:best_iter],
                n_grown=len(trees))
