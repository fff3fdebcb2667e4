"""SPEC-OBJ (include/otto_objective.h) restated in NumPy float64 and Python integers on top of
tests/gbdt_restatement.py and tests/xgb_restatement.py: the pointwise logistic gradients, the label counts and initial
scores, rank:ndcg, NDCG@k, AUC, logloss and the two train loops with the new objectives and metrics.

Written from the spec, for clarity. Every float64 operation is a single NumPy / Python operation, so each rounds once, in
the order the spec pins; the integer sums of AUC are Python integers. tests/test_objectives_cpu.py checks this file against
independent formulations (all pairs, plain sorts, exact exp, hand-worked fractions).
"""
import numpy as np

import gbdt_restatement as gr
import gbdt_sampling_restatement as sr
import xgb_restatement as xr

MAX_QUERY = gr.MAX_QUERY
MAX_LABEL = 31
BINS = gr.SIGMOID_BINS
mix = sr.mix


def gain(label):
    return np.float64((1 << int(label)) - 1)


# ---- 1. pointwise logistic gradients

def binary(score, label, sigma=1.0, w_pos=1.0, w_neg=1.0, hess_floor=0.0):
    """(grad, hess, bad_label): float64 [n]; a row whose label lies outside 0..31 stays zero and sets ``bad_label``."""
    score = np.asarray(score, dtype=np.float64)
    label = np.asarray(label)
    table, t_lo, factor, _ = gr._tables(1.0)
    sigma, w_pos, w_neg, floor = (np.float64(v) for v in (sigma, w_pos, w_neg, hess_floor))
    with np.errstate(invalid='ignore', over='ignore'):
        x = (-(sigma * score) - t_lo) * factor
        x = np.where(x > 0.0, x, 0.0)                           # NaN -> 0
        x = np.where(x < float(BINS - 1), x, float(BINS - 1))
        p = table[x.astype(np.int64)]
        t = (label > 0).astype(np.float64)
        w = np.where(label > 0, w_pos, w_neg)
        grad = sigma * (p - t) * w
        h = sigma * sigma * p * (1.0 - p)
        hess = np.where(h > floor, h, floor) * w
    bad = (label < 0) | (label > MAX_LABEL)
    grad[bad] = 0.0
    hess[bad] = 0.0
    return grad, hess, bool(bad.any())


# ---- 2. label counts and initial scores

def label_counts(label):
    label = np.asarray(label)
    return int((label > 0).sum()), int(label.size)


def class_weights(n_pos, n, is_unbalance=False, scale_pos_weight=1.0):
    w_pos, w_neg = np.float64(1.0), np.float64(1.0)
    n_neg = n - n_pos
    if is_unbalance and n_pos > 0 and n_neg > 0:
        if n_pos > n_neg:
            w_neg = np.float64(n_pos) / np.float64(n_neg)
        else:
            w_pos = np.float64(n_neg) / np.float64(n_pos)
    return float(w_pos * np.float64(scale_pos_weight)), float(w_neg)


def init_score(n_pos, n, sigma=1.0):
    pavg = np.float64(n_pos) / np.float64(n)
    pavg = min(max(pavg, np.float64(1e-15)), np.float64(1.0 - 1e-15))
    return float(np.log(pavg / (1.0 - pavg)) / np.float64(sigma))


def base_margin(base_score):
    b = np.float64(base_score)
    return float(np.log(b / (1.0 - b)))


# ---- 3. rank:ndcg

def lambdamart(score, label, query_off, seed, it, weighting=1):
    """(grad, hess, n_invalid_queries, bad_label) of SPEC-XGB's pairs with SPEC-OBJ's weights; ``weighting = 0`` repeats
    ``xgb_restatement.pairwise`` operation for operation."""
    score = np.asarray(score, dtype=np.float64)
    table, t_lo, factor, discount = gr._tables(1.0)
    n = score.size
    grad, hess = np.zeros(n), np.zeros(n)
    invalid, bad_label = 0, False
    seed_it = mix(seed, it)
    top = float(BINS - 1)
    for q in range(len(query_off) - 1):
        if not gr.valid_query(query_off, q, n):
            invalid += 1
            continue
        lo, hi = int(query_off[q]), int(query_off[q + 1])
        cnt = hi - lo
        order = gr.rank_order(score[lo:hi])
        s = score[lo:hi][order]
        lab = np.asarray(label[lo:hi])[order].astype(np.int64)
        if ((lab < 0) | (lab > MAX_LABEL)).any():
            bad_label = True
            lab = np.clip(lab, 0, MAX_LABEL)
        idcg = np.float64(0.0)
        for r, l in enumerate(sorted(lab.tolist(), reverse=True)):
            idcg = idcg + gain(l) * discount[r]
        inv_idcg = np.float64(0.0) if idcg == 0.0 else 1.0 / idcg
        g_q, h_q = np.zeros(cnt), np.zeros(cnt)
        for _, high, low in xr.query_pairs(lab, lo + order, seed_it):
            d = s[low] - s[high]
            x = (d - t_lo) * factor
            x = x if x > 0.0 else 0.0                           # NaN -> 0
            x = x if x < top else top
            p = table[int(x)]
            g = p - 1.0
            h = p * (1.0 - p)
            h = h if h > 1e-16 else 1e-16
            h2 = 2.0 * h
            if weighting:
                delta = abs((gain(lab[high]) - gain(lab[low])) * (discount[high] - discount[low])) * inv_idcg
                g = g * delta
                h2 = h2 * delta
            g_q[high] = g_q[high] + g
            g_q[low] = g_q[low] - g
            h_q[high] = h_q[high] + h2
            h_q[low] = h_q[low] + h2
        grad[lo + order], hess[lo + order] = g_q, h_q
    return grad, hess, invalid, bad_label


# ---- 4. metrics

def ndcg_at_k(score, label, query_off, k):
    """(ndcg float64 [Q], n_invalid): -1 where maxDCG is 0 and for a refused query."""
    score = np.asarray(score, dtype=np.float64)
    _, _, _, discount = gr._tables(1.0)
    Q = len(query_off) - 1
    out = np.full(Q, -1.0)
    invalid = 0
    for q in range(Q):
        if not gr.valid_query(query_off, q, score.size):
            invalid += 1
            continue
        lo, hi = int(query_off[q]), int(query_off[q + 1])
        lab = np.clip(np.asarray(label[lo:hi])[gr.rank_order(score[lo:hi])].astype(np.int64), 0, MAX_LABEL)
        top = min(k, hi - lo)
        dcg, best = np.float64(0.0), np.float64(0.0)
        for r in range(top):
            dcg = dcg + gain(lab[r]) * discount[r]
        for r, l in enumerate(sorted(lab.tolist(), reverse=True)[:top]):
            best = best + gain(l) * discount[r]
        if best != 0.0:
            out[q] = dcg / best
    return out, invalid


def mean_ndcg(ndcg, minus=False):
    v = np.where(ndcg < 0, 0.0 if minus else 1.0, ndcg)
    return float(np.sum(v) / v.size) if v.size else float('nan')


def score_key(x):
    """SPEC-GBDT's order-preserving uint64 image of a float64 as a Python int: -0.0 folded onto +0.0, every NaN -> 1."""
    x = np.float64(x)
    if x != x:
        return 1
    b = 0 if x == 0.0 else int(np.array(x).view(np.uint64))
    return (~b) & ((1 << 64) - 1) if b >> 63 else b | (1 << 63)


def auc_counts(score, label):
    """(A2, P, N) as Python integers, by tie groups of the descending key."""
    key = [((1 << 64) - 1) ^ score_key(s) for s in np.asarray(score, dtype=np.float64)]
    pos = [1 if l > 0 else 0 for l in np.asarray(label)]
    order = sorted(range(len(key)), key=lambda i: key[i])
    ppre = [0]
    for i in order:
        ppre.append(ppre[-1] + pos[i])
    a2, a, n = 0, 0, len(key)
    while a < n:
        b = a + 1
        while b < n and key[order[b]] == key[order[a]]:
            b += 1
        neg = (b - a) - (ppre[b] - ppre[a])
        a2 += neg * (ppre[a] + ppre[b])
        a = b
    return a2, ppre[n], n - ppre[n]


def auc_from_counts(a2, p, n):
    if p == 0 or n == 0:
        return 1.0
    return float(np.float64(a2) / (2.0 * np.float64(p) * np.float64(n)))


def auc(score, label):
    return auc_from_counts(*auc_counts(score, label))


def logloss_terms(score, label, sigma=1.0):
    m = np.float64(sigma) * np.asarray(score, dtype=np.float64)
    z = np.where(np.asarray(label) > 0, -m, m)
    with np.errstate(over='ignore'):
        return np.where(z > 0.0, z + np.log1p(np.exp(-z)), np.log1p(np.exp(z)))


def logloss_sum(score, label, sigma=1.0):
    return float(np.sum(logloss_terms(score, label, sigma)))


def logloss(score, label, sigma=1.0):
    return logloss_sum(score, label, sigma) / len(score) if len(score) else float('nan')


HIGHER = {'map': True, 'ndcg': True, 'auc': True, 'logloss': False}


def evaluate(metric, score, label, query_off, k=MAX_QUERY, minus=None, sigma=1.0):
    if metric == 'map':
        ap, invalid = gr.ap_at_k(score, label, query_off, k)
        assert invalid == 0
        if minus is None:
            return gr.mean_ap(ap)
        ap = np.where(ap < 0, 0.0 if minus else 1.0, ap)
        return float(np.sum(ap) / ap.size) if ap.size else float('nan')
    if metric == 'ndcg':
        v, invalid = ndcg_at_k(score, label, query_off, k)
        assert invalid == 0
        return mean_ndcg(v, bool(minus))
    if metric == 'auc':
        return auc(score, label)
    if metric == 'logloss':
        return logloss(score, label, sigma)
    raise ValueError(metric)


# ---- the train loops

GBDT_DEFAULTS = dict(gr.DEFAULTS, objective='binary', metric='map', is_unbalance=False, scale_pos_weight=1.0, boost_from_average=True)


def _loop(n, init, gradients, grow, route, valid, vinit, metric_of, higher, rounds, early):
    """The boosting loop both families share: scores start at ``init``; returns (trees, best_iter, history, scores after
    every tree)."""
    score = np.full(n, np.float64(init))
    if valid is not None:
        vscore = np.full(valid[0].shape[1], np.float64(vinit))
    trees, history, after = [], [], []
    best_metric, best_iter = None, 0
    for it in range(rounds):
        grad, hess = gradients(score, it)
        q, exps = gr.quantize(grad, hess)
        tree = grow(q, exps, it)
        if tree['leaf_value'].size < 2:
            break
        trees.append(tree)
        score = score + tree['leaf_value'][route(None, tree)]
        after.append(score)
        if valid is not None:
            vscore = vscore + tree['leaf_value'][route(valid[0], tree)]
            m = metric_of(vscore)
            history.append(m)
            if best_metric is None or (m > best_metric if higher else m < best_metric):
                best_metric, best_iter = m, it + 1
            if early and it + 1 - best_iter >= early:
                break
    if not trees:
        raise ValueError('no tree could be grown')
    if valid is None or not early:
        best_iter = len(trees)
    return trees, best_iter, history, after


def train_gbdt(bins, label, query_off, edge_list, params=None, valid=None, num_boost_round=100, early_stopping_rounds=None):
    """``gbdt.train`` with ``objective: binary``: dict(trees, best_iteration, history, train_score, init). The first tree of
    ``trees`` carries ``init`` in its leaf values (AddBias)."""
    p = dict(GBDT_DEFAULTS)
    p.update(params or {})
    assert p['objective'] == 'binary'
    n = bins.shape[1]
    n_pos, _ = label_counts(label)
    w_pos, w_neg = class_weights(n_pos, n, p['is_unbalance'], p['scale_pos_weight'])
    init = init_score(n_pos, n, p['sigmoid']) if p['boost_from_average'] else 0.0

    def gradients(score, it):
        g, h, bad = binary(score, label, p['sigmoid'], w_pos, w_neg, 0.0)
        assert not bad
        return g, h

    route = lambda b, tree: gr.route(bins if b is None else b, tree)
    metric_of = None
    if valid is not None:
        metric_of = lambda vs: evaluate(p['metric'], vs, valid[1], valid[2], k=p['eval_at'],
                                        minus=None if p['metric'] == 'map' else False, sigma=p['sigmoid'])
    trees, best_iter, history, after = _loop(n, init, gradients, lambda q, exps, it: gr.grow_tree(bins, q, exps, edge_list, p), route,
                                             valid, init, metric_of, HIGHER[p['metric']], num_boost_round, early_stopping_rounds)
    trees = trees[:best_iter]
    if init != 0.0:
        trees[0] = dict(trees[0], leaf_value=trees[0]['leaf_value'] + np.float64(init))
    return dict(trees=trees, best_iteration=best_iter, history=history, train_score=after[best_iter - 1], init=init)


def parse_metric(name):
    if name in ('auc', 'logloss'):
        return name, MAX_QUERY, False
    minus = name.endswith('-')
    head, _, k = (name[:-1] if minus else name).partition('@')
    return head, int(k) if k else MAX_QUERY, minus


def train_xgb(bins, label, query_off, edge_list, params=None, valid=None, num_boost_round=10, early_stopping_rounds=None):
    """``xgb.train`` with ``rank:ndcg`` or ``binary:logistic`` (no sampling): dict(trees, best_iteration, history,
    train_score, base_margin)."""
    p = dict(xr.DEFAULTS, objective='rank:ndcg', scale_pos_weight=1.0)
    p.update(params or {})
    assert p['subsample'] == 1.0 and p['colsample_bytree'] == 1.0
    n = bins.shape[1]
    objective_seed = xr.seeds(p['seed'])[0]
    base = base_margin(p['base_score']) if p['objective'] == 'binary:logistic' else float(p['base_score'])
    metric, k, minus = parse_metric(p['eval_metric'])

    def gradients(margin, it):
        if p['objective'] == 'binary:logistic':
            g, h, bad = binary(margin + np.float64(base), label, 1.0, p['scale_pos_weight'], 1.0, 1e-16)
            assert not bad
            return g, h
        g, h, invalid, bad = lambdamart(margin + np.float64(base), label, query_off, objective_seed, it, 1 if p['objective'] == 'rank:ndcg' else 0)
        assert invalid == 0 and not bad
        return g, h

    route = lambda b, tree: gr.route(bins if b is None else b, tree)
    metric_of = None
    if valid is not None:
        metric_of = lambda vm: evaluate(metric, vm + np.float64(base), valid[1], valid[2], k=k, minus=minus)
    trees, best_iter, history, after = _loop(n, 0.0, gradients, lambda q, exps, it: xr.grow_tree(bins, q, exps, edge_list, p), route, valid,
                                             0.0, metric_of, HIGHER[metric], num_boost_round, early_stopping_rounds)
    return dict(trees=trees[:best_iter], best_iteration=best_iter, history=history, margin=after[best_iter - 1],
                train_score=after[best_iter - 1] + np.float64(base), base_margin=base)
