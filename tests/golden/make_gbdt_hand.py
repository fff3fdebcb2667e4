"""Writes tests/golden/gbdt_hand.json: SPEC-GBDT worked through on 8 rows, 2 features (one NaN), 2 queries, all scores 0,
num_leaves = 3, min_data_in_leaf = 1, lambdarank_norm off -- in scalar Python (math, lists, ints), step by step, sharing
no code with tests/gbdt_restatement.py. Every intermediate is written out. With all scores 0 the sigmoid is exactly 0.5.

    python tests/golden/make_gbdt_hand.py
"""
import json
import math
import os

X = [[0.5, 1.0], [1.5, None], [0.5, 3.0], [2.5, 2.0], [1.5, 1.0], [2.5, 3.0], [0.5, 2.0], [3.5, 1.0]]     # None: NaN
LABEL = [0, 1, 0, 1, 0, 1, 0, 1]
QUERY_OFF = [0, 4, 8]
EDGES = [[0.5, 1.5, 2.5], [1.0, 2.0]]          # the distinct values of each column but the last
P = dict(num_leaves=3, min_data_in_leaf=1, min_sum_hessian_in_leaf=1e-3, lambda_l2=0.01, min_gain_to_split=1e-5,
         learning_rate=0.1, lambdarank_truncation_level=30, lambdarank_norm=False, sigmoid=1.0)

bins = [[255 if x[f] is None else sum(1 for e in EDGES[f] if e < x[f]) for x in X] for f in range(2)]
disc = [1.0 / math.log2(2.0 + r) for r in range(4)]
grad, hess = [0.0] * 8, [0.0] * 8
for q in range(2):
    rows = list(range(QUERY_OFF[q], QUERY_OFF[q + 1]))        # all scores equal: rank order = position order
    gains = sorted((2.0 ** LABEL[r] - 1.0 for r in rows), reverse=True)
    max_dcg = 0.0
    for r, g in enumerate(gains):
        max_dcg = max_dcg + g * disc[r]
    inv = 1.0 / max_dcg
    for i in range(4):
        for j in range(i + 1, 4):
            a, b = rows[i], rows[j]
            if LABEL[a] == LABEL[b]:
                continue
            high, low = (a, b) if LABEL[a] > LABEL[b] else (b, a)
            delta = 1.0 * abs(disc[i] - disc[j]) * inv        # gain difference 1; no norm
            lam = -1.0 * delta * 0.5
            eta = 1.0 * delta * 0.5 * 0.5
            grad[high] += lam
            grad[low] -= lam
            hess[high] += eta
            hess[low] += eta
eg = 30 - math.frexp(max(abs(g) for g in grad))[1]
eh = 30 - math.frexp(max(hess))[1]
qg = [round(math.ldexp(g, eg)) for g in grad]                  # round(): half to even
qh = [round(math.ldexp(h, eh)) for h in hess]


def hist_of(rows):
    h = {}
    for f in range(2):
        for r in rows:
            c = h.setdefault((f, bins[f][r]), [0, 0, 0])
            c[0] += qg[r]; c[1] += qh[r]; c[2] += 1
    return h


def search(rows):
    h = hist_of(rows)
    gP, hP, cP = sum(qg[r] for r in rows), sum(qh[r] for r in rows), len(rows)
    G = lambda v: math.ldexp(float(v), -eg)
    H = lambda v: math.ldexp(float(v), -eh)
    best = None
    for f in range(2):
        for b in range(len(EDGES[f])):
            for dl in (0, 1):
                gL = hL = cL = 0
                for (ff, bb), c in h.items():
                    if ff == f and (bb <= b or (dl and bb == 255)):
                        gL += c[0]; hL += c[1]; cL += c[2]
                gR, hR, cR = gP - gL, hP - hL, cP - cL
                if cL < P['min_data_in_leaf'] or cR < P['min_data_in_leaf']:
                    continue
                if H(hL) < P['min_sum_hessian_in_leaf'] or H(hR) < P['min_sum_hessian_in_leaf']:
                    continue
                gain = (G(gL) * G(gL) / (H(hL) + P['lambda_l2']) + G(gR) * G(gR) / (H(hR) + P['lambda_l2'])) \
                    - G(gP) * G(gP) / (H(hP) + P['lambda_l2'])
                if gain > P['min_gain_to_split'] and (best is None or gain > best['gain']):
                    best = dict(feature=f, bin=b, default_left=dl, gain=gain, cnt_left=cL, g_left=gL, h_left=hL, cnt=cP, g=gP, h=hP)
    return best


def split_rows(rows, s):
    left = [r for r in rows if (bins[s['feature']][r] == 255 and s['default_left']) or
            (bins[s['feature']][r] != 255 and bins[s['feature']][r] <= s['bin'])]
    return left, [r for r in rows if r not in left]


root = list(range(8))
s0 = search(root)
leaf0, leaf1 = split_rows(root, s0)
c0, c1 = search(leaf0), search(leaf1)
pick = 0 if (c0 is not None and (c1 is None or c0['gain'] >= c1['gain'])) else 1
s1 = c0 if pick == 0 else c1
leaves = [leaf0, leaf1]
leaves[pick], new = split_rows(leaves[pick], s1)
leaves.append(new)
left_child, right_child = [~0, 0], [~1, 0]
(left_child if pick == 0 else right_child)[0] = 1
left_child[1], right_child[1] = ~pick, ~2
leaf_value = []
for rows in leaves:
    Gv = math.ldexp(float(sum(qg[r] for r in rows)), -eg)
    Hv = math.ldexp(float(sum(qh[r] for r in rows)), -eh)
    leaf_value.append(-(Gv / (Hv + P['lambda_l2'])) * P['learning_rate'])
hist_json = lambda rows: [[f, b, *c] for (f, b), c in sorted(hist_of(rows).items())]
out = dict(X=X, label=LABEL, query_off=QUERY_OFF, edges=EDGES, params=P, bins=bins, discount=disc, grad=grad, hess=hess,
           exp=[eg, eh], qg=qg, qh=qh, root_hist=hist_json(root), root_split=s0, leaf0_rows=leaf0, leaf1_rows=leaf1,
           leaf0_hist=hist_json(leaf0), leaf1_hist=hist_json(leaf1), leaf0_split=c0, leaf1_split=c1, second_split_leaf=pick,
           leaf_rows=leaves, split_feature=[s0['feature'], s1['feature']], split_bin=[s0['bin'], s1['bin']],
           default_left=[s0['default_left'], s1['default_left']],
           threshold=[EDGES[s0['feature']][s0['bin']], EDGES[s1['feature']][s1['bin']]],
           left_child=left_child, right_child=right_child, leaf_value=leaf_value)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gbdt_hand.json'), 'w') as fh:
    json.dump(out, fh, indent=1)
print(json.dumps({k: out[k] for k in ('grad', 'exp', 'qg', 'root_split', 'leaf0_split', 'leaf1_split', 'left_child', 'right_child', 'leaf_value')}))
