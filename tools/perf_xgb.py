"""Times of the XGBoost ranker family (include/otto_xgb.h) -> profiles/xgb/perf_xgb.json.

The rank:pairwise objective at 2^24 rows in queries of 50; one whole depth-wise tree at max_depth 6 on 2^24 rows x 54
features; and, for comparison, in the same job and alternated with it, the leaf-wise ``gbdt.grow_tree`` at num_leaves 64 on
the same bins and gradients with min_data_in_leaf 0 and the same hessian floor. Device events, 1 warm-up and 5 repeats,
median (min - max); the stream synchronisations per tree of both growers."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from otto_amd.ranker import gbdt, xgb

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1 << 24)
ap.add_argument('--features', type=int, default=54)
ap.add_argument('--query', type=int, default=50)
ap.add_argument('--max-depth', type=int, default=6)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=os.path.join('profiles', 'xgb', 'perf_xgb.json'))
a = ap.parse_args()


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


dev = torch.device('cuda:0')
n, F = a.rows, a.features
g = torch.Generator(device=dev).manual_seed(1)
off = torch.arange(0, n + a.query, a.query, dtype=torch.int64, device=dev).clamp_(max=n)
X = torch.randn((n, F), generator=g, device=dev)
score = 0.5 + 0.3 * X[:, 0].to(torch.float64)
# the label follows a few columns, so that the trees find real splits
label = ((X[:, 0] - 0.7 * X[:, 1] + 0.5 * X[:, 2].abs() + 0.8 * torch.randn(n, generator=g, device=dev)) > 1.6).to(torch.int32)
mapper = gbdt.fit_bins(X[:: max(n // 200000, 1)].cpu().numpy())
bins = gbdt.bin_matrix(X, mapper)
del X
seed = xgb.derived_seeds(0)[0]

objective = []
for r in range(a.repeats + 1):
    ms, (grad, hess) = event_ms(lambda: xgb.pairwise_gradients(score, label, off, seed, 0))
    if r:
        objective.append(ms)
gh, exp = gbdt.quantize_gradients(grad, hess)

px = xgb.resolve_params({'max_depth': a.max_depth})[0]
L = 1 << a.max_depth
pl = gbdt.resolve_params({'num_leaves': L, 'min_data_in_leaf': 0, 'min_sum_hessian_in_leaf': px['min_child_weight'],
                          'lambda_l2': px['lambda'], 'min_gain_to_split': px['gamma'], 'learning_rate': px['eta']})
work_x = torch.empty(xgb.workspace_bytes(n, F, a.max_depth), dtype=torch.uint8, device=dev)
work_l = torch.empty(gbdt.workspace_bytes(n, F, L), dtype=torch.uint8, device=dev)
depthwise, leafwise = [], []
for r in range(a.repeats + 1):                              # alternated: one tree of each per repeat
    ms_x, tx = event_ms(lambda: xgb.grow_tree(bins, gh, exp, mapper, px, work_x))
    ms_l, tl = event_ms(lambda: gbdt.grow_tree(bins, gh, exp, mapper, pl, work_l))
    if r:
        depthwise.append(ms_x)
        leafwise.append(ms_l)

out = dict(
    device=torch.cuda.get_device_name(0), rows=n, features=F, query=a.query, repeats=a.repeats,
    objective_ms=spread(objective),
    depthwise=dict(max_depth=a.max_depth, tree_ms=spread(depthwise), leaves=int(tx.n_leaves), hist_rows=int(tx.hist_rows),
                   stream_synchronisations=int(tx.n_syncs)),
    # otto_gbdt_grow_tree: one synchronisation for the root, one per split that searches its children (every split but
    # the one that fills num_leaves), one for the error words
    leafwise=dict(num_leaves=L, min_data_in_leaf=0, tree_ms=spread(leafwise), leaves=int(tl.n_leaves), hist_rows=int(tl.hist_rows),
                  stream_synchronisations=1 + max(tl.n_leaves - 1 - (1 if tl.n_leaves == L else 0), 0) + 1),
    split_params={k: px[k] for k in ('min_child_weight', 'lambda', 'gamma', 'eta')})
out['faster'] = 'depthwise' if out['depthwise']['tree_ms']['median'] < out['leafwise']['tree_ms']['median'] else 'leafwise'
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')
print(json.dumps(out))
