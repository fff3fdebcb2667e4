"""Time ``forest_predict`` and ``session_topk`` (csrc/otto_forest.hip) at ranker size and print one JSON line.

n_rows = 2^24 candidate rows, F = 54, a synthetic forest of T = 285 trees x 128 leaves whose split features follow the
frequencies of the 8-tree fixture (tests/golden/forest_order_fold1_head.lgb.txt) and whose thresholds are drawn from
that fixture's thresholds of the same feature; columns uniform over the fixture's feature_infos ranges; k = 20 over
sessions of 100 rows. hipEvents around each call, warm-up, several repeats, median. Node visits are counted exactly on
a 65,536-row sample (leaf depths of ``forest_leaves``) and scaled to n_rows. Needs a GPU; there is no fallback.

    python tools/perf_forest.py [--rows 16777216] [--trees 285] [--leaves 128] [--warmup 1] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12     # bytes / s, MI355X data sheet


def _time(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def synthetic_forest(head, T, L, rng):
    """Random binary trees (a random leaf is split each time) over the head fixture's split statistics."""
    from otto_amd.ranker.forest import Forest
    feats, counts = np.unique(head.split_feature, return_counts=True)
    by_feature = {int(f): head.threshold[head.split_feature == f] for f in feats}
    nint = L - 1
    sf = rng.choice(feats, size=T * nint, p=counts / counts.sum()).astype(np.int32)
    thr = np.array([rng.choice(by_feature[int(f)]) for f in sf], dtype=np.float64)
    dt = rng.choice(np.array([2, 2, 2, 2, 8, 10], dtype=np.int8), T * nint)
    lc, rc = np.zeros(T * nint, dtype=np.int32), np.zeros(T * nint, dtype=np.int32)
    for t in range(T):
        left, right = lc[t * nint:(t + 1) * nint], rc[t * nint:(t + 1) * nint]
        slots = [(-1, 0)]
        for i in range(nint):
            j = int(rng.integers(len(slots)))
            p, side = slots.pop(j)
            if p >= 0:
                (left if side == 0 else right)[p] = i
            slots[j:j] = [(i, 0), (i, 1)]
        for leaf, (p, side) in enumerate(slots):
            if p >= 0:
                (left if side == 0 else right)[p] = ~leaf
    off = np.arange(T + 1, dtype=np.int64)
    return Forest(off * nint, off * L, sf, thr, dt, lc, rc, rng.standard_normal(T * L) * 0.05, head.n_features)


def leaf_depths(forest):
    """depth[t][leaf] = internal nodes visited on the way to that leaf."""
    out = []
    for t in range(forest.n_trees):
        n0, L = int(forest.node_off[t]), int(forest.leaf_off[t + 1] - forest.leaf_off[t])
        d = np.zeros(L, dtype=np.int64)
        stack = [(0, 1)] if L > 1 else []
        while stack:
            i, depth = stack.pop()
            for c in (int(forest.left_child[n0 + i]), int(forest.right_child[n0 + i])):
                if c >= 0:
                    stack.append((c, depth + 1))
                else:
                    d[~c] = depth
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 24)
    ap.add_argument('--trees', type=int, default=285)
    ap.add_argument('--leaves', type=int, default=128)
    ap.add_argument('--session-rows', type=int, default=100)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_forest: no ROCm device visible (this tool does not fall back)')
    from otto_amd.ranker.forest import forest_leaves, forest_predict, load_lightgbm_model, session_topk
    dev = torch.device('cuda:0')
    path = os.path.join(ROOT, 'tests', 'golden', 'forest_order_fold1_head.lgb.txt')
    head = load_lightgbm_model(path)
    with open(path) as fh:
        infos = [l for l in fh.read().splitlines() if l.startswith('feature_infos=')][0].split('=', 1)[1].split()
    lo, hi = (torch.tensor([float(i.strip('[]').split(':')[j]) for i in infos], dtype=torch.float32, device=dev) for j in (0, 1))
    rng = np.random.default_rng(285)
    forest = synthetic_forest(head, args.trees, args.leaves, rng).to(dev)
    n, F = args.rows, head.n_features
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.rand((n, F), device=dev, generator=g) * (hi - lo) + lo

    sample = min(n, 1 << 16)
    leaf = forest_leaves(forest, X[:sample]).cpu().numpy()
    depth = leaf_depths(forest)
    visits_per_row = sum(float(depth[t][leaf[:, t]].mean()) for t in range(forest.n_trees))

    ms_p, all_p = _time(lambda: forest_predict(forest, X), args.warmup, args.repeats)
    raw = forest_predict(forest, X)
    S = (n + args.session_rows - 1) // args.session_rows
    row_off = torch.clamp(torch.arange(S + 1, dtype=torch.int64, device=dev) * args.session_rows, max=n)
    aid = torch.randint(0, 1855603, (n,), dtype=torch.int32, device=dev, generator=g)
    ms_t, all_t = _time(lambda: session_topk(raw, aid, row_off, k=args.k), args.warmup, args.repeats)
    print(json.dumps({
        'tool': 'perf_forest', 'device': torch.cuda.get_device_name(0), 'n_rows': n, 'F': F, 'trees': args.trees, 'leaves': args.leaves,
        'sessions': S, 'k': args.k, 'warmup': args.warmup, 'repeats': args.repeats,
        'predict_ms': round(ms_p, 3), 'predict_ms_all': [round(x, 3) for x in all_p],
        'topk_ms': round(ms_t, 3), 'topk_ms_all': [round(x, 3) for x in all_t],
        'node_visits_per_row': round(visits_per_row, 1), 'node_visits_per_s': round(visits_per_row * n / (ms_p * 1e-3), 0),
        'x_bytes_per_s': round(4.0 * n * F / (ms_p * 1e-3), 0), 'x_share_of_hbm_peak': round(4.0 * n * F / (ms_p * 1e-3) / HBM_PEAK, 4),
        'topk_rows_per_s': round(n / (ms_t * 1e-3), 0)}))


if __name__ == '__main__':
    main()
