"""Time the LambdaRank tree trainer (csrc/otto_gbdt.hip) at ranker size and print one JSON line.

n = 2^24 candidate rows x F = 54 float32 columns, queries of 50 rows, about 4 % positives that follow the columns,
num_leaves = 128, min_data_in_leaf = 2000: the shape of one fold of the reference's lgb.train. hipEvents around each
call, warm-up, several repeats, median and all values. Per boosting iteration: the objective, the quantisation, one whole
tree (histograms, split search, partition; one host round trip per split). The histogram kernel alone is timed on the
root (all rows, through a row list as a leaf's would be) and its rate is given over its algorithmic bytes, rows x (F bin
bytes + 8 bytes of packed (qg, qh) + 4 bytes of row id), as a share of the 8 TB/s HBM peak; ``hist_rows`` is what one
tree's histogram launches read in all (the smaller child of every split; the larger one is a subtraction).
``--cpu-rows`` also times tests/gbdt_restatement.py (NumPy, one core) on that many rows of the same data on this
machine's host: the CPU baseline. ``--trees-only N`` grows N trees and nothing else after the set-up: under
``rocprofv3 --kernel-trace --stats`` the total of ``k_hist`` is then those trees' histogram time, which over
``hist_algorithmic_bytes_per_tree`` gives the rate summed over the leaves actually built. Needs a GPU; there is no fallback.

``--bagging-fraction p`` / ``--feature-fraction q`` (SPEC-GBDT, Sampling): the tree is grown on the bag of draw 0 and the
feature list of iteration 0, ``bag_rows`` at n rows is timed as well, and ``--trees-only`` grows its trees with them.
``--only-tree`` times nothing but one whole tree after the set-up. ``--root DIR`` imports the package from another checkout
of this repository (built there): alternating ``--root <parent checkout> --only-tree`` with ``--only-tree`` in one job is how
two commits are compared, since kernel times move by several per cent with the chip's power state.

    python tools/perf_gbdt.py [--rows 16777216] [--features 54] [--leaves 128] [--min-data 2000] [--cpu-rows 262144]
                              [--bagging-fraction 0.9] [--feature-fraction 0.9] [--only-tree] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 24)
    ap.add_argument('--features', type=int, default=54)
    ap.add_argument('--leaves', type=int, default=128)
    ap.add_argument('--min-data', type=int, default=2000)
    ap.add_argument('--query-rows', type=int, default=50)
    ap.add_argument('--cpu-rows', type=int, default=0)
    ap.add_argument('--trees-only', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--bagging-fraction', type=float, default=1.0)
    ap.add_argument('--feature-fraction', type=float, default=1.0)
    ap.add_argument('--bagging-seed', type=int, default=3)
    ap.add_argument('--feature-fraction-seed', type=int, default=2)
    ap.add_argument('--only-tree', action='store_true')
    ap.add_argument('--root', default=ROOT)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_gbdt: no ROCm device visible (this tool does not fall back)')
    from otto_amd.ranker import gbdt
    dev = torch.device('cuda:0')
    n, F = args.rows, args.features
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((n, F), device=dev, generator=g)
    X[torch.rand((n, F), device=dev, generator=g) < 0.05] = float('nan')
    signal = torch.nan_to_num(X[:, 0]) - 0.7 * torch.nan_to_num(X[:, 1]) + 0.8 * torch.randn(n, device=dev, generator=g)
    label = (signal > 2.2).to(torch.int32)
    Q = (n + args.query_rows - 1) // args.query_rows
    query_off = torch.clamp(torch.arange(Q + 1, dtype=torch.int64, device=dev) * args.query_rows, max=n)
    mapper = gbdt.fit_bins(X[:200000].cpu().numpy())
    out = {'tool': 'perf_gbdt', 'device': torch.cuda.get_device_name(0), 'n_rows': n, 'F': F, 'num_leaves': args.leaves,
           'min_data_in_leaf': args.min_data, 'query_rows': args.query_rows, 'warmup': args.warmup, 'repeats': args.repeats}
    if root != ROOT:
        out['root'] = args.root
    if not args.only_tree:
        out['bin_ms'], out['bin_ms_all'] = _time(lambda: gbdt.bin_matrix(X, mapper), args.warmup, args.repeats)
    bins = gbdt.bin_matrix(X, mapper)
    p = gbdt.resolve_params({'num_leaves': args.leaves, 'min_data_in_leaf': args.min_data})
    score = torch.zeros(n, dtype=torch.float64, device=dev)
    grad, hess = torch.empty_like(score), torch.empty_like(score)
    obj = lambda: gbdt.lambdarank_gradients(score, label, query_off, p['sigmoid'], p['lambdarank_truncation_level'], True, out=(grad, hess))
    if args.only_tree:
        obj()
    else:
        out['objective_ms'], out['objective_ms_all'] = _time(obj, args.warmup, args.repeats)
        out['quantize_ms'], out['quantize_ms_all'] = _time(lambda: gbdt.quantize_gradients(grad, hess), args.warmup, args.repeats)
    gh, exp = gbdt.quantize_gradients(grad, hess)
    work = torch.empty(gbdt.workspace_bytes(n, F, args.leaves), dtype=torch.uint8, device=dev)
    sampled = {}
    if args.bagging_fraction < 1.0 or args.feature_fraction < 1.0:
        out['bagging_fraction'], out['feature_fraction'] = args.bagging_fraction, args.feature_fraction
        if args.bagging_fraction < 1.0:
            m, seed = gbdt.bag_size(args.bagging_fraction, n), gbdt.mix(args.bagging_seed, 0)
            if not args.trees_only:
                out['bag_rows_ms'], out['bag_rows_ms_all'] = _time(lambda: gbdt.bag_rows(n, m, seed, dev), args.warmup, args.repeats)
            sampled['bag'] = gbdt.bag_rows(n, m, seed, dev)
            out['bag_size'] = m
        if args.feature_fraction < 1.0:
            # the device list, made once: a tree of the boosting loop pays one small host-to-device copy for it
            feats = gbdt.sample_features(F, args.feature_fraction, args.feature_fraction_seed, 0)
            sampled['features'] = torch.from_numpy(feats).to(dev)
            out['n_used'] = int(feats.size)
    grow = lambda: gbdt.grow_tree(bins, gh, exp, mapper, p, work, **sampled)
    if args.trees_only:
        # for a kernel trace: nothing but this many trees launches k_hist, so its traced total is theirs
        for _ in range(args.trees_only):
            tree = grow()
        torch.cuda.synchronize()
        print(json.dumps({'tool': 'perf_gbdt', 'trees_only': args.trees_only, 'n_rows': n, 'F': F, 'tree_leaves': tree.n_leaves,
                          'bagging_fraction': args.bagging_fraction, 'feature_fraction': args.feature_fraction,
                          'hist_rows_per_tree': tree.hist_rows, 'hist_algorithmic_bytes_per_tree': tree.hist_rows * (F + 8 + 4)}))
        return
    out['tree_ms'], out['tree_ms_all'] = _time(grow, args.warmup, args.repeats)
    tree = grow()
    out['tree_leaves'], out['hist_rows'] = tree.n_leaves, tree.hist_rows
    if args.only_tree:
        print(json.dumps(out))
        return
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    out['root_hist_ms'], out['root_hist_ms_all'] = _time(lambda: gbdt.leaf_histogram(bins, gh, rows), args.warmup, args.repeats)
    per_row = F + 8 + 4
    out['root_hist_bytes_per_s'] = round(n * per_row / (out['root_hist_ms'] * 1e-3), 0)
    out['root_hist_share_of_hbm_peak'] = round(out['root_hist_bytes_per_s'] / HBM_PEAK, 4)
    out['tree_hist_algorithmic_bytes'] = tree.hist_rows * per_row
    out['add_tree_ms'], out['add_tree_ms_all'] = _time(lambda: gbdt.add_tree(bins, tree, score), args.warmup, args.repeats)
    if args.cpu_rows:
        import gbdt_restatement as gr
        m = min(args.cpu_rows, n) // args.query_rows * args.query_rows
        bins_np, label_np = bins[:, :m].cpu().numpy(), label[:m].cpu().numpy()
        off_np = np.arange(0, m + 1, args.query_rows, dtype=np.int64)
        edge_list = [mapper.feature_edges(f) for f in range(F)]
        t0 = time.perf_counter()
        g_np, h_np, _ = gr.lambdarank(np.zeros(m), label_np, off_np)
        t1 = time.perf_counter()
        q_np, exps = gr.quantize(g_np, h_np)
        t2 = time.perf_counter()
        t_np = gr.grow_tree(bins_np, q_np, exps, edge_list, dict(p, min_data_in_leaf=args.min_data))
        t3 = time.perf_counter()
        out['cpu_baseline'] = {'what': 'tests/gbdt_restatement.py, NumPy, one core, one run', 'rows': m,
                               'objective_ms': round((t1 - t0) * 1e3, 1), 'quantize_ms': round((t2 - t1) * 1e3, 1),
                               'tree_ms': round((t3 - t2) * 1e3, 1), 'tree_leaves': int(t_np['leaf_value'].size)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
