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

    python tools/perf_gbdt.py [--rows 16777216] [--features 54] [--leaves 128] [--min-data 2000] [--cpu-rows 262144]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
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
    args = ap.parse_args()
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
    out['bin_ms'], out['bin_ms_all'] = _time(lambda: gbdt.bin_matrix(X, mapper), args.warmup, args.repeats)
    bins = gbdt.bin_matrix(X, mapper)
    p = gbdt.resolve_params({'num_leaves': args.leaves, 'min_data_in_leaf': args.min_data})
    score = torch.zeros(n, dtype=torch.float64, device=dev)
    grad, hess = torch.empty_like(score), torch.empty_like(score)
    obj = lambda: gbdt.lambdarank_gradients(score, label, query_off, p['sigmoid'], p['lambdarank_truncation_level'], True, out=(grad, hess))
    out['objective_ms'], out['objective_ms_all'] = _time(obj, args.warmup, args.repeats)
    out['quantize_ms'], out['quantize_ms_all'] = _time(lambda: gbdt.quantize_gradients(grad, hess), args.warmup, args.repeats)
    gh, exp = gbdt.quantize_gradients(grad, hess)
    work = torch.empty(gbdt.workspace_bytes(n, F, args.leaves), dtype=torch.uint8, device=dev)
    if args.trees_only:
        # for a kernel trace: nothing but this many trees launches k_hist, so its traced total is theirs
        for _ in range(args.trees_only):
            tree = gbdt.grow_tree(bins, gh, exp, mapper, p, work)
        torch.cuda.synchronize()
        print(json.dumps({'tool': 'perf_gbdt', 'trees_only': args.trees_only, 'n_rows': n, 'F': F, 'tree_leaves': tree.n_leaves,
                          'hist_rows_per_tree': tree.hist_rows, 'hist_algorithmic_bytes_per_tree': tree.hist_rows * (F + 8 + 4)}))
        return
    out['tree_ms'], out['tree_ms_all'] = _time(lambda: gbdt.grow_tree(bins, gh, exp, mapper, p, work), args.warmup, args.repeats)
    tree = gbdt.grow_tree(bins, gh, exp, mapper, p, work)
    out['tree_leaves'], out['hist_rows'] = tree.n_leaves, tree.hist_rows
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
