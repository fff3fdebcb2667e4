"""Time the fold machinery (csrc/otto_folds.hip) at ranker size and print one JSON line.

n = 2^24 candidate rows, queries of 50 rows, about 4 % positives, F = 54 bin columns, 5 folds, negative sampling ratio
0.3: the shape of one event type of the reference's fold loop. hipEvents around each call, warm-up, several repeats,
median with min and max. ``group_kfold`` is timed whole and its sequential walk on its own (the library brackets that one
kernel with events); ``fold_indices`` for fold 0; ``gather_bins`` of that fold's training rows. Each is given over its
algorithmic bytes as a share of the 8 TB/s HBM peak:

  gather      read F * (m + touched 64-byte lines * 64) + 4 m, written F * m
  index sets  per row: the label (1 byte) read, the state byte cleared, written and read by the 8 select passes, the
              count pass and the emit pass (1 + 2 + 8 + 1 + 1 bytes); per query 16 bytes of offsets in each of the three
              per-query kernels, 4 + 2 * 8 bytes of counts and scans written and read; 4 bytes per emitted row id
  fold walk   per query 16 bytes of offsets twice, 2 + 4 bytes placed, 2 + 1 bytes walked, 4 + 1 + 4 bytes scattered

``--host`` also times, once each on this machine's host, scikit-learn's GroupKFold over the same groups, pandas'
``sample(frac=0.3, random_state=42)`` over the eligible negatives and the NumPy fancy index ``bins[:, idx]``, if they can
be imported. Needs a GPU; there is no fallback.

    python tools/perf_folds.py [--rows 16777216] [--features 54] [--query-rows 50] [--host] [--out profiles/folds/perf_folds.json]
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
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def _rate(entry, n_bytes):
    entry['algorithmic_bytes'] = int(n_bytes)
    entry['bytes_per_s'] = round(n_bytes / (entry['median_ms'] * 1e-3), 0)
    entry['share_of_hbm_peak'] = round(entry['bytes_per_s'] / HBM_PEAK, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 24)
    ap.add_argument('--features', type=int, default=54)
    ap.add_argument('--query-rows', type=int, default=50)
    ap.add_argument('--splits', type=int, default=5)
    ap.add_argument('--ratio', type=float, default=0.3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_folds: no ROCm device visible (this tool does not fall back)')
    from otto_amd.ranker import folds
    dev = torch.device('cuda:0')
    n, F, k = args.rows, args.features, args.splits
    g = torch.Generator(device=dev).manual_seed(1)
    label = (torch.rand(n, device=dev, generator=g) < 0.04).to(torch.uint8)
    Q = (n + args.query_rows - 1) // args.query_rows
    query_off = torch.clamp(torch.arange(Q + 1, dtype=torch.int64, device=dev) * args.query_rows, max=n)
    bins = torch.randint(0, 256, (F, n), dtype=torch.uint8, device=dev, generator=g)
    out = {'tool': 'perf_folds', 'device': torch.cuda.get_device_name(0), 'n_rows': n, 'Q': Q, 'F': F, 'n_splits': k,
           'ratio': args.ratio, 'query_rows': args.query_rows, 'warmup': args.warmup, 'repeats': args.repeats}

    walks = []

    def kfold():
        t = {}
        r = folds.group_kfold(query_off, k, n=n, timing=t)
        walks.append(t['walk_ms'])
        return r
    out['group_kfold'] = _time(kfold, args.warmup, args.repeats)
    _rate(out['group_kfold'], Q * (2 * 16 + 6 + 3 + 9))
    w = walks[args.warmup:]
    out['group_kfold_walk'] = {'median_ms': round(statistics.median(w), 3), 'min_ms': round(min(w), 3), 'max_ms': round(max(w), 3),
                               'ns_per_query': round(statistics.median(w) * 1e6 / Q, 2)}
    fold_of_query, fold_rows = kfold()
    out['fold_rows'] = fold_rows.cpu().tolist()

    out['fold_indices'] = _time(lambda: folds.fold_indices(label, query_off, fold_of_query, 0, args.ratio, 42), args.warmup, args.repeats)
    fi = folds.fold_indices(label, query_off, fold_of_query, 0, args.ratio, 42)
    Mt, Mv = fi.train_idx.numel(), fi.val_idx.numel()
    out.update(n_eligible=fi.n_eligible, n_kept=fi.n_kept, train_rows=Mt, val_rows=Mv, train_queries=fi.train_query.numel())
    _rate(out['fold_indices'], n * (1 + 2 + 8 + 1 + 1) + Q * (3 * 16 + 2 * (4 + 16)) + 4 * (Mt + Mv))

    out['gather_bins'] = _time(lambda: folds.gather_bins(bins, fi.train_idx), args.warmup, args.repeats)
    lines = int(torch.unique(fi.train_idx >> 6).numel())
    out['gather_touched_lines_per_feature'] = lines
    _rate(out['gather_bins'], F * (Mt + lines * 64) + 4 * Mt + F * Mt)

    if args.host:
        host = {}
        off_np, label_np = query_off.cpu().numpy(), label.cpu().numpy()
        try:
            from sklearn.model_selection import GroupKFold
            groups = np.repeat(np.arange(Q), np.diff(off_np))
            t0 = time.perf_counter()
            for _ in GroupKFold(n_splits=k).split(np.zeros((n, 1), dtype=np.uint8), groups=groups):
                pass
            host['sklearn_group_kfold_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        except ImportError:
            host['sklearn_group_kfold_ms'] = 'scikit-learn cannot be imported here'
        try:
            import pandas as pd
            t0 = time.perf_counter()
            kept = pd.Series(np.zeros(fi.n_eligible, dtype=np.uint8)).sample(frac=args.ratio, random_state=42)
            host['pandas_sample_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            host['pandas_sample_rows'] = len(kept)
        except ImportError:
            host['pandas_sample_ms'] = 'pandas cannot be imported here'
        bins_np, idx_np = bins.cpu().numpy(), fi.train_idx.cpu().numpy()
        t0 = time.perf_counter()
        bins_np[:, idx_np]
        host['numpy_fancy_index_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        host['what'] = 'one run each, one process, on the host of the GPU machine'
        out['host'] = host
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
