"""Time the three SPEC-BLEND calls (csrc/otto_blend.hip) at inference size and print one JSON line.

Default shape: 4 models x 2^26 rows over 2^20 sessions; every model draws its keys from one universe of
rows / overlap keys, so about ``overlap`` (0.7) of a model's keys are in any other model; model 1 is left_of_base, the
reference's click weights. hipEvents around each call, warm-up, several repeats, median. The bytes a call MUST move:

    robust_stats   8 n        (one read of the float64 column; the select reads it 8 times)
    scale          12 n       (read float64, write float32)
    join           12 N + 12 R  (read session, aid, score of all N rows; write aid, pred, pred64-less rows and the CSR)

Beside it, as context only, the same shape through the pandas merge path on this host (``--pandas-rows`` caps the rows
per model it is given; 0 skips it). Needs a GPU; there is no fallback.

    python tools/perf_blend.py [--models 4] [--rows 67108864] [--sessions 1048576] [--overlap 0.7] [--warmup 1] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12     # bytes / s, MI355X data sheet
CLICK_WEIGHTS = (0.05, 0.05, 0.70, 0.20)


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


def make_model(dev, rows, universe, per_session, seed):
    """rows distinct keys out of ``universe``, on the device: key u -> (session u // per_session, aid u % per_session)."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randperm(universe, device=dev, generator=g)[:rows]          # a random subset, in random order
    score = torch.randn(u.numel(), device=dev, generator=g, dtype=torch.float64)
    return (u // per_session).to(torch.int32), (u % per_session).to(torch.int32), score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', type=int, default=4)
    ap.add_argument('--rows', type=int, default=1 << 26, help='rows per model')
    ap.add_argument('--sessions', type=int, default=1 << 20)
    ap.add_argument('--overlap', type=float, default=0.7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--pandas-rows', type=int, default=1 << 21, help='rows per model given to the pandas path (0: skip)')
    args = ap.parse_args()

    import torch
    from otto_amd.ranker import blend

    dev = torch.device('cuda:0')
    M, n = args.models, args.rows
    universe = int(round(n / args.overlap))
    per_session = -(-universe // args.sessions)
    weights = (CLICK_WEIGHTS * 2)[:M]
    left = [0, 1] + [0] * (M - 2) if M >= 2 else [0]
    models = [make_model(dev, n, universe, per_session, 100 + m) for m in range(M)]

    res = {'models': M, 'rows_per_model': n, 'sessions': args.sessions, 'overlap': args.overlap, 'warmup': args.warmup,
           'repeats': args.repeats, 'hbm_peak_bytes_per_s': HBM_PEAK}
    x = models[0][2]
    ms, all_ms = _time(lambda: blend.robust_stats(x), args.warmup, args.repeats)
    res['robust_stats'] = {'ms': ms, 'all_ms': all_ms, 'must_move_bytes': 8 * n, 'share_of_hbm_peak': 8 * n / (ms * 1e-3) / HBM_PEAK}
    nv, stats = blend.robust_stats(x)
    center, scale = blend.center_scale(nv, stats)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    from otto_amd import _lib
    ms, all_ms = _time(lambda: _lib.call('otto_blend_scale', dev, x, n, center, scale, out), args.warmup, args.repeats)
    res['scale'] = {'ms': ms, 'all_ms': all_ms, 'must_move_bytes': 12 * n, 'share_of_hbm_peak': 12 * n / (ms * 1e-3) / HBM_PEAK}
    del out

    scaled = [(s, a, blend.robust_scale(v)[0]) for s, a, v in models]
    del models, x
    R = [0]

    def join():
        R[0] = blend.blend_predictions(scaled, weights, left, scale=False)[2].numel()
    ms, all_ms = _time(join, args.warmup, args.repeats)
    must = 12 * M * n + 12 * R[0]
    res['join'] = {'ms': ms, 'all_ms': all_ms, 'rows_in': M * n, 'rows_out': R[0], 'must_move_bytes': must,
                   'share_of_hbm_peak': must / (ms * 1e-3) / HBM_PEAK}
    ms, all_ms = _time(lambda: blend.blend_topk(scaled, weights, left, k=20, scale=False), args.warmup, max(1, args.repeats // 2))
    res['join_and_top20'] = {'ms': ms, 'all_ms': all_ms}

    if args.pandas_rows:
        try:
            import pandas as pd
            from sklearn.preprocessing import RobustScaler
            pn = min(n, args.pandas_rows)
            frames = [pd.DataFrame({'session': s[:pn].cpu().numpy(), 'aid': a[:pn].cpu().numpy(), f'p{m}': v[:pn].cpu().numpy()})
                      for m, (s, a, v) in enumerate(scaled)]
            t0 = time.perf_counter()
            RobustScaler().fit_transform(frames[0][['p0']].to_numpy().astype(np.float64))
            t1 = time.perf_counter()
            df = frames[0]
            for m in range(1, M):
                df = df.merge(frames[m], how='left' if left[m] else 'outer', on=['session', 'aid'])
            df = df.fillna(0)
            df['p'] = sum(df[f'p{m}'] * weights[m] for m in range(M))
            df = df.sort_values(['session', 'p'], ascending=[True, False]).groupby('session').head(20)
            t2 = time.perf_counter()
            res['pandas_context'] = {'rows_per_model': pn, 'robust_scaler_one_column_ms': (t1 - t0) * 1e3,
                                     'merge_weight_sort_head20_ms': (t2 - t1) * 1e3,
                                     'note': 'the first rows_per_model rows of every model, on this host: context only, not the same size'}
        except ImportError as e:
            res['pandas_context'] = f'not measured: {e}'
    print(json.dumps(res))


if __name__ == '__main__':
    main()
