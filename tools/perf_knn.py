"""Time ``neighbour_table`` (csrc/otto_knn.hip) at OTTO size and print one JSON line.

N = 1,855,603 aids, d in {32, 64}, k = 45, euclidean; all rows and a 783,486-row query subset (the number of distinct
test aids). hipEvents around each call, warm-up, several repeats, median. TFLOP/s = 2 R N d / t,
and that as a share of what ``k_score`` (``score_topk``, k = 32, its widest list) reaches in the same process on a
4096-row batch of the same d. Needs a GPU; there is no fallback.

    python tools/perf_knn.py [--n-aids N] [--dims 32 64] [--k 45] [--warmup 1] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-aids', type=int, default=1855603)
    ap.add_argument('--subset', type=int, default=783486)
    ap.add_argument('--dims', type=int, nargs='+', default=[32, 64])
    ap.add_argument('--k', type=int, default=45)
    ap.add_argument('--metric', default='euclidean')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_knn: no ROCm device visible (this tool does not fall back)')
    from otto_amd.matrix_factorization.engine import score_topk
    from otto_amd.matrix_factorization.neighbours import neighbour_table
    dev = torch.device('cuda:0')
    N = args.n_aids
    g = torch.Generator(device=dev).manual_seed(1)
    out = {'tool': 'perf_knn', 'device': torch.cuda.get_device_name(0), 'n_aids': N, 'k': args.k, 'metric': args.metric,
           'warmup': args.warmup, 'repeats': args.repeats, 'runs': []}
    for d in args.dims:
        E = torch.randn((N, d), device=dev, generator=g)
        U = E[torch.randperm(N, device=dev, generator=g)[:4096]].contiguous()
        ms_s, _ = _time(lambda: score_topk(U, E, k=32), max(args.warmup, 2), max(args.repeats, 5))
        tf_s = 2.0 * 4096 * N * d / (ms_s * 1e-3) / 1e12
        subset = torch.randperm(N, device=dev, generator=g)[:min(args.subset, N)].to(torch.int32).contiguous()
        for name, rows in (('all', None), ('subset', subset)):
            R = N if rows is None else rows.numel()
            ms, all_ms = _time(lambda: neighbour_table(E, k=args.k, metric=args.metric, rows=rows), args.warmup, args.repeats)
            tf = 2.0 * R * N * d / (ms * 1e-3) / 1e12
            out['runs'].append({'d': d, 'rows': name, 'n_rows': R, 'ms': round(ms, 2), 'ms_all': [round(x, 2) for x in all_ms],
                                'tflops': round(tf, 2), 'k_score_4096_ms': round(ms_s, 3), 'k_score_tflops': round(tf_s, 2),
                                'share_of_k_score': round(tf / tf_s, 3)})
        del E, U, subset
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
