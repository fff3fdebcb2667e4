"""Time the SPEC-EVAL calls (csrc/otto_eval.hip) at the validation week's size and print one JSON line.

Default shape: 1.8 M sessions with OTTO-like lengths (geometric body, one session in 200 drawn from 65..499, about 6
events on average), types 0.88 / 0.09 / 0.03; hits over 1.8 M x 20 padded rows for three types and 1.8 M x 100 CSR rows. hipEvents around each
call (the call's one stream synchronisation is inside the bracket), warm-up, repeats, median with min - max. The bytes a
call MUST move:

    cutoffs        E + 8 S + 4 S                      (typ once, sess_off, cutoff out)
    split          9 E + 12 S  +  9 kept + 4 labels + 32 S   (events once, sess_off + cutoff; kept events, label aids and the
                                                              four offset arrays written once; the count pass reads again)
    hits           4 (P k or R) + 8 S + 4 L + 8 S     (rows once, label offsets and aids, hits + denom out)

The only comparison stated: ``metrics.recall_at_20`` over Python lists of the same top-20 and labels, timed once on this
host (``--host-sessions`` caps the sessions it is given; 0 skips it). Needs a GPU; there is no fallback.

    python tools/perf_eval.py [--sessions 1800000] [--warmup 1] [--repeats 5] [--out profiles/eval/perf_eval.json]
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
    return {'ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'all_ms': ms}


def _with_bytes(t, must):
    t['must_move_bytes'] = int(must)
    t['share_of_hbm_peak'] = must / (t['ms'] * 1e-3) / HBM_PEAK
    return t


def make_events(S, n_aids, seed):
    rng = np.random.default_rng(seed)
    n = np.minimum(rng.geometric(0.25, S) + 1, 64)
    long = rng.random(S) < 0.005
    n[long] = rng.integers(65, 500, int(long.sum()))
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    E = int(off[-1])
    aid = rng.integers(0, n_aids, E).astype(np.int32)
    typ = rng.choice(3, E, p=(0.88, 0.09, 0.03)).astype(np.uint8)
    ts = np.arange(E, dtype=np.int32)
    return aid, ts, typ, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=1_800_000)
    ap.add_argument('--aids', type=int, default=1_855_603)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-sessions', type=int, default=1_800_000, help='sessions given to the host recall loop (0: skip)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval', 'perf_eval.json'), help="where the JSON line is also written ('' : nowhere)")
    args = ap.parse_args()

    import torch
    from otto_amd import metrics
    from otto_amd.events import DeviceEvents
    from otto_amd.ranker import evaluate as ev

    dev = torch.device('cuda:0')
    S = args.sessions
    aid, ts, typ, off = make_events(S, args.aids, 1)
    E = len(aid)
    t = lambda a: torch.from_numpy(a).to(dev)
    events = DeviceEvents(t(aid), t(ts), t(typ), t(off), None, None, args.aids)
    res = {'sessions': S, 'events': E, 'warmup': args.warmup, 'repeats': args.repeats, 'hbm_peak_bytes_per_s': HBM_PEAK}

    res['cutoffs'] = _with_bytes(_time(lambda: ev.cutoffs(events, 7), args.warmup, args.repeats), E + 12 * S)
    cut, without = ev.cutoffs(events, 7)
    res['sessions_without_click'] = without
    kept, labels = ev.split(events, cut)
    n_lab = sum(int(labels[n][1].numel()) for n in ev.TYPES)
    res['kept_events'], res['labels'] = kept.n_events, {n: int(labels[n][1].numel()) for n in ev.TYPES}
    res['split'] = _with_bytes(_time(lambda: ev.split(events, cut), args.warmup, args.repeats),
                               9 * E + 12 * S + 9 * kept.n_events + 4 * n_lab + 32 * S)

    g = torch.Generator(device=dev)
    g.manual_seed(3)
    top = {}
    for n in ev.TYPES:                                   # 20 random aids per session, the label planted in a third of the rows
        p = torch.randint(0, args.aids, (S, 20), device=dev, generator=g, dtype=torch.int32)
        o, a = labels[n]
        has = torch.nonzero((o[1:] - o[:-1]) > 0).flatten()[::3]
        p[has, 5] = a[o[has]]
        top[n] = p
    res['hits_padded_3_types'] = _with_bytes(_time(lambda: ev.evaluate(top, labels), args.warmup, args.repeats),
                                             3 * (80 * S + 16 * S) + 4 * n_lab)
    res['recall'] = ev.evaluate(top, labels)
    rows = torch.randint(0, args.aids, (S * 100,), device=dev, generator=g, dtype=torch.int32)
    row_off = torch.arange(S + 1, device=dev, dtype=torch.int64) * 100
    res['hits_csr_100'] = _with_bytes(_time(lambda: ev.hits(labels['carts'], (row_off, rows), cap=None), args.warmup, args.repeats),
                                      400 * S + 24 * S + 4 * int(labels['carts'][1].numel()))
    del rows, row_off

    if args.host_sessions:
        m = min(S, args.host_sessions)
        host = {}
        for n in ev.TYPES:
            o, a = (x.cpu().numpy() for x in labels[n])
            host[n] = (top[n][:m].cpu().numpy().tolist(), [a[o[s]:o[s + 1]].tolist() for s in range(m)])
        t0 = time.perf_counter()
        r = {n: metrics.recall_at_20(*host[n]) for n in ev.TYPES}
        t1 = time.perf_counter()
        res['host_recall_at_20'] = {'sessions': m, 'ms': (t1 - t0) * 1e3, 'recall': r,
                                    'note': 'metrics.recall_at_20 over Python lists, three types, timed once; the conversion of '
                                            'the device arrays to lists is not counted'}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
