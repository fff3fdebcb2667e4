"""GRU4Rec on the synthetic shape the other perf tools use: 2 M sessions of `synth.py`, batch 2048, L 50,
at De 64 / H 128 and De 32 / H 32. Each of the four calls (plan, encode, grad, apply) per step, three fresh processes each;
encode + `score_topk` for 4096 sessions; against the same training step in torch on the host CPU (`nn.GRU` + autograd +
`optim.Adam`, dense over the whole item table as RecBole runs it) at its best thread count.

    python tools/perf_gru.py [--sessions 2000000] [--out profiles/gru/perf_gru.json]

Device: hipEvents, 2 warm-up + 10 steps per process, the median step of every process, then the median (min - max) of the three
processes. The plan is one call per epoch and is timed as such. Host: 1 warm-up + 3 steps at 1, 4, 8 and 16 threads. The
library must be built before (`__graft_entry__.build()`).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((64, 128), (32, 32))
BATCH, L, TOPK_SESSIONS = 2048, 50, 4096


def events_on(dev, n):
    from otto_amd.synth import generate_sessions_torch
    ev = generate_sessions_torch(n, device=dev)

    class Ev:
        aid, type, sess_off, n_aids = ev['aid'], ev['type'], ev['sess_off'], ev['n_aids']
    return Ev


def device_child(n_sessions, De, H, dev):
    import torch
    from otto_amd.recbole.gru4rec import GRU4Rec
    ev = events_on(dev, n_sessions)
    model = GRU4Rec(ev.n_aids, De, H).to(dev)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize(dev)
        return got, e0.elapsed_time(e1)
    plan, plan_ms = None, []
    for epoch in range(3):
        plan, ms = timed(lambda: model.plan_epoch(ev, 42, epoch, L))
        plan_ms.append(ms)
    enc, grd, app, steps = [], [], [], []
    for q in range(12):
        b = slice(q * BATCH, (q + 1) * BATCH)
        args = (ev.aid, plan.seq_lo[b], plan.seq_len[b])
        _, ms = timed(lambda: model.encode(*args, L))
        enc.append(ms)
        g, ms = timed(lambda: model.grad(*args, plan.target[b], plan.neg[b], L))
        grd.append(ms)
        _, ms = timed(lambda: model.apply(g))
        app.append(ms)
        steps.append(int(plan.seq_len[b].sum()))
    sub = slice(0, TOPK_SESSIONS + 1)
    off = ev.sess_off[sub]

    class Few:
        aid, sess_off, n_aids = ev.aid, off.contiguous(), ev.n_aids
    top = [timed(lambda: model.full_sort_topk(model.encode_sessions(Few, L), 20))[1] for _ in range(4)]
    med = lambda x: float(np.median(x[2:]))
    return {'De': De, 'H': H, 'samples': len(plan), 'events': int(ev.aid.numel()), 'n_aids': ev.n_aids, 'plan_ms': float(np.median(plan_ms[1:])),
            'encode_ms': med(enc), 'grad_ms': med(grd), 'apply_ms': med(app), 'steps_per_batch': float(np.mean(steps[2:])),
            'encode_topk_ms': float(np.median(top[1:])), 'list_rows': int(g.count[0])}


def host_child(n_sessions, De, H, threads, dev):
    """the same step in torch on the CPU: padded batch, nn.GRU, BPR loss, autograd, optim.Adam over every parameter"""
    import torch
    from otto_amd.recbole.gru4rec import GRU4Rec
    ev = events_on(dev, n_sessions)
    model = GRU4Rec(ev.n_aids, De, H).to(dev)
    plan = model.plan_epoch(ev, 42, 0, L)
    aid = ev.aid.cpu()
    lo, n, tgt, neg = (x[:4 * BATCH].cpu().long() for x in (plan.seq_lo, plan.seq_len, plan.target, plan.neg))
    torch.set_num_threads(threads)
    E = torch.nn.Embedding(ev.n_aids + 1, De, padding_idx=0)
    gru, lin = torch.nn.GRU(De, H, bias=False, batch_first=True), torch.nn.Linear(H, De)
    opt = torch.optim.Adam(list(E.parameters()) + list(gru.parameters()) + list(lin.parameters()), lr=1e-3)
    ms = []
    for q in range(4):
        b = slice(q * BATCH, (q + 1) * BATCH)
        t0 = time.perf_counter()
        idx = lo[b, None] + torch.arange(L)[None, :]
        rows = torch.where(torch.arange(L)[None, :] < n[b, None], aid[idx.clamp(max=aid.numel() - 1)].long() + 1, 0)
        out, _ = gru(E(rows))
        o = lin(out[torch.arange(rows.shape[0]), n[b] - 1])
        x = (o * E(tgt[b] + 1)).sum(-1) - (o * E(neg[b] + 1)).sum(-1)
        loss = -torch.log(1e-10 + torch.sigmoid(x)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {'De': De, 'H': H, 'threads': threads, 'step_ms': float(np.median(ms[1:]))}


def run_child(*argv):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *map(str, argv)], stdout=subprocess.PIPE, text=True, check=True, timeout=900)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=2_000_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gru', 'perf_gru.json'))
    ap.add_argument('--child', choices=('device', 'host'))
    ap.add_argument('--shape', type=int, nargs=2, default=SHAPES[0])
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import torch
    from otto_amd import _lib
    _lib.lib()
    dev = torch.device('cuda:0')
    if args.child == 'device':
        print(json.dumps(device_child(args.sessions, *args.shape, dev)))
        return
    if args.child == 'host':
        print(json.dumps(host_child(args.sessions, *args.shape, args.threads, dev)))
        return
    res = {'device': torch.cuda.get_device_name(0), 'sessions': args.sessions, 'batch': BATCH, 'L': L, 'shapes': []}
    for De, H in SHAPES:
        runs = [run_child('--child', 'device', '--sessions', args.sessions, '--shape', De, H) for _ in range(3)]
        entry = dict(runs[0])
        for key in ('plan_ms', 'encode_ms', 'grad_ms', 'apply_ms', 'encode_topk_ms'):
            vals = [r[key] for r in runs]
            entry[key] = {'median': float(np.median(vals)), 'min': min(vals), 'max': max(vals)}
        entry['step_ms'] = entry['grad_ms']['median'] + entry['apply_ms']['median']
        if not args.no_host:
            entry['host'] = [run_child('--child', 'host', '--sessions', args.sessions, '--shape', De, H, '--threads', t) for t in (1, 4, 8, 16)]
            entry['host_best_step_ms'] = min(h['step_ms'] for h in entry['host'])
            entry['speedup'] = entry['host_best_step_ms'] / entry['step_ms']
        res['shapes'].append(entry)
        print(json.dumps(entry, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
