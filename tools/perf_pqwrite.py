"""Device-side Parquet encode: `otto_pqw_plan` / `otto_pqw_emit` alone, and the builder's write leg end
to end against the existing host path, on one row set of 2^25 rows with the README's column shapes -- aid_x runs of 20 over
sorted distinct aids, aid_y uniform below 1,855,603, 16.16 fixed-point weights -- cut into the 6 parts of a `top_<kind>` set.

    python tools/perf_pqwrite.py [--aids 1677722] [--out profiles/pqwrite/perf_pqwrite.json]

Kernels: hipEvents around each call, 1 warm-up + 5 repeats, median (min - max). End to end: `engine.topk_to_device_rows` +
`builder.write_device_parts` against `engine.topk_to_rows` + `builder.write_jobs` on the same dense top-k, alternating, three
fresh processes each (`--child device|host`), wall time from the dense tensors to the closed files; file bytes per row of both.
"""
import argparse
import json
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_AIDS, K, PARTS = 1855603, 20, 6


def dense_topk(aids, dev):
    """(y int32 [n_aids, K], w int64 [n_aids, K], n int32 [n_aids]): `aids` distinct sorted aids hold K neighbours each."""
    import torch
    g = torch.Generator(device=dev).manual_seed(11)
    rows = torch.randperm(N_AIDS, device=dev, generator=g)[:aids].sort().values
    n = torch.zeros(N_AIDS, dtype=torch.int32, device=dev)
    n[rows] = K
    y = torch.randint(0, N_AIDS, (N_AIDS, K), dtype=torch.int32, device=dev, generator=g)
    w = torch.randint(1, 1 << 30, (N_AIDS, K), dtype=torch.int64, device=dev, generator=g)
    return y, w, n


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def kernels(aids, dev):
    import torch
    from otto_amd import parquet_write as pw
    from otto_amd.covisitation import builder, engine
    aid_x, aid_y, wgt = engine.topk_to_device_rows(*dense_topk(aids, dev))
    rows = int(aid_x.numel())
    lay = pw.Layout(3, builder.split_parts_device(aid_x, PARTS, N_AIDS), pw.PAGE_ROWS, pw.ROW_GROUP_ROWS)
    job = pw.DeviceJob([aid_x, aid_y, wgt], [pw.DELTA, pw.DELTA, pw.PLAIN], lay.pages)
    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize(dev)
        return got, e0.elapsed_time(e1)
    plan_ms, emit_ms = [], []
    for rep in range(6):                                      # 1 warm-up + 5
        page_bytes, ms = timed(job.plan)
        plan_ms.append(ms)
    dst = np.r_[0, np.cumsum(page_bytes)[:-1]]
    out = torch.empty(int(page_bytes.sum()), dtype=torch.uint8, device=dev)
    for rep in range(6):
        emit_ms.append(timed(lambda: job.emit(dst, out))[1])
    plan_ms, emit_ms = plan_ms[1:], emit_ms[1:]
    by_col = {name: int(page_bytes[lay.pages['column'] == j].sum()) for j, name in enumerate(('aid_x', 'aid_y', 'wgt'))}
    read_plan, read_emit, written = 8 * rows, 12 * rows, int(page_bytes.sum())
    res = {'rows': rows, 'pages': int(len(lay.pages)), 'body_bytes': written, 'body_bytes_per_row': {k: v / rows for k, v in by_col.items()},
           'otto_pqw_plan': summary(plan_ms), 'otto_pqw_emit': summary(emit_ms)}
    res['otto_pqw_plan']['GBps_read'] = read_plan / np.median(plan_ms) / 1e6
    res['otto_pqw_emit']['GBps_read_plus_written'] = (read_emit + written) / np.median(emit_ms) / 1e6
    return res


def child(mode, aids, dev):
    import torch
    from otto_amd.covisitation import builder, engine
    y, w, n = dense_topk(aids, dev)
    torch.cuda.synchronize(dev)
    d = pathlib.Path(tempfile.mkdtemp(prefix='perf_pqwrite_'))
    try:
        t0 = time.perf_counter()
        if mode == 'device':
            rows = engine.topk_to_device_rows(y, w, n)
            t1 = time.perf_counter()
            builder.write_device_parts(d, 'top', 'clicks', rows, PARTS, N_AIDS)
        else:
            rows = engine.topk_to_rows(y, w, n)
            t1 = time.perf_counter()
            builder.write_jobs(builder.part_jobs(d, 'top', 'clicks', rows, PARTS, N_AIDS))
        t2 = time.perf_counter()
        size = sum(os.path.getsize(d / f) for f in os.listdir(d))
        return {'mode': mode, 'rows': int(len(rows[0])), 'rows_s': t1 - t0, 'write_s': t2 - t1, 'wall_s': t2 - t0, 'file_bytes': size,
                'file_bytes_per_row': size / len(rows[0]), 'files': len(os.listdir(d))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--aids', type=int, default=(1 << 25) // K)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pqwrite', 'perf_pqwrite.json'))
    ap.add_argument('--child', choices=('device', 'host'))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    dev = torch.device('cuda:0')
    if args.child:
        from otto_amd import _lib
        _lib.lib()
        print(json.dumps(child(args.child, args.aids, dev)))
        return
    g.build()
    res = {'device': torch.cuda.get_device_name(0), 'kernels': kernels(args.aids, dev), 'end_to_end': []}
    for rep in range(3):
        for mode in ('host', 'device'):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--aids', str(args.aids)], stdout=subprocess.PIPE,
                               text=True, check=True, timeout=300)
            res['end_to_end'].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(res['end_to_end'][-1], flush=True)
    for mode in ('host', 'device'):
        walls = [r['wall_s'] for r in res['end_to_end'] if r['mode'] == mode]
        res[f'{mode}_wall_s'] = {'median': float(np.median(walls)), 'min': min(walls), 'max': max(walls)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
