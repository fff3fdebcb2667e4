"""Device-side Snappy (include/otto_snappy.h): `otto_snappy_plan` / `otto_snappy_emit` alone, and
`parquet_write.write_tables` with and without the codec against `DataFrame.to_parquet`, on one shape: the four chunk-writer
columns (session int32, aid int32, ts int64, type stored as int32) and a covisitation weight column (float32) of a synthetic
split of 2 M sessions, as the bytes of their PLAIN pages of 2^16 values -- one stream per page, all columns in one job.

    python tools/perf_snappy.py [--sessions 2000000] [--out profiles/snappy/perf_snappy.json]

Kernels: hipEvents around each call, 1 warm-up + 5 repeats, median (min - max); GB/s of input; the share of the 8 TB/s HBM peak
from the bytes each call must move (plan: the input once; emit: the literal bytes in, the streams out). Sizes: the compressed
fraction per column beside pyarrow's `Codec('snappy')` over the same bytes. End to end: `write_tables` of the five columns
in chunks of 100,000 sessions, `compression=None`, `'snappy'`, and pandas `to_parquet` with its defaults on the same chunks,
alternating, three fresh processes each (`--child none|snappy|pandas`), wall time from the resident columns to the closed files.
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
PAGE_VALUES, CHUNK_SESSIONS, HBM_PEAK = 1 << 16, 100_000, 8.0e12


def columns(sessions, dev):
    """{name: device tensor} of the shape, and the session offsets."""
    import torch
    from otto_amd.synth import generate_sessions_torch
    ev = generate_sessions_torch(sessions, device=dev)
    off = ev['sess_off']
    n = int(ev['aid'].numel())
    g = torch.Generator(device=dev).manual_seed(5)
    session = torch.repeat_interleave(torch.arange(sessions, device=dev, dtype=torch.int32), off[1:] - off[:-1], output_size=n)
    wgt = torch.empty(n, device=dev).geometric_(0.35, generator=g) + 0.5 * (torch.rand(n, device=dev, generator=g) < 0.3)
    return {'session': session, 'aid': ev['aid'].contiguous(), 'ts': ev['ts'].to(torch.int64) * 1000, 'type': ev['type'].contiguous(),
            'wgt': wgt.to(torch.float32)}, off


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def kernels(sessions, dev):
    import pyarrow as pa
    import torch
    from otto_amd import snappy
    cols, _ = columns(sessions, dev)
    stored = {k: (v.to(torch.int32) if v.dtype == torch.uint8 else v) for k, v in cols.items()}     # a PLAIN page stores type as INT32
    raw = torch.cat([v.view(torch.uint8) for v in stored.values()])
    src_off, src_len, owner, at = [], [], [], 0
    for name, v in stored.items():
        step, nbytes = PAGE_VALUES * v.element_size(), v.numel() * v.element_size()
        for lo in range(0, nbytes, step):
            src_off.append(at + lo), src_len.append(min(step, nbytes - lo)), owner.append(name)
        at += nbytes
    job = snappy.DeviceJob(raw, src_off, src_len)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize(dev)
        return got, e0.elapsed_time(e1)
    plan_ms, emit_ms = [], []
    for rep in range(6):                                      # 1 warm-up + 5
        sizes, ms = timed(job.plan)
        plan_ms.append(ms)
    sizes = sizes.copy()
    dst = np.r_[0, np.cumsum(sizes)[:-1]]
    out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=dev)
    for rep in range(6):
        emit_ms.append(timed(lambda: job.emit(dst, out))[1])
    plan_ms, emit_ms = plan_ms[1:], emit_ms[1:]
    n, z = int(raw.numel()), int(sizes.sum())
    host, codec, by_col, at = raw.cpu().numpy(), pa.Codec('snappy'), {}, 0
    owner = np.array(owner)
    for name, v in stored.items():
        nbytes = v.numel() * v.element_size()
        ours = int(sizes[owner == name].sum())
        theirs = len(codec.compress(host[at:at + nbytes].tobytes(), asbytes=True))
        by_col[name] = {'raw_bytes': nbytes, 'device_bytes': ours, 'device_fraction': ours / nbytes, 'pyarrow_bytes': theirs,
                        'pyarrow_fraction': theirs / nbytes}
        at += nbytes
    back = codec.decompress(out[int(dst[-1]):].cpu().numpy().tobytes(), decompressed_size=src_len[-1], asbytes=True)
    assert back == host[src_off[-1]:src_off[-1] + src_len[-1]].tobytes(), 'the last stream does not decompress to its page'
    res = {'rows': int(stored['aid'].numel()), 'input_bytes': n, 'streams': len(src_off), 'stream_bytes': z, 'fraction': z / n,
           'workspace_bytes': int(job.work.numel()), 'columns': by_col, 'otto_snappy_plan': summary(plan_ms), 'otto_snappy_emit': summary(emit_ms)}
    p, e = np.median(plan_ms) * 1e-3, np.median(emit_ms) * 1e-3
    res['otto_snappy_plan'].update(GBps_input=n / p / 1e9, hbm_share=n / HBM_PEAK / p)
    res['otto_snappy_emit'].update(GBps_input=n / e / 1e9, hbm_share=2 * z / HBM_PEAK / e)      # at most z literal bytes in, z bytes out
    res['both'] = {'median_ms': float((p + e) * 1e3), 'GBps_input': n / (p + e) / 1e9}
    return res


def child(mode, sessions, dev):
    import torch
    from otto_amd import parquet_write
    cols, off = columns(sessions, dev)
    cuts = off[torch.arange(0, sessions + CHUNK_SESSIONS, CHUNK_SESSIONS, device=dev).clamp_(max=sessions)].cpu().tolist()
    torch.cuda.synchronize(dev)
    d = pathlib.Path(tempfile.mkdtemp(prefix='perf_snappy_'))
    paths = [d / f'chunk_{i}.parquet' for i in range(len(cuts) - 1)]
    try:
        t0 = time.perf_counter()
        if mode == 'pandas':
            import pandas as pd
            frame = pd.DataFrame({k: v.cpu().numpy() for k, v in cols.items()})
            t1 = time.perf_counter()
            for p, lo, hi in zip(paths, cuts, cuts[1:]):
                frame.iloc[lo:hi].to_parquet(p)
        else:
            t1 = t0
            parquet_write.write_tables(paths, cols, cuts, compression=None if mode == 'none' else 'snappy')
        t2 = time.perf_counter()
        size = sum(os.path.getsize(p) for p in paths)
        return {'mode': mode, 'rows': int(cols['aid'].numel()), 'files': len(paths), 'to_host_s': t1 - t0, 'wall_s': t2 - t0, 'file_bytes': size}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=2_000_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'snappy', 'perf_snappy.json'))
    ap.add_argument('--child', choices=('none', 'snappy', 'pandas'))
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    if not torch.cuda.is_available():
        raise SystemExit('perf_snappy needs a ROCm device: nothing is measured without one')
    dev = torch.device('cuda:0')
    if args.child:
        from otto_amd import _lib
        _lib.lib()
        print(json.dumps(child(args.child, args.sessions, dev)))
        return
    g.build()
    res = {'device': torch.cuda.get_device_name(0), 'sessions': args.sessions, 'kernels': kernels(args.sessions, dev), 'end_to_end': []}
    print(json.dumps(res['kernels']), flush=True)
    modes = () if args.kernels_only else ('none', 'snappy', 'pandas')
    for rep in range(3):
        for mode in modes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--sessions', str(args.sessions)], stdout=subprocess.PIPE,
                               text=True, check=True, timeout=300)
            res['end_to_end'].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(res['end_to_end'][-1], flush=True)
    for mode in modes:
        runs = [r for r in res['end_to_end'] if r['mode'] == mode]
        walls = [r['wall_s'] for r in runs]
        res[f'{mode}_wall_s'] = {'median': float(np.median(walls)), 'min': min(walls), 'max': max(walls), 'file_bytes': runs[0]['file_bytes']}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
