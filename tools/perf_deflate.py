"""Rates of the device-side DEFLATE (include/otto_deflate.h) -> profiles/deflate/perf_deflate.json.

The text of tools/perf_submit.py: 3 x 1,671,803 lines x 20 aids drawn from ``synth`` (about 821 MB). Device events, 1 warm-up
and 5 repeats, median (min - max), for otto_deflate_plan (k_deflate_plan and the scan) and otto_deflate_emit (the clear and
k_deflate_emit) over the whole text in one call. End to end: ``write_csv`` to ``.csv.gz`` with ``compressor='device'`` and
with zlib at level 6 on 8 workers, alternately in the same job. File sizes beside zlib's levels 1 and 6 and Z_HUFFMAN_ONLY
over the same cut into 64 KiB members.

The time of each kernel on its own comes from a second run, ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
python tools/perf_deflate.py --kernels-only --out DIR/entry_points.json`` (profiles/deflate/kernel_stats.csv)."""
import argparse
import concurrent.futures
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from otto_amd import _lib, deflate, submission
from otto_amd.synth import generate_sessions_torch

ap = argparse.ArgumentParser()
ap.add_argument('--sessions', type=int, default=1_671_803)
ap.add_argument('--k', type=int, default=20)
ap.add_argument('--event-sessions', type=int, default=2_000_000, help='synthetic sessions the aids are drawn from')
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--rounds', type=int, default=2, help='write_csv runs per compressor, alternating')
ap.add_argument('--threads', type=int, default=8)
ap.add_argument('--host-threads', type=int, default=16, help='workers of the zlib size comparison')
ap.add_argument('--out', default=os.path.join('profiles', 'deflate', 'perf_deflate.json'))
ap.add_argument('--tmp', default=None, help='directory of the files write_csv writes')
ap.add_argument('--kernels-only', action='store_true',
                help='stop after the two entry points: the run to put under rocprofv3 --kernel-trace --stats for the time of each kernel')
a = ap.parse_args()
BLOCK = deflate.BLOCK_MAX


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def timed(fn, repeats):
    """milliseconds of fn() between two device events, 1 warm-up"""
    out = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r:
            out.append(e0.elapsed_time(e1))
    return out


dev = torch.device('cuda:0')
S, k, T = a.sessions, a.k, 3
ev = generate_sessions_torch(a.event_sessions, device=dev)
E = int(ev['aid'].numel())
idx = torch.arange(S * k, device=dev)
tables = [(ev['aid'][(idx + t * 7_000_003) % E].view(S, k).contiguous(), torch.full((S,), k, dtype=torch.int32, device=dev))
          for t in range(T)]
session_id = (12_899_779 + torch.arange(S, device=dev)).to(torch.int32)
text = submission.format_rows(session_id, tables, [0, 1, 2])
del idx, tables, ev
n = int(text.numel())
res = dict(lines=S * T, k=k, text_bytes=n, block_bytes=BLOCK, blocks=-(-n // BLOCK), cpu_count=os.cpu_count(), timing_repeats=a.repeats)
print(f'{n} bytes of text, {res["blocks"]} blocks', flush=True)

# ---- the two entry points over the whole text ---------------------------------------------------------------------------------
wb = int(_lib.lib().otto_deflate_workspace(n, BLOCK))
work = _lib.workspace(wb, dev)
total = C.c_int64(0)
plan_ms = timed(lambda: _lib.call('otto_deflate_plan', dev, text, n, BLOCK, C.byref(total), work, wb), a.repeats)
z = torch.empty(int(total.value), dtype=torch.uint8, device=dev)
emit_ms = timed(lambda: _lib.call('otto_deflate_emit', dev, text, n, BLOCK, z, int(z.numel()), work, wb), a.repeats)
both = [p + e for p, e in zip(plan_ms, emit_ms)]
res.update(workspace_bytes=wb, member_bytes=int(total.value), ratio=int(total.value) / n, plan_ms=spread(plan_ms), emit_ms=spread(emit_ms),
           plan_plus_emit_ms=spread(both), text_gb_per_s=n / (statistics.median(both) * 1e-3) / 1e9)
print(json.dumps({key: res[key] for key in ('member_bytes', 'ratio', 'plan_ms', 'emit_ms', 'text_gb_per_s')}), flush=True)
if a.kernels_only:
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    sys.exit(0)
host_text = text.cpu().numpy().tobytes()
assert gzip.decompress(z.cpu().numpy().tobytes()) == host_text, 'the members do not decompress to the text'
del z, work


# ---- zlib over the same cut -----------------------------------------------------------------------------------------------------
def zlib_bytes(args):
    lo, hi, level, strategy = args
    size = 0
    for b in range(lo, hi, BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
        size += len(c.compress(host_text[b:min(b + BLOCK, hi)]) + c.flush())
    return size


span = 256 * BLOCK
with concurrent.futures.ThreadPoolExecutor(max_workers=a.host_threads) as pool:
    for name, level, strategy in (('huffman_only', 6, zlib.Z_HUFFMAN_ONLY), ('level1', 1, 0), ('level6', 6, 0)):
        t0 = time.perf_counter()
        size = sum(pool.map(zlib_bytes, [(lo, min(lo + span, n), level, strategy) for lo in range(0, n, span)]))
        res['zlib_' + name] = dict(bytes=size, ratio=size / n, wall_s=time.perf_counter() - t0, threads=a.host_threads)
        print(name, json.dumps(res['zlib_' + name]), flush=True)

# ---- end to end, alternating ------------------------------------------------------------------------------------------------------
runs = dict(device=[], zlib=[])
with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
    for r in range(a.rounds):
        for compressor in ('device', 'zlib'):
            path = os.path.join(tmp, f'{compressor}.csv.gz')
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            stats = submission.write_csv(path, [submission.HEADER, text], level=6, threads=a.threads, compressor=compressor)
            stats['wall_s'] = time.perf_counter() - t0
            runs[compressor].append(stats)
            print(compressor, json.dumps(stats), flush=True)
    with open(os.path.join(tmp, 'device.csv.gz'), 'rb') as f:
        assert gzip.decompress(f.read()) == submission.HEADER + host_text, 'the device file does not decompress to the text'
res['write_csv'] = runs
res['write_csv_wall_s'] = {c: spread([s['wall_s'] for s in runs[c]]) for c in runs}
res['write_csv_speedup'] = res['write_csv_wall_s']['zlib']['median'] / res['write_csv_wall_s']['device']['median']

os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
