"""Rates of the device-side JSONL ingest (include/otto_jsonl.h) -> profiles/jsonl/perf_jsonl.json.

Input: 100,000 ``synth.generate_sessions`` sessions serialised once in the dataset's form, repeated to at least 1 GiB (the
parser does not mind repeated session ids). With device events, 1 warm-up and 5 repeats, median (min - max): otto_jsonl_count
and otto_jsonl_parse per GiB, and the host-to-device copy of the same bytes from pinned memory (the floor of any end-to-end
figure). With a host clock ending in a synchronise: events.jsonl_to_events_device from a file on disk. The CPU figure is
the reference's create_dataframe restated (pd.read_json(lines=True, chunksize=100000) and its loop) on the 100,000-session
block, on this host."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from otto_amd import _lib, events
from otto_amd.synth import generate_sessions

HBM_PEAK = 8.0e12            # bytes/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument('--sessions', type=int, default=100_000)
ap.add_argument('--gib', type=float, default=1.0)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=os.path.join('profiles', 'jsonl', 'perf_jsonl.json'))
ap.add_argument('--tmp', default=None, help='directory of the file the end-to-end call reads')
a = ap.parse_args()


def serialise(ev):
    names = ('clicks', 'carts', 'orders')
    off, aid, ts, typ = ev.sess_off.tolist(), ev.aid.tolist(), (ev.ts.astype(np.int64) * 1000 + 25).tolist(), ev.type.tolist()
    lines = []
    for s in range(len(off) - 1):
        body = ','.join(f'{{"aid":{aid[i]},"ts":{ts[i]},"type":"{names[typ[i]]}"}}' for i in range(off[s], off[s + 1]))
        lines.append(f'{{"session":{s},"events":[{body}]}}\n')
    return ''.join(lines).encode()


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
ev = generate_sessions(a.sessions)
t0 = time.time()
block = serialise(ev)
print(f'{a.sessions} sessions, {ev.n_events} events -> {len(block)} bytes ({len(block) / a.sessions:.0f} B/line, '
      f'{len(block) / ev.n_events:.1f} B/event), serialised in {time.time() - t0:.1f} s; os.cpu_count() = {os.cpu_count()}', flush=True)
reps = max(1, -(-int(a.gib * (1 << 30)) // len(block)))
n = reps * len(block)
assert n < 1 << 31, 'one call takes less than 2 GiB'
host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
hv = host.numpy()
for r in range(reps):
    hv[r * len(block):(r + 1) * len(block)] = np.frombuffer(block, dtype=np.uint8)
d_bytes = torch.empty(n, dtype=torch.uint8, device=dev)
gib = n / (1 << 30)
res = dict(sessions_block=a.sessions, events_block=int(ev.n_events), bytes_block=len(block), repeats_of_block=reps, n_bytes=n,
           cpu_count=os.cpu_count(), timing_repeats=a.repeats)

copy_ms = timed(lambda: d_bytes.copy_(host, non_blocking=True), a.repeats)
res['h2d_pinned_ms_per_gib'] = spread([m / gib for m in copy_ms])

lib = _lib.lib()
wb = int(lib.otto_jsonl_workspace(n))
work = _lib.workspace(wb, dev)
counts = (C.c_int64 * 2)()
count_ms = timed(lambda: _lib.call('otto_jsonl_count', dev, d_bytes, n, counts, work, wb), a.repeats)
S, E = int(counts[0]), int(counts[1])
assert (S, E) == (reps * a.sessions, reps * ev.n_events), (S, E)
cols = [torch.empty(E, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]
off, sid = torch.empty(S + 1, dtype=torch.int64, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
parse_ms = timed(lambda: _lib.call('otto_jsonl_parse', dev, d_bytes, n, 0, S, E, *cols, off, sid, counts, work, wb), a.repeats)
assert np.array_equal(cols[1][:ev.n_events].cpu().numpy().view(np.uint32), ev.aid.astype(np.uint32))
res['count_ms_per_gib'] = spread([m / gib for m in count_ms])
res['parse_ms_per_gib'] = spread([m / gib for m in parse_ms])
res['S'], res['E'] = S, E
# algorithmic bytes: count reads the text once; parse reads it twice and writes 17 B per event and 12 B per session
alg_count, alg_parse = n, 2 * n + 17 * E + 12 * S
res['algorithmic_bytes'] = dict(count=alg_count, parse=alg_parse)
res['share_of_hbm_peak'] = dict(count=alg_count / (statistics.median(count_ms) * 1e-3) / HBM_PEAK,
                                parse=alg_parse / (statistics.median(parse_ms) * 1e-3) / HBM_PEAK)
res['sessions_per_s_count_plus_parse'] = S / ((statistics.median(count_ms) + statistics.median(parse_ms)) * 1e-3)
print(json.dumps({k: res[k] for k in ('h2d_pinned_ms_per_gib', 'count_ms_per_gib', 'parse_ms_per_gib', 'share_of_hbm_peak')}), flush=True)
del cols, off, sid, work, d_bytes

# end to end from a file (the page cache holds it after the first read: "disk" here is a memory copy)
with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
    path = os.path.join(tmp, 'perf.jsonl')
    with open(path, 'wb') as f:
        f.write(memoryview(hv))
    del host, hv
    wall = []
    for r in range(a.repeats + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        de = events.jsonl_to_events_device(path, dev)
        torch.cuda.synchronize(dev)
        if r:
            wall.append(time.perf_counter() - t0)
        assert de.n_events == E
        del de
    read = []
    buf = bytearray(64 << 20)
    for r in range(3):
        t0 = time.perf_counter()
        with open(path, 'rb', buffering=0) as f:
            while f.readinto(buf):
                pass
        read.append(time.perf_counter() - t0)
res['end_to_end_s_per_gib'] = spread([w / gib for w in wall])
res['file_read_s_per_gib'] = spread([w / gib for w in read])
res['end_to_end_sessions_per_s'] = S / statistics.median(wall)

# the reference's create_dataframe, restated, on the block
import pandas as pd
with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
    path = os.path.join(tmp, 'block.jsonl')
    with open(path, 'wb') as f:
        f.write(block)
    t0 = time.perf_counter()
    type_dict = {'clicks': 0, 'carts': 1, 'orders': 2}
    frames = []
    for chunk in pd.read_json(path, lines=True, chunksize=100000):
        cols = {'session': [], 'aid': [], 'ts': [], 'type': []}
        for session, evs in zip(chunk['session'].tolist(), chunk['events'].tolist()):
            for e in evs:
                cols['session'].append(session)
                cols['aid'].append(e['aid'])
                cols['ts'].append(e['ts'])
                cols['type'].append(type_dict[e['type']])
        frames.append(pd.DataFrame(cols).astype({'session': np.uint32, 'aid': np.uint32, 'ts': np.uint64, 'type': np.uint8}))
    df = pd.concat(frames).reset_index(drop=True)
    cpu_s = time.perf_counter() - t0
assert len(df) == ev.n_events
res['cpu_create_dataframe_s_block'] = cpu_s
res['cpu_sessions_per_s'] = a.sessions / cpu_s
os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
