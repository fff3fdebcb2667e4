"""Rates of the device-side Parquet decode (include/otto_parquet.h) -> profiles/parquet/perf_parquet.json.

Input: ``synth.generate_sessions`` sessions (default 2,000,000, the generator of the other perf tools) as the split files
are written: ``DataFrame.to_parquet`` with default settings, train and val halves. With device events, 1 warm-up and 5
repeats, median (min - max): the Snappy phase alone, the runs + decode phase alone (``otto_parquet_decode`` with one
phase each, over the batch ``read_columns`` itself built), and the host-to-device copy of the same compressed bytes from
pinned memory (the floor of any end-to-end figure). With a host clock ending in a synchronise, the files in the page
cache: ``parquet.read_columns``, ``events.parquet_to_events_device``, and the path they replace on the same host in the
same job: ``pyarrow.parquet.read_table`` alone and with ``events.frame_to_events_device`` behind it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from otto_amd import events, parquet
from otto_amd.synth import generate_sessions

HBM_PEAK = 8.0e12            # bytes/s, MI355X
COLUMNS = ['session', 'aid', 'ts', 'type']

ap = argparse.ArgumentParser()
ap.add_argument('--sessions', type=int, default=2_000_000)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--out', default=os.path.join('profiles', 'parquet', 'perf_parquet.json'))
ap.add_argument('--tmp', default=None, help='directory of the files')
a = ap.parse_args()


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


def wall(fn, repeats):
    """seconds of fn() on the host clock, ending in a synchronise, 1 warm-up"""
    out = []
    for r in range(repeats + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        keep = fn()
        torch.cuda.synchronize(dev)
        if r:
            out.append(time.perf_counter() - t0)
        del keep
    return out


dev = torch.device('cuda:0')
t0 = time.time()
fr = generate_sessions(a.sessions).to_frame()
print(f'{a.sessions} sessions, {len(fr)} events, frame dtypes {dict(fr.dtypes.astype(str))}, generated in {time.time() - t0:.1f} s; '
      f'os.cpu_count() = {os.cpu_count()}', flush=True)
with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
    cut = int(np.searchsorted(fr['session'].to_numpy(), fr['session'].iloc[len(fr) * 4 // 5]))
    paths = [os.path.join(tmp, 'train.parquet'), os.path.join(tmp, 'val.parquet')]
    fr.iloc[:cut].to_parquet(paths[0])
    fr.iloc[cut:].to_parquet(paths[1])
    E = len(fr)
    del fr
    file_bytes = sum(os.path.getsize(p) for p in paths)

    # the batch read_columns builds, kept for the phase timings
    kept = []
    inner = parquet._decode

    def keep_batch(dev_, d_bytes, n, table, cols, infos, **kw):
        kept.append((d_bytes, n, table, cols, infos))
        return inner(dev_, d_bytes, n, table, cols, infos, **kw)
    parquet._decode = keep_batch
    out = parquet.read_columns(paths, COLUMNS, dev, batch_bytes=1 << 40)
    parquet._decode = inner
    assert len(kept) == 1, 'one batch expected'
    d_bytes, n, table, cols, infos = kept[0]
    table = np.asarray(table, dtype=np.int64)
    comp = int(table[:, parquet.F['comp_size']].sum())
    decoded = sum(int(t.numel() * t.element_size()) for t in out)
    bodies = int(table[table[:, parquet.F['is_compressed']] != 0, parquet.F['uncomp_size']].sum())
    res = dict(sessions=a.sessions, events=E, file_bytes=file_bytes, compressed_page_bytes=comp, decompressed_body_bytes=bodies,
               decoded_bytes=decoded, pages=len(table), tiles=int(sum((int(v) + parquet.TILE - 1) // parquet.TILE
                                                                     for v, t in zip(table[:, parquet.F['num_values']], table[:, parquet.F['page_type']]) if t != 2)),
               largest_page_bytes=int(table[:, parquet.F['uncomp_size']].max()), cpu_count=os.cpu_count(), timing_repeats=a.repeats)
    work = inner(dev, d_bytes, n, table, cols, infos)
    snappy_ms = timed(lambda: inner(dev, d_bytes, n, table, cols, infos, phases=1, work=work), a.repeats)
    decode_ms = timed(lambda: inner(dev, d_bytes, n, table, cols, infos, phases=2, work=work), a.repeats)
    both_ms = timed(lambda: inner(dev, d_bytes, n, table, cols, infos, phases=3, work=work), a.repeats)
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    copy_ms = timed(lambda: d_bytes[:n].copy_(host, non_blocking=True), a.repeats)
    res['snappy_ms'], res['runs_decode_ms'], res['decode_call_ms'], res['h2d_pinned_ms'] = map(spread, (snappy_ms, decode_ms, both_ms, copy_ms))
    res['gb_per_s'] = dict(snappy_in=comp / statistics.median(snappy_ms) / 1e6, snappy_out=bodies / statistics.median(snappy_ms) / 1e6,
                           decode_out=decoded / statistics.median(decode_ms) / 1e6,
                           call_compressed_in=comp / statistics.median(both_ms) / 1e6, call_decoded_out=decoded / statistics.median(both_ms) / 1e6)
    # algorithmic bytes of the whole call: the compressed bytes read, the bodies written and read, the columns written
    res['share_of_hbm_peak'] = (comp + 2 * bodies + decoded) / (statistics.median(both_ms) * 1e-3) / HBM_PEAK
    print(json.dumps({k: res[k] for k in ('snappy_ms', 'runs_decode_ms', 'decode_call_ms', 'h2d_pinned_ms', 'gb_per_s')}), flush=True)
    del out, kept, work, host, d_bytes

    import pyarrow.parquet as pq
    res['read_columns_s'] = spread(wall(lambda: parquet.read_columns(paths, COLUMNS, dev), a.repeats))
    res['parquet_to_events_device_s'] = spread(wall(lambda: events.parquet_to_events_device(paths, dev), a.repeats))
    res['pyarrow_read_table_s'] = spread(wall(lambda: [pq.read_table(p, columns=COLUMNS) for p in paths], a.repeats))
    res['pyarrow_frame_to_events_device_s'] = spread(wall(
        lambda: events.frame_to_events_device([pq.read_table(p, columns=COLUMNS) for p in paths], dev), a.repeats))
os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
