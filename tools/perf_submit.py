"""Rates of the submission writer and the most-frequent-aid statistics (include/otto_submit.h) ->
profiles/submit/perf_submit.json.

Format: otto_submit_measure + otto_submit_format for 3 x 1,671,803 lines x 20 aids drawn from ``synth`` (about 0.9 GB of
text), device events, 1 warm-up and 5 repeats, median (min - max); GB/s of algorithmic bytes (text written + 4 k + 8 per
line read) and the share of the 8 TB/s peak. Host comparison in the same job: the reference's row expression
(``' '.join(str(aid) ...)`` per row + ``to_csv``) restated at 2^18 lines. End to end: ``write_csv`` to ``.csv`` and
``.csv.gz`` with copy, zlib and file time apart. Frequency: otto_freq_count over the synthetic events (about 33.4 M, 1,855,603
aids), then the top 20."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from otto_amd import _lib, submission
from otto_amd.synth import OTTO_N_AIDS, generate_sessions_torch

HBM_PEAK = 8.0e12            # bytes/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument('--sessions', type=int, default=1_671_803)
ap.add_argument('--k', type=int, default=20)
ap.add_argument('--event-sessions', type=int, default=2_000_000, help='synthetic sessions the events are drawn from')
ap.add_argument('--host-lines', type=int, default=1 << 18)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--threads', type=int, default=8)
ap.add_argument('--out', default=os.path.join('profiles', 'submit', 'perf_submit.json'))
ap.add_argument('--tmp', default=None, help='directory of the files write_csv writes')
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


dev = torch.device('cuda:0')
S, k, T = a.sessions, a.k, 3
ev = generate_sessions_torch(a.event_sessions, device=dev)
E = int(ev['aid'].numel())
res = dict(sessions=S, k=k, tables=T, events=E, n_aids=OTTO_N_AIDS, cpu_count=os.cpu_count(), timing_repeats=a.repeats)
print(f'{E} synthetic events; os.cpu_count() = {os.cpu_count()}', flush=True)

# ---- format ---------------------------------------------------------------------------------------------------------------
idx = torch.arange(S * k, device=dev)
tables = [(ev['aid'][(idx + t * 7_000_003) % E].view(S, k).contiguous(), torch.full((S,), k, dtype=torch.int32, device=dev))
          for t in range(T)]
del idx
session_id = (12_899_779 + torch.arange(S, device=dev)).to(torch.int32)
arr = lambda i: (C.c_void_p * T)(*[_lib.ptr(tb[i]) for tb in tables])
head = (T, arr(0), arr(1), (C.c_int32 * T)(0, 1, 2), session_id, S, k, k, 0)
wb = int(_lib.lib().otto_submit_workspace(S, T))
work = _lib.workspace(wb, dev)
total = C.c_int64(0)
measure_ms = timed(lambda: _lib.call('otto_submit_measure', dev, *head, C.byref(total), work, wb), a.repeats)
n_text = int(total.value)
out = torch.empty(n_text, dtype=torch.uint8, device=dev)
format_ms = timed(lambda: _lib.call('otto_submit_format', dev, *head, out, n_text, 0, work, wb), a.repeats)
lines = S * T
read_bytes = lines * (4 * k + 8)
both = [m + f for m, f in zip(measure_ms, format_ms)]
res.update(lines=lines, text_bytes=n_text, measure_ms=spread(measure_ms), format_ms=spread(format_ms), measure_plus_format_ms=spread(both),
           algorithmic_bytes=n_text + read_bytes)
res['format_gb_per_s'] = (n_text + read_bytes) / (statistics.median(format_ms) * 1e-3) / 1e9
res['measure_plus_format_gb_per_s'] = (n_text + read_bytes) / (statistics.median(both) * 1e-3) / 1e9
res['share_of_hbm_peak'] = dict(format=res['format_gb_per_s'] * 1e9 / HBM_PEAK, measure_plus_format=res['measure_plus_format_gb_per_s'] * 1e9 / HBM_PEAK)
res['device_lines_per_s'] = lines / (statistics.median(both) * 1e-3)
print(json.dumps({key: res[key] for key in ('text_bytes', 'measure_ms', 'format_ms', 'format_gb_per_s', 'share_of_hbm_peak')}), flush=True)

# ---- the reference's row expression, restated, on this host ------------------------------------------------------------
import pandas as pd
H = min(a.host_lines, S)
h_top, h_sid = tables[0][0][:H].cpu().numpy(), session_id[:H].cpu().numpy()
t0 = time.perf_counter()
rows = []
for s in range(H):
    rows.append({'session_type': f'{h_sid[s]}_clicks', 'labels': ' '.join([str(aid) for aid in h_top[s]])})
host_text = pd.DataFrame(rows).to_csv(index=False).encode()
host_s = time.perf_counter() - t0
first = submission.format_rows(session_id[:H].contiguous(), [(tables[0][0][:H], tables[0][1][:H].contiguous())], [0], header=True)
assert first.cpu().numpy().tobytes() == host_text, 'device text differs from the host expression'
res.update(host_lines=H, host_join_to_csv_s=host_s, host_lines_per_s=H / host_s)
del first, rows, host_text

# ---- end to end ----------------------------------------------------------------------------------------------------------
with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
    for suffix in ('.csv', '.csv.gz'):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        stats = submission.write_csv(os.path.join(tmp, 'perf' + suffix), [submission.HEADER, out], threads=a.threads)
        stats['wall_s'] = time.perf_counter() - t0
        stats['threads'] = min(a.threads, submission.MAX_WORKERS)
        res['write_csv' + suffix.replace('.', '_')] = stats
        print(suffix, json.dumps(stats), flush=True)
del out, tables, work

# ---- most frequent aids ----------------------------------------------------------------------------------------------------
counts = torch.zeros((3, OTTO_N_AIDS), dtype=torch.int32, device=dev)


def count():
    counts.zero_()
    _lib.call('otto_freq_count', dev, ev['aid'], ev['type'], E, OTTO_N_AIDS, counts)


count_ms = timed(count, a.repeats)
top = [torch.empty((4, 20), dtype=dt, device=dev) for dt in (torch.int32, torch.int64)] + [torch.empty(4, dtype=torch.int32, device=dev)]
topk_ms = timed(lambda: _lib.call('otto_freq_topk', dev, counts, OTTO_N_AIDS, 20, *top), a.repeats)
want = torch.bincount(ev['aid'].long(), minlength=OTTO_N_AIDS)
order = torch.argsort(-(want * (1 << 22)) + torch.arange(OTTO_N_AIDS, device=dev))[:20]       # count descending, aid ascending
assert torch.equal(top[0][0].long(), order), 'top 20 differs from a sort of the counts'
res.update(freq_count_ms=spread(count_ms), freq_topk_ms=spread(topk_ms), freq_events_per_s=E / (statistics.median(count_ms) * 1e-3))

os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
