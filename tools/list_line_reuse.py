"""CPU estimate of how the runs of the covisitation index use the 128-byte lines of the shared component lists (NumPy only,
synthetic sessions): lines per run, how often the partition pass fetches each list line that a partitioned aid touches, and
chunks per partitioned aid. The estimate behind the chunk order of the partition pass ("Round-6 measurements").

Model (csrc/otto_covis.hip, "component lists"): a window is the last 30 events of a session; its list region is n words at
ev_base[s] (dense, 4 bytes a word); every distinct aid of the window has one run that reads the window's list of d distinct
aids. Windows are taken as ONE component (99 % of the OTTO-shape windows consist of cliques only), private rows are
ignored. An aid's records and runs are scaled from the sample to full OTTO (14,571,582 sessions) before the partition rule
of the index (heavy_mode / l_log2r) is applied; the fetch counts themselves are those of the sample."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from otto_amd.synth import generate_sessions, OTTO_N_AIDS, OTTO_N_SESSIONS

WINDOW, LINE, M_CAP, L_CAP, PACKED_MAX_RUNS, PART_CHUNK_RUNS = 30, 128, 3072, 6144, 4096, 256

ap = argparse.ArgumentParser()
ap.add_argument('--sessions', type=int, default=1_000_000)
ap.add_argument('--seed', type=int, default=42)
a = ap.parse_args()

ev = generate_sessions(a.sessions, n_aids=OTTO_N_AIDS, seed=a.seed)
L = np.diff(ev.sess_off)
n_win = np.where(np.minimum(L, WINDOW) >= 2, np.minimum(L, WINDOW), 0)
sess = np.repeat(np.arange(len(L), dtype=np.int64), L)
pos = np.arange(len(sess), dtype=np.int64) - ev.sess_off[:-1][sess]
tail = pos >= (L - n_win)[sess]
# runs: the distinct (window, aid) pairs
key = np.unique((sess[tail] << 32) | ev.aid[tail].astype(np.int64))
rs, rx = key >> 32, key & 0xFFFFFFFF
d = np.bincount(rs, minlength=len(L))                          # distinct aids per window
keep = d[rs] >= 2                                              # a window of one aid has no pair
rs, rx = rs[keep], rx[keep]
start = np.r_[0, np.cumsum(n_win)][:-1]                        # first list word of a window
first = start * 4 // LINE
last = (start + np.maximum(d, 1) - 1) * 4 // LINE
nl = last - first + 1
lines_per_run = float(nl[rs].sum() / len(rs))
used = float(4 * d[rs].sum() / len(rs))

scale = OTTO_N_SESSIONS / a.sessions
runs = np.bincount(rx, minlength=OTTO_N_AIDS) * scale
recs = np.bincount(rx, weights=d[rs] - 1, minlength=OTTO_N_AIDS) * scale
part = (recs > M_CAP) & np.where(runs < PACKED_MAX_RUNS, recs > 2 * L_CAP, recs > L_CAP)
chunks = np.ceil(runs[part] / PART_CHUNK_RUNS)
mine = part[rx]
fetches = int(nl[rs[mine]].sum())
touched = np.unique(np.r_[first[rs[mine]], last[rs[mine]]])
print(json.dumps({
    'sessions': a.sessions, 'runs': int(len(rs)), 'lines_per_run': round(lines_per_run, 3),
    'bytes_fetched_per_run': round(lines_per_run * LINE, 1), 'bytes_used_per_run': round(used, 1),
    'partitioned_aids_at_full_scale': int(part.sum()), 'runs_of_partitioned_aids': int(mine.sum()),
    'line_fetches_by_partitioned_aids': fetches, 'unique_lines_touched': int(len(touched)),
    'fetches_per_unique_line': round(fetches / max(1, len(touched)), 2),
    'chunks_per_partitioned_aid': {'min': int(chunks.min()) if len(chunks) else 0, 'median': float(np.median(chunks)) if len(chunks) else 0,
                                   'total_at_full_scale': int(chunks.sum())},
    'list_region_bytes': int(n_win.sum() * 4), 'unique_line_bytes': int(len(touched) * LINE),
    'list_region_bytes_at_full_scale': int(n_win.sum() * 4 * scale),
}))
