"""val_labels.parquet to three resident label lists: the phases of `evaluate.read_labels` and the whole
of it against the host path, on a synthetic file at the size of the real one -- 1.8 M sessions, each with a clicks row (95 %),
a carts row (17 %) and an orders row (8 %), one click label, 1 + geometric(0.45) cart / order labels below 1,855,603 --
written by pyarrow with the settings of `DataFrame.to_parquet` (Snappy, V1 pages of 1 MiB, dictionary where it pays).

    python tools/perf_labels.py [--sessions 1800000] [--out profiles/labels/perf_labels.json]
    python tools/perf_labels.py --loop FILE      write FILE and run read_labels three times, nothing timed (for a kernel trace)

Phases: `read_labels` in one process, 1 warm-up + 5 repeats, with hipEvents around every `otto_parquet_snappy` (the V1 bodies
of the list column), `otto_pqlist_levels` (the level kernels), `otto_parquet_decode` (the values of the list column, and
apart from them the session and type columns) and `otto_labels_count` + `otto_labels_fill`; median (min - max) of the
per-repeat sums. End to end: `read_labels` from a file in the page cache against `pd.read_parquet` + the reference's `map`,
three `merge(how='left')` and `fillna` + `np.cumsum` + upload, alternating, three fresh processes each (`--child device|host`),
wall time from the path to the synchronised lists. The library must be built before (`__graft_entry__.build()`).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_AIDS = 1855603
TYPES = ('clicks', 'carts', 'orders')


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def write_file(path, n_sessions, seed=0):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(11098528, 11098528 + 2 * n_sessions), size=n_sessions, replace=False)).astype(np.int64)
    sess, typ, lens = [], [], []
    for t, share in enumerate((0.95, 0.17, 0.08)):
        has = rng.random(n_sessions) < share
        sess.append(ids[has])
        typ.append(np.full(int(has.sum()), t, dtype=np.int8))
        lens.append(np.ones(int(has.sum()), dtype=np.int64) if t == 0 else rng.geometric(0.45, size=int(has.sum())).astype(np.int64))
    sess, typ, lens = np.concatenate(sess), np.concatenate(typ), np.concatenate(lens)
    order = np.lexsort((typ, sess))                            # session-major, as validation.py writes the labels
    sess, typ, lens = sess[order], typ[order], lens[order]
    off = np.r_[0, np.cumsum(lens)].astype(np.int32)
    values = rng.integers(0, N_AIDS, size=int(off[-1])).astype(np.int64)
    tab = pa.table({'session': pa.array(sess), 'type': pa.array(np.array(TYPES)[typ]),
                    'ground_truth': pa.ListArray.from_arrays(pa.array(off), pa.array(values))})
    pq.write_table(tab, path)
    return {'sessions': int(n_sessions), 'rows': int(len(sess)), 'values': int(len(values)), 'file_bytes': os.path.getsize(path),
            'rows_per_type': [int((typ == t).sum()) for t in range(3)]}


def phases(path, dev):
    """per-repeat sums of the event times around the entry points read_labels goes through"""
    import torch
    from otto_amd import _lib, parquet
    from otto_amd.ranker import evaluate
    acc, state = {}, {'list': False}
    real_call, real_lists = _lib.call, parquet.read_lists

    def call(name, d, *a, **kw):
        key = {'otto_parquet_snappy': 'list_snappy', 'otto_pqlist_levels': 'list_levels', 'otto_labels_count': 'labels', 'otto_labels_fill': 'labels',
               'otto_parquet_decode': 'list_values' if state['list'] else 'flat_columns'}.get(name)
        if key is None:
            return real_call(name, d, *a, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            return real_call(name, d, *a, **kw)
        finally:
            e1.record()
            acc.setdefault(key, []).append((e0, e1))

    def read_lists(*a, **kw):
        state['list'] = True
        try:
            return real_lists(*a, **kw)
        finally:
            state['list'] = False
    _lib.call, parquet.read_lists = call, read_lists
    out = {}
    try:
        for rep in range(6):                                    # 1 warm-up + 5
            acc.clear()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            session, labels, dropped = evaluate.read_labels(path, dev, n_aids=N_AIDS)
            torch.cuda.synchronize(dev)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                for k, evs in acc.items():
                    out.setdefault(k, []).append(sum(a.elapsed_time(b) for a, b in evs))
                out.setdefault('read_labels_wall', []).append(wall)
    finally:
        _lib.call, parquet.read_lists = real_call, real_lists
    res = {k: summary(v) for k, v in out.items()}
    res['sessions'] = int(session.numel())
    res['label_counts'] = [int(labels[t][1].numel()) for t in TYPES]
    return res


def host_labels(path, dev):
    """the reference's chain, then CSR through np.cumsum and the upload (INTEGRATION.md section 2h before this path existed)"""
    import pandas as pd
    import torch
    df = pd.read_parquet(path)
    base = pd.DataFrame({'session': np.sort(df['session'].unique())})
    out = {}
    for name in TYPES:
        sub = df.loc[df['type'] == name, ['session', 'ground_truth']]
        m = base.merge(sub, on='session', how='left')
        col = m['ground_truth']
        lists = [v if isinstance(v, np.ndarray) else () for v in col]           # fillna([]) on a column of arrays
        lens = np.fromiter((len(v) for v in lists), dtype=np.int64, count=len(lists))
        aid = np.concatenate([v for v in lists if len(v)]).astype(np.int32) if lens.sum() else np.zeros(0, dtype=np.int32)
        out[name] = (torch.from_numpy(np.r_[0, np.cumsum(lens)].astype(np.int64)).to(dev), torch.from_numpy(aid).to(dev))
    return torch.from_numpy(base['session'].to_numpy().astype(np.int32)).to(dev), out


def child(mode, path, dev):
    import torch
    from otto_amd.ranker import evaluate
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if mode == 'device':
        session, labels, _ = evaluate.read_labels(path, dev, n_aids=N_AIDS)
    else:
        session, labels = host_labels(path, dev)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    return {'mode': mode, 'wall_s': t1 - t0, 'sessions': int(session.numel()),
            'checksum': [int(labels[t][1].long().sum()) + int(labels[t][0].sum()) for t in TYPES]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=1800000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'labels', 'perf_labels.json'))
    ap.add_argument('--child', choices=('device', 'host'))
    ap.add_argument('--file')
    ap.add_argument('--loop')
    args = ap.parse_args()
    import torch
    from otto_amd import _lib
    _lib.lib()
    dev = torch.device('cuda:0')
    if args.child:
        print(json.dumps(child(args.child, args.file, dev)))
        return
    if args.loop:
        from otto_amd.ranker import evaluate
        write_file(args.loop, args.sessions)
        for rep in range(3):
            evaluate.read_labels(args.loop, dev, n_aids=N_AIDS)
        torch.cuda.synchronize(dev)
        os.remove(args.loop)
        return
    d = tempfile.mkdtemp(prefix='perf_labels_')
    path = os.path.join(d, 'val_labels.parquet')
    try:
        res = {'device': torch.cuda.get_device_name(0), 'file': write_file(path, args.sessions)}
        print(json.dumps(res['file']), flush=True)
        res['phases'] = phases(path, dev)
        print(json.dumps(res['phases']), flush=True)
        torch.cuda.empty_cache()
        res['end_to_end'] = []
        for rep in range(3):
            for mode in ('host', 'device'):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--file', path], stdout=subprocess.PIPE, text=True,
                                   check=True, timeout=240)
                res['end_to_end'].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(res['end_to_end'][-1], flush=True)
        assert len({(r['sessions'], tuple(r['checksum'])) for r in res['end_to_end']}) == 1, 'the two paths disagree'
        for mode in ('host', 'device'):
            walls = [r['wall_s'] for r in res['end_to_end'] if r['mode'] == mode]
            res[f'{mode}_wall_s'] = {'median': float(np.median(walls)), 'min': min(walls), 'max': max(walls)}
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
