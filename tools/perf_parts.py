"""Part files back to resident top-k arrays (DESIGN.md sections 2e and 2g): the delta decode and `otto_rows_topk` alone, and
`parts.load_matrix` end to end against the host path, on the row set of `tools/perf_pqwrite.py` -- 2^25 rows, aid_x runs of 20
over sorted distinct aids, aid_y uniform below 1,855,603, 16.16 fixed-point weights -- device-written as the 6 parts of a
`top_<kind>` set (aid_x and aid_y DELTA_BINARY_PACKED, wgt PLAIN).

    python tools/perf_parts.py [--aids 1677722] [--out profiles/parts/perf_parts.json]
    python tools/perf_parts.py --loop DIR        the decode and the regrouping three times, nothing timed (for a kernel trace)

Kernels: hipEvents around `otto_parquet_decode` over the six file images resident on the device (all of its kernels: the
delta walk, block sums, scan and store for aid_x and aid_y, the PLAIN copy for wgt) and around `otto_rows_topk`, 1 warm-up +
5 repeats, median (min - max). End to end: `parts.load_matrix` from files in the page cache against `pd.read_parquet` of the
parts + upload + the same `rows_to_topk`, alternating, three fresh processes each (`--child device|host`), wall time from the
paths to the synchronised arrays. The library must be built before (`__graft_entry__.build()`).
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
N_AIDS, K, PARTS = 1855603, 20, 6
COLUMNS = ['aid_x', 'aid_y', 'wgt']


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def write_parts(directory, aids, dev):
    from perf_pqwrite import dense_topk
    from otto_amd.covisitation import builder, engine
    rows = engine.topk_to_device_rows(*dense_topk(aids, dev))
    builder.write_device_parts(pathlib.Path(directory), 'top', 'clicks', rows, PARTS, N_AIDS)
    return int(rows[0].numel())


def paths_of(directory):
    from otto_amd.covisitation import parts
    return [str(p) for p in parts.part_paths(directory, 'top', 'clicks', PARTS)]


def resident_jobs(directory, dev):
    """per file: (device image, page table, column records, infos) for one otto_parquet_decode call, and the output columns"""
    import torch
    from otto_amd import parquet
    jobs, total = [], 0
    metas = [parquet.page_table(p, COLUMNS, floats=True) for p in paths_of(directory)]
    n_rows = sum(m.num_rows for m, _ in metas)
    outs = [torch.empty(n_rows, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32)]
    cols = [(o.data_ptr(), 4, n_rows, 4, 0) for o in outs]
    for (meta, pages) in metas:
        image = torch.from_numpy(np.fromfile(meta.path, dtype=np.uint8)).to(dev)
        table, infos, row = [], [], total
        for g, rg in enumerate(meta.row_groups):
            for j, c in enumerate(COLUMNS):
                r = row
                for k, p in enumerate(pages[g, c]):
                    table.append((rg.chunks[c].start + p.src_off, p.comp_size, p.uncomp_size, p.page_type, p.encoding, p.def_len, p.rep_len,
                                  p.num_values, p.is_compressed, r, j, -1))
                    infos.append((f'{meta.path}: column {c!r}, row group {g}', k))
                    r += p.num_values
            row += rg.num_rows
        total = row
        jobs.append((image, table, infos))
    return jobs, cols, outs, n_rows


def decode_all(jobs, cols, dev, works):
    from otto_amd import parquet
    for (image, table, infos), work in zip(jobs, works):
        parquet._decode(dev, image, int(image.numel()), table, cols, infos, work=work)


def kernels(directory, dev):
    import ctypes as C
    import torch
    from otto_amd import _lib
    from otto_amd.covisitation import parts
    jobs, cols, outs, n_rows = resident_jobs(directory, dev)
    works = []
    for image, table, _ in jobs:
        t = np.ascontiguousarray(table, dtype=np.int64)
        works.append(_lib.workspace(int(_lib.lib().otto_parquet_workspace(t.ctypes.data_as(C.c_void_p), len(t))), dev))

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize(dev)
        return got, e0.elapsed_time(e1)
    dec, top = [], []
    for rep in range(6):                                      # 1 warm-up + 5
        dec.append(timed(lambda: decode_all(jobs, cols, dev, works))[1])
    work = torch.empty(4096, dtype=torch.uint8, device=dev)
    for rep in range(6):
        top.append(timed(lambda: parts.rows_to_topk(*outs, N_AIDS, K, work=work))[1])
    file_bytes = sum(int(j[0].numel()) for j in jobs)
    res = {'rows': n_rows, 'file_bytes': file_bytes, 'file_bytes_per_row': file_bytes / n_rows, 'pages': sum(len(j[1]) for j in jobs),
           'otto_parquet_decode_6_files': summary(dec[1:]), 'otto_rows_topk': summary(top[1:])}
    res['otto_parquet_decode_6_files']['Mrows_per_s'] = n_rows / np.median(dec[1:]) / 1e3
    res['otto_rows_topk']['GBps_read_plus_written'] = (12 * n_rows + 8 * n_rows + (8 * K + 4) * N_AIDS) / np.median(top[1:]) / 1e6
    return res


def child(mode, directory, dev):
    import torch
    from otto_amd.covisitation import parts
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if mode == 'device':
        y, w, n = parts.load_matrix(directory, 'top', 'clicks', PARTS, N_AIDS, K, dev)
    else:
        import pandas as pd
        df = pd.concat([pd.read_parquet(p) for p in paths_of(directory)], ignore_index=True)
        cols = [torch.from_numpy(df[c].to_numpy()).to(dev) for c in COLUMNS]
        y, w, n = parts.rows_to_topk(*cols, N_AIDS, K)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    return {'mode': mode, 'wall_s': t1 - t0, 'rows': int(n.sum()), 'checksum': int(y.long().sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--aids', type=int, default=(1 << 25) // K)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'parts', 'perf_parts.json'))
    ap.add_argument('--child', choices=('device', 'host'))
    ap.add_argument('--dir')
    ap.add_argument('--loop')
    args = ap.parse_args()
    import torch
    from otto_amd import _lib
    _lib.lib()
    dev = torch.device('cuda:0')
    if args.child:
        print(json.dumps(child(args.child, args.dir, dev)))
        return
    if args.loop:
        from otto_amd.covisitation import parts
        os.makedirs(args.loop, exist_ok=True)
        write_parts(args.loop, args.aids, dev)
        for rep in range(3):
            parts.load_matrix(args.loop, 'top', 'clicks', PARTS, N_AIDS, K, dev)
        torch.cuda.synchronize(dev)
        shutil.rmtree(args.loop, ignore_errors=True)
        return
    d = tempfile.mkdtemp(prefix='perf_parts_')
    try:
        rows = write_parts(d, args.aids, dev)
        res = {'device': torch.cuda.get_device_name(0), 'rows_written': rows, 'kernels': kernels(d, dev), 'end_to_end': []}
        torch.cuda.empty_cache()
        for rep in range(3):
            for mode in ('host', 'device'):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--dir', d], stdout=subprocess.PIPE, text=True,
                                   check=True, timeout=300)
                res['end_to_end'].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(res['end_to_end'][-1], flush=True)
        assert len({(r['rows'], r['checksum']) for r in res['end_to_end']}) == 1, 'the two paths disagree'
        for mode in ('host', 'device'):
            walls = [r['wall_s'] for r in res['end_to_end'] if r['mode'] == mode]
            res[f'{mode}_wall_s'] = {'median': float(np.median(walls)), 'min': min(walls), 'max': max(walls)}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
