"""The TF-IDF similarity model on the synthetic validation-split shape the other perf tools use:
`fit_transform`, the two transposes + re-normalisation of the aid direction, and `similar_aids` for every distinct last aid at
k = 49; against scikit-learn's `TfidfVectorizer` + `cosine_similarity(X.T, dense_output=False)` + per-row top-49 on the same
host, at the largest session count whose aid x aid product that host can hold.

    python tools/perf_tfidf.py [--sessions 2000000] [--host-budget-gb 8] [--host-seconds 120] [--out profiles/tfidf/perf_tfidf.json]

Device: hipEvents, 1 warm-up + 5 repeats, median (min - max). Algorithmic bytes of the top-k: 12 bytes (index + value) per
posting walked, over the queries' candidate bounds: once for a query of the small tier, twice (accumulate, select) for one
of the large tier. Comparison: the session count is doubled from 1,250 while an upper estimate of the product's bytes (every
session adds at most len^2 stored entries of 12 bytes) stays inside the budget and the last host run stayed inside
`--host-seconds`; at that count the two sides alternate in one job, three fresh processes each (`--child device|host`),
wall time from the resident event arrays to the top-49 lists. If not even 1,250 sessions fit the budget the tool says so
and writes the device figures alone. The library must be built before (`__graft_entry__.build()`).
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
K = 49


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def sessions_on(dev, n):
    from otto_amd.synth import generate_sessions_torch
    ev = generate_sessions_torch(n, device=dev)
    return ev['aid'], ev['type'], ev['sess_off'], ev['n_aids']


def last_aids(aid, off):
    import torch
    return torch.unique(aid[off[1:] - 1]).to(torch.int32).contiguous()


def device_figures(dev, n_sessions):
    import torch
    from otto_amd.tfidf import similarity
    aid, _, off, n_aids = sessions_on(dev, n_sessions)
    queries = last_aids(aid, off)
    queries = queries[queries >= similarity.SKLEARN_MIN_AID].contiguous()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = call()
        e1.record()
        torch.cuda.synchronize(dev)
        return got, e0.elapsed_time(e1)
    fit, tr, top = [], [], []
    for rep in range(6):                                      # 1 warm-up + 5
        m, ms = timed(lambda: similarity.fit_transform(aid, off, n_aids))
        fit.append(ms)
        (a, at), ms = timed(lambda: similarity.aid_matrices(m))
        tr.append(ms)
        (ids, sim, n), ms = timed(lambda: similarity.cosine_topk(a, at, queries, K, True))
        top.append(ms)
    df = (at.row_off[1:] - at.row_off[:-1])                    # entries per session of AT's rows = the posting lists' lengths
    rows = a.row_off
    cum = torch.zeros(a.nnz + 1, dtype=torch.int64, device=dev)
    torch.cumsum(df[a.col.long()], 0, out=cum[1:])
    bound = cum[rows[1:]] - cum[rows[:-1]]                     # candidate bound of every aid
    qb = bound[queries.long()]
    res = {'sessions': n_sessions, 'tokens': int(aid.numel()), 'n_aids': n_aids, 'nnz': m.nnz, 'queries': int(queries.numel()), 'k': K,
           'fit_transform': summary(fit[1:]), 'aid_matrices': summary(tr[1:]), 'similar_aids': summary(top[1:]),
           'postings_walked': int(qb.sum()), 'small_tier_queries': int((qb <= similarity.SMALL_CAP).sum()),
           'large_tier_queries': int((qb > similarity.SMALL_CAP).sum()), 'largest_bound': int(qb.max()),
           'lists_full': int((n == K).sum())}
    large = int(qb[qb > similarity.SMALL_CAP].sum())
    res['postings_walked_large_tier'] = large
    res['similar_aids']['algorithmic_GBps'] = 12 * (res['postings_walked'] + large) / np.median(top[1:]) / 1e6
    res['similar_aids']['queries_per_s'] = res['queries'] / np.median(top[1:]) * 1e3
    return res


def host_topk(aid, off):
    """the reference's calls: vectorizer, aid x aid cosine, per-row top-49 of the last aids"""
    from sklearn.feature_extraction.text import TfidfVectorizer
    from sklearn.metrics.pairwise import cosine_similarity
    docs = [' '.join(map(str, aid[off[s]:off[s + 1]])) for s in range(len(off) - 1)]
    vec = TfidfVectorizer()
    X = vec.fit_transform(docs)
    S = cosine_similarity(X.T, dense_output=False).tocsr()
    vocab = vec.vocabulary_
    total = 0
    for a in np.unique(aid[off[1:] - 1]):
        i = vocab.get(str(a))
        if i is None:
            continue
        b, e = S.indptr[i], S.indptr[i + 1]
        vals, idx = S.data[b:e], S.indices[b:e]
        keep = idx != i
        order = np.argsort(-vals[keep], kind='stable')[:K]
        total += len(order)
    return total, int(S.nnz)


def child(mode, n_sessions, dev):
    import torch
    aid, _, off, n_aids = sessions_on(dev, n_sessions)
    torch.cuda.synchronize(dev)
    if mode == 'device':
        from otto_amd.tfidf import similarity
        t0 = time.perf_counter()
        queries = last_aids(aid, off)
        ids, sim, n = similarity.similar_aids(similarity.fit_transform(aid, off, n_aids), queries, K)
        total = int(n.sum())
        t1 = time.perf_counter()
        return {'mode': mode, 'wall_s': t1 - t0, 'entries': total}
    h_aid, h_off = aid.cpu().numpy(), off.cpu().numpy()
    t0 = time.perf_counter()
    total, nnz = host_topk(h_aid, h_off)
    t1 = time.perf_counter()
    return {'mode': mode, 'wall_s': t1 - t0, 'entries': total, 'product_nnz': nnz}


def product_bytes(dev, n_sessions):
    """upper estimate of the aid x aid product's stored bytes: every session adds at most len^2 entries"""
    from otto_amd.tfidf import similarity
    aid, _, off, n_aids = sessions_on(dev, n_sessions)
    row_off, _, _, _ = similarity.count(aid, off, n_aids)
    lens = (row_off[1:] - row_off[:-1]).double()
    return float((lens * lens).sum()) * 12


def run_child(mode, n):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode, '--sessions', str(n)], stdout=subprocess.PIPE, text=True,
                       check=True, timeout=1500)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=2_000_000)
    ap.add_argument('--host-budget-gb', type=float, default=8.0)
    ap.add_argument('--host-seconds', type=float, default=120.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tfidf', 'perf_tfidf.json'))
    ap.add_argument('--child', choices=('device', 'host'))
    args = ap.parse_args()
    import torch
    from otto_amd import _lib
    _lib.lib()
    dev = torch.device('cuda:0')
    if args.child:
        print(json.dumps(child(args.child, args.sessions, dev)))
        return
    res = {'device': torch.cuda.get_device_name(0), 'kernels': device_figures(dev, args.sessions), 'host_search': [], 'end_to_end': []}
    print(json.dumps(res['kernels'], indent=1), flush=True)
    torch.cuda.empty_cache()
    n, held = 1_250, None
    while n <= args.sessions:
        est = product_bytes(dev, n)
        if est > args.host_budget_gb * 2 ** 30:
            res['host_search'].append({'sessions': n, 'estimated_product_bytes': est, 'run': False})
            break
        r = run_child('host', n)
        res['host_search'].append({'sessions': n, 'estimated_product_bytes': est, 'run': True, **r})
        print(res['host_search'][-1], flush=True)
        held = n
        if r['wall_s'] > args.host_seconds / 2:                # the next doubling would leave the time the comparison may take
            break
        n *= 2
    res['host_sessions'] = held
    if held is None:
        print(f'the product of {n} sessions is estimated above the budget of {args.host_budget_gb} GB: no comparison', flush=True)
    for rep in range(3 if held is not None else 0):
        for mode in ('host', 'device'):
            res['end_to_end'].append(run_child(mode, held))
            print(res['end_to_end'][-1], flush=True)
    if held is not None:
        for mode in ('host', 'device'):
            walls = [r['wall_s'] for r in res['end_to_end'] if r['mode'] == mode]
            res[f'{mode}_wall_s'] = {'median': float(np.median(walls)), 'min': min(walls), 'max': max(walls)}
        res['speedup_at_host_sessions'] = res['host_wall_s']['median'] / res['device_wall_s']['median']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
