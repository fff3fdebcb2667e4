"""Times of the objectives and metrics of SPEC-OBJ (include/otto_objective.h) ->
profiles/objectives/perf_objectives.json.

2^24 rows in queries of 50. Timed, alternated inside every repeat so that all see the same power state: ``otto_obj_binary``
against ``otto_gbdt_quantize`` (the streaming kernel whose HBM rate it should sit near; both rates over their algorithmic
bytes per row: 12 in and 16 out; 16 for the maxima, then 16 in and 8 out), ``otto_obj_ndcg_at_k`` against ``otto_gbdt_ap_at_k``, ``otto_xgb_lambdamart`` with the NDCG
weights against the same call without them (``weighting = 0``, ``rank:pairwise``) and ``otto_gbdt_lambdarank``, ``otto_obj_auc`` against the 64-bit radix sort of as many
keys (``otto_events_sort`` stands in: a pair sort plus one scan), ``otto_obj_logloss`` and ``otto_obj_label_counts``. Device
events, 1 warm-up and 5 repeats, median (min - max).

``--only-pairwise`` times ``xgb.pairwise_gradients`` alone after the set-up and prints one JSON line; ``--root DIR`` imports the
package from another checkout of this repository (built there). Alternating the two in one job is how the pairwise kernel
is compared with the commit before the NDCG template parameter, since kernel times move by several per cent with the chip's
power state.

    python tools/perf_objectives.py [--rows 16777216] [--query 50] [--repeats 5] [--only-pairwise] [--root DIR]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12     # bytes / s, MI355X data sheet

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1 << 24)
ap.add_argument('--query', type=int, default=50)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--only-pairwise', action='store_true')
ap.add_argument('--root', default=ROOT)
ap.add_argument('--out', default=os.path.join('profiles', 'objectives', 'perf_objectives.json'))
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import torch

from otto_amd import _lib
from otto_amd.ranker import gbdt, xgb


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns):
    """{name: spread of ms}: one call of each per repeat, in the order given; the first round is the warm-up."""
    ms = {k: [] for k in fns}
    for r in range(a.repeats + 1):
        for k, fn in fns.items():
            t = event_ms(fn)
            if r:
                ms[k].append(t)
    return {k: spread(v) for k, v in ms.items()}


dev = torch.device('cuda:0')
n = a.rows
g = torch.Generator(device=dev).manual_seed(1)
off = torch.arange(0, n + a.query, a.query, dtype=torch.int64, device=dev).clamp_(max=n)
score = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
label = (torch.rand(n, generator=g, device=dev) < 0.04).to(torch.int32)
seed = xgb.derived_seeds(0)[0]
grad, hess = torch.empty_like(score), torch.empty_like(score)

if a.only_pairwise:
    out = dict(root=os.path.abspath(a.root), rows=n, query=a.query,
               pairwise_ms=alternate({'pairwise': lambda: xgb.pairwise_gradients(score, label, off, seed, 0, out=(grad, hess))})['pairwise'])
    print(json.dumps(out))
    sys.exit(0)

from otto_amd.ranker import objectives

Q = off.numel() - 1
ap_out = torch.empty(Q, dtype=torch.float64, device=dev)
auc_work = _lib.workspace(_lib.lib().otto_obj_auc_workspace_bytes(n), dev)
sort_work = _lib.workspace(_lib.lib().otto_events_sort_workspace(n), dev)
# uint32 columns travel as int32 bit patterns, as in otto_amd.events
session = torch.randint(0, (1 << 31) - 1, (n,), generator=g, device=dev, dtype=torch.int32)
ts = torch.randint(0, (1 << 31) - 1, (n,), generator=g, device=dev, dtype=torch.int64)
aid = torch.zeros(n, dtype=torch.int32, device=dev)
typ = torch.zeros(n, dtype=torch.uint8, device=dev)
s_aid, s_ts, s_type = torch.empty_like(aid), torch.empty(n, dtype=torch.int32, device=dev), torch.empty_like(typ)
s_off, s_id = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
import ctypes as C
n_sessions = C.c_int64(0)


def radix_sort():
    # 64 varying key bits (session, second), as the AUC's score keys have
    _lib.call('otto_events_sort', dev, session, ts, aid, typ, n, 1, s_aid, s_ts, s_type, None, s_off, s_id, C.byref(n_sessions),
              sort_work, sort_work.numel())


times = {}
times.update(alternate({
    'obj_binary': lambda: objectives.binary_gradients(score, label, 1.0, 1.0, 1.0, 0.0, out=(grad, hess)),
    'gbdt_quantize': lambda: gbdt.quantize_gradients(grad, hess),
}))
times.update(alternate({
    'obj_ndcg_at_20': lambda: objectives.ndcg_at_k(score, label, off, 20),
    'gbdt_ap_at_20': lambda: gbdt.ap_at_k(score, label, off, 20),
}))
times.update(alternate({
    'xgb_lambdamart_ndcg': lambda: xgb.lambdamart_gradients(score, label, off, seed, 0, 1, out=(grad, hess)),
    'xgb_pairwise': lambda: xgb.pairwise_gradients(score, label, off, seed, 0, out=(grad, hess)),
    'gbdt_lambdarank': lambda: gbdt.lambdarank_gradients(score, label, off, out=(grad, hess)),
}))
times.update(alternate({
    'obj_auc': lambda: objectives.auc_counts(score, label, auc_work),
    'events_sort_64_bit_keys': radix_sort,
}))
times.update(alternate({
    'obj_logloss': lambda: objectives.logloss_sum(score, label),
    'obj_label_counts': lambda: objectives.label_counts(label),
}))
med = lambda k: times[k]['median']
out = dict(
    device=torch.cuda.get_device_name(0), rows=n, query=a.query, repeats=a.repeats, ms=times,
    obj_binary_share_of_hbm_peak=round(n * 28 / (med('obj_binary') * 1e-3) / HBM_PEAK, 3),
    gbdt_quantize_share_of_hbm_peak=round(n * 40 / (med('gbdt_quantize') * 1e-3) / HBM_PEAK, 3),
    ndcg_over_ap=round(med('obj_ndcg_at_20') / med('gbdt_ap_at_20'), 3),
    rank_ndcg_over_rank_pairwise=round(med('xgb_lambdamart_ndcg') / med('xgb_pairwise'), 3),
    auc_over_sort=round(med('obj_auc') / med('events_sort_64_bit_keys'), 3))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')
print(json.dumps(out))
