"""Inputs aimed at the PROCESSING ORDER of the partition-pass chunks (``order_chunks`` / ``k_chunk_keys`` / ``k_ord_scatter``
in ``csrc/otto_covis.hip``, options ``part_order`` and ``part_q``). Shared by tests/test_part_order_inputs_cpu.py (which
proves from the oracle's records and runs that every stream has the chunks claimed here) and tests/test_covis_part_order_gpu.py.
Plain NumPy.

Restated here beyond tests/reduce_inputs.py:
    PART_CHUNK_RUNS = 256              runs per partition-pass chunk
    ChunkCount                         an aid has chunks if it is an L aid of more than one hash partition: ceil(runs / 256)
    ORD_KEY_RUNS = 64                  descriptors of a chunk that k_chunk_keys looks at for a shared list
    part_q                             bins of the counting sort (default 1024, at most 2048)

A small `l_cap` puts small aids through the partition pass: with l_cap = 1024 and fewer than 4096 runs an aid of more than
2048 records (and more than M_CAP = 3072, or it is no L aid) is reduced in partitions of 1024 records.

The spoke streams (tests/reduce_inputs.py) have one shared list per session, so every chunk of theirs starts with a run that
reads a shared list. `gap_stream` below adds what they lack: windows that are ONE time-connected component but no clique
(the general row loop: every run of the window is a private row), and windows cut in two components in which the hub meets
partners again (its run of the second component is a private row).
"""
import numpy as np

import reduce_inputs as ri
from reduce_inputs import Case, Target
from otto_amd.synth import Events

PART_CHUNK_RUNS = 256
ORD_KEY_RUNS = 64
DEFAULT_Q = 1024
LCAP = 1024
TYPE3 = ('click_weighted', 'cart_weighted', 'order_weighted')
TIMED = TYPE3 + ('time_weighted',)


def chunks_per_aid(n, runs, l_cap, packed_heavy=2):
    """int64 [n_aids]: partition-pass chunks of every aid (ChunkCount), from its records and runs."""
    out = np.zeros(len(n), dtype=np.int64)
    for x in np.flatnonzero(n > ri.M_CAP):
        _, items = ri.kernel_of(int(n[x]), int(runs[x]), packed_heavy, l_cap)
        if items > 1:
            out[x] = -(-int(runs[x]) // PART_CHUNK_RUNS)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# spoke streams
# ---------------------------------------------------------------------------------------------------------------------
def _t(name, counts, runs, items):
    return Target(name=name, counts=counts, runs=runs, expect={'kernel': {2: ('L13x512', items)}})


_DOM_KEY, _DOM_N = 3000, 4000

SPOKE = (
    # two partitioned aids of 3 chunks each: 6 chunks, no multiple of the 4 a workgroup dequeues at a time
    Case('two-aids', (_t('a-600-runs', ri.mixed(4000, seed=41), 600, 4), _t('b-700-runs', ri.mixed(5000, seed=42), 700, 8)),
         option_sets=({'l_cap': LCAP},)),
    # 200 runs: exactly one chunk in all
    Case('one-chunk', (_t('a-200-runs', ri.mixed(4000, seed=43), 200, 4),), option_sets=({'l_cap': LCAP},)),
    # one key holds 3000 of the aid's 4000 records: its partition overflows a sized bucket (2 * 1000 + 256 records), the aid is
    # flagged and redone in an exact round (count pass + scatter pass, both over the ordered chunks)
    Case('dominant-key', (_t('a-3100-runs', np.r_[[[_DOM_KEY, 0, 0]], ri.mixed(_DOM_N - _DOM_KEY, seed=44)], 3100, 4),),
         option_sets=({'l_cap': LCAP},), other_max=ri.L_CAP, min_retries={0: 1}),
)
SPOKE_BY_NAME = {c.name: c for c in SPOKE}
assert ri.bucket_cap(_DOM_N, 2) < _DOM_KEY
# chunks in all, per case (proved in tests/test_part_order_inputs_cpu.py)
# (dominant-key: 13 of the target and 12 of the key itself, whose 3000 runs hold the target 3000 times)
SPOKE_CHUNKS = {'two-aids': 6, 'one-chunk': 1, 'dominant-key': 25}


# ---------------------------------------------------------------------------------------------------------------------
# windows with gaps above max_gap and repeated partners
# ---------------------------------------------------------------------------------------------------------------------
MAX_GAP = 86400
# per hub: sessions of each shape, in stream order (the runs of an aid follow session order in the index)
#   chain : hub, 8 partners 50,000 s later, 8 partners another 50,000 s later. Neighbours are within max_gap, the ends are not:
#           one component, no clique -> general row loop, every run a private row. The hub has 8 records in 1 run.
#   cut   : hub + 6 partners, then 200,000 s later the hub, 3 of the 6 and 4 new partners. Two cliques; in the second the hub has
#           met 3 aids before -> a private row of 4 records. The hub has 6 + 4 records in 2 runs.
#   plain : hub + 7 partners seconds apart: one clique, a shared list. 7 records in 1 run.
GAP_HUBS = {'hub-a': dict(chain=300, cut=200, plain=200), 'hub-b': dict(chain=150, cut=200, plain=200)}
GAP_POOL = 3000                                    # partner ids 2 .. 2 + GAP_POOL


def gap_hub_shape(name):
    s = GAP_HUBS[name]
    return dict(n=8 * s['chain'] + 10 * s['cut'] + 7 * s['plain'], runs=s['chain'] + 2 * s['cut'] + s['plain'],
                private_runs=s['chain'] + s['cut'])


_gap = {}


def gap_stream():
    """(Events, {hub name: aid})"""
    if _gap:
        return _gap['ev'], _gap['hubs']
    rng = np.random.default_rng(7)
    hubs = {name: i for i, name in enumerate(GAP_HUBS)}
    aid, ts, lens = [], [], []
    t0 = ri.T0
    for name, shape in GAP_HUBS.items():
        h = hubs[name]
        for kind in ('chain', 'cut', 'plain'):
            for _ in range(shape[kind]):
                p = 2 + rng.choice(GAP_POOL, 17, replace=False)
                if kind == 'chain':
                    a = np.r_[h, p[:16]]
                    t = np.r_[0, 50000 + np.arange(8), 100000 + np.arange(8)]
                elif kind == 'cut':
                    a = np.r_[h, p[:6], h, p[:3], p[6:10]]
                    t = np.r_[np.arange(7), 200000 + np.arange(8)]
                else:
                    a = np.r_[h, p[:7]]
                    t = np.arange(8)
                aid.append(a); ts.append(t0 + t); lens.append(len(a))
                t0 += 400000
    aid = np.concatenate(aid)
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    typ = rng.choice(3, len(aid), p=(0.8, 0.12, 0.08))
    ev = Events(aid=aid.astype(np.uint32), ts=np.concatenate(ts).astype(np.int32), type=typ.astype(np.uint8), sess_off=off,
                n_aids=2 + GAP_POOL)
    assert int(ev.ts.max()) < 2 ** 31 - 1
    _gap['ev'], _gap['hubs'] = ev, hubs
    return ev, hubs


GAP_CHUNKS = 7                                     # hub-a: 900 runs -> 4, hub-b: 750 runs -> 3

# ---------------------------------------------------------------------------------------------------------------------
# GPU runs: (stream, kinds, feed() calls, options beside l_cap and part_order)
# ---------------------------------------------------------------------------------------------------------------------
RUNS = (
    ('two-aids', TYPE3, 1, {}),                    # 6 chunks: fewer than Q = 1024, no multiple of 4
    ('two-aids', TYPE3, 1, {'part_q': 4}),         # more chunks than bins
    ('two-aids', TYPE3, 1, {'part_q': 2048}),      # the most bins
    ('two-aids', TYPE3, 2, {}),                    # two feed() calls: two list regions
    ('two-aids', TIMED, 1, {}),                    # the time channel travels with the records
    ('one-chunk', TYPE3, 1, {}),
    ('dominant-key', TYPE3, 1, {}),                # exact retry round
    ('dominant-key', TYPE3, 1, {'part_q': 2}),
    ('dominant-key', TIMED, 1, {'part_sized': 0}), # counted buckets from the start
    ('gaps', TYPE3, 1, {}),
    ('gaps', TIMED, 2, {}),
    ('gaps', TIMED, 1, {'part_q': 2}),
)
