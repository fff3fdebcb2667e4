"""Inputs aimed at the HAND-OVER between two work items of one workgroup of the covisitation reduce kernel (``k_reduce`` in
``csrc/otto_covis.hip``): the item pipeline in the last wave, the next-item warm-up during the single-wave selection phases
and the table that one item leaves to the next. Shared by tests/test_reduce_handover_inputs_cpu.py (which proves from the
restated geometry that every stream has the shape claimed here) and tests/test_covis_reduce_handover_gpu.py. Plain NumPy.

A workgroup of a multi-wave kernel reserves 2 x DQ = 8 work indices at its first dequeue: whichever workgroup dequeues
first gets indices 0 .. 7. A kernel whose work list has at most 8 entries therefore runs all of them in ONE workgroup, in
list order: the smallest shape in which every item is handed over to the next. The work list of the M bin is the item
list (aids ascending); a heavy layout's list is pilot first (the first partition of every aid of the layout, aids
ascending, then the other partitions aid by aid: k_fill_order).

Restated here beyond tests/reduce_inputs.py:
    k_reduce: DQ = 4                   work indices a multi-wave workgroup reserves per dequeue (twice that at the first)
    k_reduce: SH, SHR = 4              the single-wave selection serves an item with k <= heavy keys <= 64 * SHR
    k_reduce: WARM_B = 4               64 * WARM_B run descriptors of the next item are warmed
    k_reduce: pshift / pmask           partition of a key in a heavy aid of 2^lg partitions: the lg hash bits below the slot
    k_fill_order                       pilot-first order of a heavy layout
An M item of ONE run does not exist (a run holds at most 29 records, the bin starts at 385): the case uses the fewest
runs an M aid can have, 14.

NOT REACHABLE from a stream, and therefore not covered here: an M item whose single-wave (SH) candidate list exceeds EXCAP
and takes the exact fallback. The kernel's keys are totally ordered (weight, then the smaller aid_y), so keys that tie in
weight do not tie for the kernel; the SH threshold is the k-th best LANE best, exactly k lanes hold a key at or above it and
a lane holds at most SHR = 4 keys, so more than 64 candidates need 17 to 64 of the best keys packed four to a lane in k
lanes. Which lane holds which key follows from the order in which the waves entered the keys into the table (the order of
the runs inside an aid is unspecified), which no input controls and no statistic reports. m5 below is an item with ties
at the k-th WEIGHT (110 keys at or above it); it takes the ordinary SH path. The same holds for the list overflows of the
two-pass path (P3, `s_more`): which keys share a lane or a group is not controlled by the input. What the L cases below fix
is the number of keys of each weight class per hash partition; the outcome of a guess follows from it IF the pilot leaves a
two-click threshold (at least 32 of its 64 group bests valid), which is the common case but is not proved here.
"""
import numpy as np

import reduce_inputs as ri
from reduce_inputs import Case, Target

DQ = 4
FIRST_RESERVE = 2 * DQ
SH_MAX_HEAVY = 256
WARM_RUNS = 64 * 4
KS = (20, 32)


def partition_of(y, log2t, lg):
    """Hash partition of key y in a heavy aid of 2^lg partitions reduced in a 2^log2t table."""
    h = (np.asarray(y, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(32 - log2t - lg)) & np.uint64((1 << lg) - 1)).astype(np.int64)


def ids_in_partitions(sizes, base, log2t, lg):
    """sizes[p] ascending ids >= base per partition p; returns a list of arrays."""
    need = max(sizes)
    y = np.arange(base, base + (need + 64) * (2 << lg) * 2, dtype=np.int64)
    part = partition_of(y, log2t, lg)
    out = []
    for p, m in enumerate(sizes):
        ids = y[part == p][:m]
        assert len(ids) == m
        out.append(ids)
    return out


def clicks(d, c):
    rows = np.zeros((d, 3), dtype=np.int64)
    rows[:, 0] = c
    return rows


def work_order(ev, kernel, packed_heavy=2, l_cap=ri.L_CAP):
    """[(aid, partition, log2 partitions)] in the order the kernel's work list holds them."""
    n, runs = ri.records_runs(ev)
    aids = [(int(x), ri.kernel_of(int(n[x]), int(runs[x]), packed_heavy, l_cap)) for x in np.flatnonzero(n)]
    aids = [(x, items) for x, (kern, items) in aids if kern == kernel]
    lg = lambda items: items.bit_length() - 1
    if kernel in ('S', 'M'):
        return [(x, 0, 0) for x, _ in aids]
    return [(x, 0, lg(c)) for x, c in aids] + [(x, p, lg(c)) for x, c in aids for p in range(1, c)]


# ---------------------------------------------------------------------------------------------------------------------
# M bin: 8 items in one workgroup
# ---------------------------------------------------------------------------------------------------------------------
def _m(name, counts, runs, kind, **expect):
    counts = np.asarray(counts)
    heavy = int((~ri.is_light(counts)).sum())
    return Target(name=name, counts=counts, runs=runs, expect={'kernel': {2: ('M', 1)}, 'heavy': heavy, 'path': kind, **expect})


def _m_targets():
    few_runs = ri._shuffled(np.r_[ri.heavy_rows(40), ri.singles(270)], 1)
    n_few = int(few_runs.sum())
    many = ri.heavy_and_light(50, 2800, seed=2)
    tie = ri.tie_counts(100, 10, 700, seed=5)
    return (
        # the fewest runs an M aid can have: one descriptor batch, mostly empty
        _m('m0-fewest-runs', few_runs, -(-n_few // (ri.MAX_SESSION - 1)), 'sh'),
        # one record per run: more runs than the warm-up touches, several descriptor batches per wave
        _m('m1-many-runs', many, int(many.sum()), 'sh'),
        _m('m2-not-sh', ri.heavy_and_light(300, 600, seed=3), ri.long_runs(int(ri.heavy_and_light(300, 600, seed=3).sum())), 'two-pass'),
        _m('m3-sh-again', ri.heavy_and_light(100, 800, seed=4), ri.long_runs(int(ri.heavy_and_light(100, 800, seed=4).sum())), 'sh'),
        # fewer than k heavy keys for k = 20 and k = 32: the walks are redone over every key
        _m('m4-ten-heavy', ri.heavy_and_light(10, 900, seed=6), ri.long_runs(int(ri.heavy_and_light(10, 900, seed=6).sum())), 'redo'),
        # 10 keys of three clicks, then 100 keys of two clicks tie at the k-th weight: the rows must order the tie by aid_y.
        # (NOT the SH list overflow: the kernel's keys are distinct, see the module docstring)
        _m('m5-weight-ties', tie, ri.long_runs(int(tie.sum())), 'sh', ge_kth={20: 110, 32: 110}),
        # a small item behind it: a slot left from m5 would add keys or weight to these rows
        _m('m6-small-after', ri.heavy_and_light(33, 360, seed=7), ri.long_runs(int(ri.heavy_and_light(33, 360, seed=7).sum())), 'sh'),
        # the last item of the list: there is no next item
        _m('m7-last', ri.heavy_and_light(12, 1200, seed=8), ri.long_runs(int(ri.heavy_and_light(12, 1200, seed=8).sum())), 'redo'),
    )


# ---------------------------------------------------------------------------------------------------------------------
# L 2^13 x 512: one aid, 8 partitions, every guess outcome
# ---------------------------------------------------------------------------------------------------------------------
L512_LCAP = 1024
L512_LG = 3
# partition -> (keys of three clicks, keys of two clicks, keys of one click)
# (the outcomes named here hold when the pilot leaves a two-click key as the threshold guess: see the module docstring)
L512_PARTS = ((0, 510, 0),       # pilot: 510 keys of two clicks and nothing else: every threshold it can leave is a two-click key
              (40, 0, 400),      # 40 keys above any two-click key: k <= 40 <= 64, the ranked list of the guess is the result
              (10, 0, 400),      # 10 < k keys above it: too few, two-pass path
              (100, 0, 300),     # 100 > 64 keys above it: the guess list overflows, two-pass path
              (40, 0, 400), (33, 0, 350), (64, 0, 300), (45, 0, 420))


def _l512_target():
    sizes = [a + b + c for a, b, c in L512_PARTS]
    ids = ids_in_partitions(sizes, 1000, 13, L512_LG)
    counts = np.concatenate([np.r_[clicks(a, 3), clicks(b, 2), clicks(c, 1)] for a, b, c in L512_PARTS])
    n = int(counts.sum())
    return Target(name='l512-eight-partitions', counts=counts, runs=ri.long_runs(n), partner_ids=np.concatenate(ids),
                  expect={'kernel': {2: ('L13x512', 8)}})


# ---------------------------------------------------------------------------------------------------------------------
# L 2^13 x 512: whole-aid gather items between partition buckets (l_cap = 4000)
# ---------------------------------------------------------------------------------------------------------------------
GB_LCAP = 4000


def _gather_bucket_targets():
    a = ri.heavy_and_light(60, 3000, seed=11)
    b = ri.mixed(8100, seed=12)
    d = ri.heavy_and_light(45, 3050, seed=13)
    return (Target(name='gb-a-whole', counts=a, runs=ri.long_runs(int(a.sum())), expect={'kernel': {2: ('L13x512', 1)}}),
            Target(name='gb-b-four-partitions', counts=b, runs=3000, expect={'kernel': {2: ('L13x512', 4)}}),
            Target(name='gb-d-whole', counts=d, runs=ri.long_runs(int(d.sum())), expect={'kernel': {2: ('L13x512', 1)}}))


# ---------------------------------------------------------------------------------------------------------------------
# the 1024-thread kernels (PREF), l_cap = 5000, packed_heavy = 1: in each of them a whole-aid gather item, the pilot bucket
# of a partitioned aid, a second whole-aid gather item, then the sibling buckets -- the last of them the largest item
# ---------------------------------------------------------------------------------------------------------------------
PREF_LCAP = 5000
PREF_LG = 2
# partition -> (keys of three clicks, keys of one click)
PREF_PARTS = {'L14': ((40, 4780), (40, 4780), (40, 4780), (40, 6880)),       # 4900, 4900, 4900, 7000 records
              'Lwide': ((40, 1646), (40, 1646), (40, 1646), (40, 4680))}     # 1766, 1766, 1766, 4800 records
PREF_LOG2T = {'L14': 14, 'Lwide': 13}


def _partitioned(name, kernel, base, runs):
    parts = PREF_PARTS[kernel]
    ids = ids_in_partitions([a + c for a, c in parts], base, PREF_LOG2T[kernel], PREF_LG)
    counts = np.concatenate([np.r_[clicks(a, 3), clicks(c, 1)] for a, c in parts])
    n = int(counts.sum())
    return Target(name=name, counts=counts, runs=runs(n), partner_ids=np.concatenate(ids), expect={'kernel': {1: (kernel, 4)}})


def _pref_targets():
    a14, d14 = ri.heavy_and_light(60, 5100, seed=21), ri.heavy_and_light(45, 5300, seed=22)
    aw, dw = ri.heavy_and_light(50, 4050, seed=23), ri.heavy_and_light(45, 4100, seed=24)
    whole = lambda name, c, kernel, runs: Target(name=name, counts=c, runs=runs, expect={'kernel': {1: (kernel, 1)}})
    return (whole('p14-a-whole', a14, 'L14', ri.long_runs(int(a14.sum()))),
            _partitioned('p14-b-four-partitions', 'L14', 20000, lambda n: 3000),
            whole('p14-d-whole', d14, 'L14', ri.long_runs(int(d14.sum()))),
            whole('pw-a-whole', aw, 'Lwide', int(aw.sum())),
            _partitioned('pw-b-four-partitions', 'Lwide', 200000, lambda n: n),
            whole('pw-d-whole', dw, 'Lwide', int(dw.sum())))


# ---------------------------------------------------------------------------------------------------------------------
# LDS table overflow: 9000 distinct keys in the 2^13-slot wide table, then a small wide item in the same workgroup
# ---------------------------------------------------------------------------------------------------------------------
OVF_LCAP = 10000


def _ovf_targets():
    g = ri.heavy_and_light(50, 4200, seed=31)
    return (Target(name='ovf-9000-keys', counts=ri.singles(9000), runs=9000, expect={'kernel': {2: ('Lwide', 1)}}),
            Target(name='ovf-small-after', counts=g, runs=int(g.sum()), expect={'kernel': {2: ('Lwide', 1)}}))


_HOT = ({}, {'guess': 0}, {'hot': 0}, {'hot': 1}, {'hot': 2})

CASES = (
    Case('handover-m', _m_targets(), option_sets=_HOT, ks=KS),
    Case('handover-l512-guess', (_l512_target(),), option_sets=tuple({'l_cap': L512_LCAP, **o} for o in _HOT), ks=KS),
    Case('handover-l512-gather-bucket', _gather_bucket_targets(), option_sets=({'l_cap': GB_LCAP}, {'l_cap': GB_LCAP, 'guess': 0}), ks=KS),
    Case('handover-pref', _pref_targets(), option_sets=({'l_cap': PREF_LCAP, 'packed_heavy': 1}, {'l_cap': PREF_LCAP, 'packed_heavy': 1, 'guess': 0}),
         ks=KS),
    Case('handover-ovf', _ovf_targets(), option_sets=({'l_cap': OVF_LCAP},), ks=KS, min_retries={0: 1}),
)
CASE_BY_NAME = {c.name: c for c in CASES}
