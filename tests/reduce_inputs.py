"""Inputs aimed at the capacities of the covisitation reduce kernel (``k_reduce`` and its host side in
``csrc/otto_covis.hip``), shared by tests/test_reduce_inputs_cpu.py (which proves that every input has the shape its
name claims) and tests/test_covis_reduce_edges_gpu.py (which compares the device rows with the oracle). Plain NumPy;
nothing here touches a device.

Geometry restated here from csrc/otto_covis.hip (the code is the authority; the constants are named as they are there):
    S_CAP / M_CAP / L_CAP, *_LOG2T, *_THREADS      "size bins of the reduce kernel": an aid of n records is S (n <= 384, 2^9
                                                   slots, 1 wave), M (n <= 3072, 2^12 slots, 4 waves), else L
    PACKED_MAX_RUNS, heavy_mode(), heavy_log2t()   layout of an L aid: 0 wide (2^13 slots, 1024 threads), 1 packed 2^14 slots
                                                   / 1024 threads, 2 packed 2^13 slots / 512 threads
    l_log2r()                                      log2 of the hash partitions of an L aid
    bucket_cap(), ItemCap                          records a sized partition bucket holds (2 x mean + 256)
    k_reduce: EXCAP, CCAP, LISTCAP, OCAP, RCAP     candidate lists, compacted list of the one-wave bin, dense list of
                                                   occupied slots (OCAP entries, RCAP per wave)
    k_reduce, "HEAVY FIRST"                        a key is light when its counters are exactly ONE click record
    ITEM_BLOCK_AIDS                                aids per workgroup of k_aid_totals / k_items_fill
    launch_reduce()                                which instantiation serves which bin / layout
"""
from dataclasses import dataclass, field

import numpy as np

from otto_amd.synth import Events

Q16 = 65536
S_CAP, M_CAP, L_CAP = 384, 3072, 6144
PACKED_MAX_RUNS = 4096
EXCAP, CCAP, LISTCAP = 64, 256, 384
ITEM_BLOCK_AIDS = 2048
MAX_K = 32
MAX_SESSION = 30                       # window of the builds: sessions of at most 30 events lose no event

# the five instantiations of k_reduce per group: slots, threads, records that fit for certain (in units of l_cap for the L
# layouts), dense list entries in all and per wave
KERNELS = {
    'S': dict(log2t=9, threads=64, cap=S_CAP, ocap=None, rcap=None),
    'M': dict(log2t=12, threads=256, cap=M_CAP, ocap=1920, rcap=480),
    'L13x512': dict(log2t=13, threads=512, cap=L_CAP, ocap=4608, rcap=576),
    'L14': dict(log2t=14, threads=1024, cap=2 * L_CAP, ocap=10240, rcap=640),
    'Lwide': dict(log2t=13, threads=1024, cap=L_CAP, ocap=6144, rcap=384),
}
for _k in KERNELS.values():
    assert _k['ocap'] is None or _k['rcap'] == _k['ocap'] // (_k['threads'] // 64)
MODE_KERNEL = {0: 'Lwide', 1: 'L14', 2: 'L13x512'}


def bin_of(n):
    return 'S' if n <= S_CAP else ('M' if n <= M_CAP else 'L')


def heavy_mode(n, runs, packed_heavy=2, l_cap=L_CAP):
    """Layout of an L aid of n records in `runs` runs (0 wide, 1 packed 2^14, 2 packed 2^13)."""
    if not packed_heavy or runs >= PACKED_MAX_RUNS:
        return 0
    if packed_heavy == 2:
        return 2 if (n <= l_cap or n > 2 * l_cap) else 1
    return 2 if n <= l_cap else 1


def log2_parts(n, runs, packed_heavy=2, l_cap=L_CAP, boost=0):
    mode = heavy_mode(n, runs, packed_heavy, l_cap)
    cap = 2 * l_cap if mode == 1 else l_cap
    parts = -(-n // cap)
    lg = 0
    while (1 << lg) < parts:
        lg += 1
    return min(lg + boost, 32 - (14 if mode == 1 else 13))


def kernel_of(n, runs, packed_heavy=2, l_cap=L_CAP):
    """(instantiation, work items) of an aid of n records in `runs` runs."""
    b = bin_of(n)
    if b != 'L':
        return b, 1
    return MODE_KERNEL[heavy_mode(n, runs, packed_heavy, l_cap)], 1 << log2_parts(n, runs, packed_heavy, l_cap)


def bucket_cap(n, lg_parts):
    """Records a partition bucket holds when the buckets are sized from the aid's record count (no count pass)."""
    return 0 if lg_parts == 0 else 2 * ((n + (1 << lg_parts) - 1) >> lg_parts) + 256


def dense_certain(kernel, d):
    """True: the dense list of occupied slots holds every key whatever the hash does (no wave can enter more than all d keys);
    False: it cannot (more keys than OCAP: some wave is over RCAP); None: depends on how the keys fall on the waves."""
    g = KERNELS[kernel]
    return True if d <= g['rcap'] else (False if d > g['ocap'] else None)


def is_light(counts):
    """[d, 3] (clicks, carts, orders) -> bool [d]: the key is exactly one click record."""
    c = np.asarray(counts)
    return (c[:, 0] == 1) & (c[:, 1] == 0) & (c[:, 2] == 0)


def ge_kth(w, k):
    """Number of keys whose weight is at least the k-th largest weight (all of them when there are at most k)."""
    w = np.sort(np.asarray(w))[::-1]
    return len(w) if len(w) <= k else int((w >= w[k - 1]).sum())


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------
T0 = 1_660_000_000


@dataclass
class Target:
    """An aid x whose records are known in advance: partner number i is met counts[i] = (clicks, carts, orders) times (the
    type of a record (x, y) is the type of y's event), in exactly `runs` sessions. `aid`: an id, 'last' (n_aids - 1) or None
    (any). `expect`: what the case claims beyond n, runs and d -- 'kernel': {packed_heavy: (instantiation, work items)},
    'heavy': keys that are not one click record, 'ge_kth': {k: keys at or above the k-th click_weighted weight},
    'dense': see dense_certain, 'top_w': {kind: Q16 weight of the best key}."""
    name: str
    counts: np.ndarray
    runs: int
    aid: object = None
    x_type: int = 0
    at_ts_max: bool = False
    partner_ids: object = None                 # ids of the partners (default: the next free ones)
    expect: dict = field(default_factory=dict)

    @property
    def n(self):
        return int(np.asarray(self.counts).sum())

    @property
    def d(self):
        return len(self.counts)


def spoke_stream(targets, same_ts=False):
    """Events stream of sessions `x, p1 .. pm` (m <= 29, every aid of a session distinct, events one second apart) that gives
    every target exactly its records; partners of different targets come from disjoint id ranges. `same_ts`: every event
    of the stream carries one timestamp. A target with `at_ts_max` has all events of its sessions at the largest timestamp
    of the stream. Returns (Events, {target name: (aid of x, partner ids int64 [d])})."""
    reserved = [t.aid for t in targets if isinstance(t.aid, (int, np.integer))]
    reserved = np.unique(np.concatenate([np.asarray(reserved, dtype=np.int64)] +
                                        [np.asarray(t.partner_ids, dtype=np.int64) for t in targets if t.partner_ids is not None]))
    nxt = 0

    def take(m):
        nonlocal nxt
        cand = np.arange(nxt, nxt + m + len(reserved), dtype=np.int64)
        cand = cand[~np.isin(cand, reserved)][:m]
        if m:
            nxt = int(cand[-1]) + 1
        return cand

    ids = {}
    for t in targets:                                  # the targets' own ids first: partners fill the space around them
        if t.aid is None:
            ids[t.name] = int(take(1)[0])
        elif t.aid != 'last':
            ids[t.name] = int(t.aid)
    aids, types, lens, at_max, where = [], [], [], [], {}
    for t in targets:
        counts = np.asarray(t.counts, dtype=np.int64).reshape(-1, 3)
        d, tot = len(counts), counts.sum(axis=1)
        n = int(tot.sum())
        assert d and (tot >= 1).all() and tot.max() <= t.runs <= n and -(-n // t.runs) <= MAX_SESSION - 1, t.name
        pids = take(d) if t.partner_ids is None else np.asarray(t.partner_ids, dtype=np.int64)
        assert len(pids) == d
        where[t.name] = pids
        occ_p = np.repeat(np.arange(d), tot)           # a partner's occurrences are contiguous and at most `runs`: dealt
        occ_t = np.repeat(np.tile(np.arange(3), d), counts.ravel())   # round robin they fall into distinct sessions
        i = np.arange(n)
        sid, rank = i % t.runs, i // t.runs
        length = np.bincount(sid, minlength=t.runs) + 1
        off = np.r_[0, np.cumsum(length)]
        a = np.empty(off[-1], dtype=np.int64)
        ty = np.empty(off[-1], dtype=np.int64)
        a[off[:-1]], ty[off[:-1]] = -1, t.x_type       # x: filled in below ('last' is known only at the end)
        a[off[sid] + 1 + rank], ty[off[sid] + 1 + rank] = pids[occ_p], occ_t
        aids.append((t.name, a)); types.append(ty); lens.append(length); at_max.append(np.full(t.runs, t.at_ts_max))
    for t in targets:
        if t.aid == 'last':
            ids[t.name] = nxt
            nxt += 1
    n_aids = max(nxt, int(reserved.max()) + 1 if len(reserved) else 0)
    assert len(set(ids.values())) == len(ids)
    aid = np.concatenate([np.where(a < 0, ids[name], a) for name, a in aids])
    length = np.concatenate(lens)
    off = np.r_[0, np.cumsum(length)].astype(np.int64)
    sess = np.repeat(np.arange(len(length)), length)
    pos = np.arange(off[-1]) - off[sess]
    if same_ts:
        ts = np.full(off[-1], T0, dtype=np.int64)
    else:
        ts = T0 + 40 * sess + pos
        ts[np.concatenate(at_max)[sess]] = T0 + 40 * (len(length) + 1)
    ev = Events(aid=aid.astype(np.uint32), ts=ts.astype(np.int32), type=np.concatenate(types).astype(np.uint8), sess_off=off,
                n_aids=int(n_aids))
    return ev, {name: (ids[name], where[name]) for name in ids}


def records_runs(ev):
    """(records int64 [n_aids], runs int64 [n_aids]) of a spoke stream: every aid of a session is distinct and no gap is
    dropped, so an event of a session of L events stands for L - 1 records and (L >= 2) one run."""
    length = np.diff(ev.sess_off)
    per_event = np.repeat(length, length)
    n = np.bincount(ev.aid, weights=per_event - 1, minlength=ev.n_aids).astype(np.int64)
    runs = np.bincount(ev.aid, weights=per_event >= 2, minlength=ev.n_aids).astype(np.int64)
    return n, runs


def expected_items(ev, packed_heavy=2, l_cap=L_CAP):
    """{'items_s', 'items_m', 'items_l'} of the first reduce round, from the restated geometry."""
    n, runs = records_runs(ev)
    out = {'items_s': 0, 'items_m': 0, 'items_l': 0}
    for x in np.flatnonzero(n):
        kern, items = kernel_of(int(n[x]), int(runs[x]), packed_heavy, l_cap)
        out['items_' + kern[0].lower()] += items
    return out


# ---------------------------------------------------------------------------------------------------------------------
# partner multisets
# ---------------------------------------------------------------------------------------------------------------------
def _shuffled(rows, seed):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def singles(d, t=0):
    c = np.zeros((d, 3), dtype=np.int64)
    c[:, t] = 1
    return c


def one_key(n_key, n_single=0):
    """One key of n_key click records (the first partner id) and n_single keys of one click record."""
    return np.r_[[[n_key, 0, 0]], singles(n_single)]


def mixed(n, seed):
    """n records: 40 keys of 1 .. 6 records of one random type each, the rest single clicks; shuffled."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((40, 3), dtype=np.int64)
    rows[np.arange(40), rng.integers(0, 3, 40)] = rng.integers(1, 7, 40)
    assert n > rows.sum()
    return _shuffled(np.r_[rows, singles(n - int(rows.sum()))], seed)


def heavy_rows(h):
    """h heavy keys: one single cart record, one single order record (heavy although single), the others two to four
    clicks with a cart record on every fifth."""
    rows = [[0, 1, 0], [0, 0, 1]] + [[2 + i % 3, int(i % 5 == 0), 0] for i in range(h - 2)]
    return np.array(rows[:h], dtype=np.int64).reshape(-1, 3)


def heavy_and_light(h, light, seed):
    return _shuffled(np.r_[heavy_rows(h), singles(light)], seed)


def dense_counts(d, n, seed, heavy=37):
    """d keys, n records, `heavy` heavy keys among single clicks. n == d: the heavy keys are single cart / order records;
    else the records beyond d are spread over the heavy keys as clicks."""
    rows = singles(d)
    if n == d:
        rows[:heavy] = 0
        rows[np.arange(heavy), 1 + np.arange(heavy) % 2] = 1
    else:
        rows[0], rows[1] = (0, 1, 0), (0, 0, 1)
        extra = n - d
        assert extra >= heavy - 2
        share = np.full(heavy - 2, extra // (heavy - 2))
        share[:extra % (heavy - 2)] += 1
        rows[2:heavy, 0] += share
        rows[2:heavy:3, 2] += 1                        # some order records among them (n grows by the number of such rows)
    return _shuffled(rows, seed)


def tie_counts(two, three, light, seed):
    return _shuffled(np.r_[np.tile([[2, 0, 0]], (two, 1)), np.tile([[3, 0, 0]], (three, 1)), singles(light)], seed)


def few_keys(d, n, seed):
    """d keys that share n records, unequal, types mixed."""
    rng = np.random.default_rng(seed)
    tot = np.full(d, n // d) + rng.integers(-(n // d) // 6, (n // d) // 6 + 1, d)
    tot[0] += n - tot.sum()
    carts = tot // rng.integers(3, 9, d)
    orders = tot // rng.integers(5, 12, d)
    return np.c_[tot - carts - orders, carts, orders]


def home_slot(y, log2t):
    """First table slot a key probes (rec_hash in csrc/otto_covis.hip)."""
    return ((np.asarray(y, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2t)


def ids_without_collisions(d, base, log2t=9):
    """d ascending ids >= base whose first slots are all different -- no key probes further, so every key sits in its first slot
    whatever the insertion order -- and whose SMALLEST id has the LAST slot of the table: the walk over the slots meets
    the key that wins every tie last."""
    y = np.arange(base, base + 64 * (1 << log2t), dtype=np.int64)
    slot = home_slot(y, log2t).astype(np.int64)
    first = int(np.flatnonzero(slot == (1 << log2t) - 1)[0])
    out, used = [int(y[first])], {(1 << log2t) - 1}
    for yy, sl in zip(y[first + 1:].tolist(), slot[first + 1:].tolist()):
        if sl not in used:
            used.add(sl)
            out.append(yy)
            if len(out) == d:
                break
    assert len(out) == d
    return np.array(out, dtype=np.int64)


def long_runs(n):
    """Fewest sessions that hold n records, and one more (so that one session is shorter)."""
    return -(-n // (MAX_SESSION - 1)) + 1


# ---------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One stream. `option_sets`: the builder options of each GPU run (name -> value; 'l_cap' among them); `ks`: the k of
    each run; `other_max`: no aid that is not a target has more records than this; `min_retries`: {option set index: retries
    that are certain}."""
    name: str
    targets: tuple
    option_sets: tuple = ({},)
    ks: tuple = (20,)
    same_ts: bool = False
    other_max: int = S_CAP
    min_retries: dict = field(default_factory=dict)


def _t(name, counts, runs, **kw):
    return Target(name=name, counts=counts, runs=runs, **kw)


BIN_EDGE_N = (383, 384, 385, 3071, 3072, 3073, 6143, 6144, 6145, 12287, 12288, 12289, 12290)
# ids on both sides of the 2048-aid blocks of the work-list kernels and on the last aid; the heavy aids sit on the edges
BIN_EDGE_IDS = {383: 0, 384: 2046, 385: 2049, 3071: 4094, 3072: 4097, 3073: 1, 6143: 6143, 6144: 4096, 6145: 2047, 12287: 6144,
                12288: 2048, 12289: 4095, 12290: 'last'}
_W = {0: 'Lwide'}
# (instantiation, work items) under packed_heavy = 0 / 1 / 2 when the aid has FEWER than 4096 runs; with runs = n >= 4096 every
# L aid has the packed_heavy = 0 entry
BIN_EDGE_KERNELS = {
    383: ('S', 1), 384: ('S', 1), 385: ('M', 1), 3071: ('M', 1), 3072: ('M', 1),
    3073: {0: ('Lwide', 1), 1: ('L13x512', 1), 2: ('L13x512', 1)},
    6143: {0: ('Lwide', 1), 1: ('L13x512', 1), 2: ('L13x512', 1)},
    6144: {0: ('Lwide', 1), 1: ('L13x512', 1), 2: ('L13x512', 1)},
    6145: {0: ('Lwide', 2), 1: ('L14', 1), 2: ('L14', 1)},
    12287: {0: ('Lwide', 2), 1: ('L14', 1), 2: ('L14', 1)},
    12288: {0: ('Lwide', 2), 1: ('L14', 1), 2: ('L14', 1)},
    12289: {0: ('Lwide', 4), 1: ('L14', 2), 2: ('L13x512', 4)},
    12290: {0: ('Lwide', 4), 1: ('L14', 2), 2: ('L13x512', 4)},
}


def _bin_edge_targets(packed):
    out = []
    for i, n in enumerate(BIN_EDGE_N):
        # packed: fewer than 4096 runs -- 4095 of them (short sessions) for odd n, as few as possible (sessions of 30) for even n
        runs = n if not packed else (min(n, PACKED_MAX_RUNS - 1) if n % 2 else long_runs(n))
        kern = BIN_EDGE_KERNELS[n]
        if isinstance(kern, tuple):
            kern = {ph: kern for ph in (0, 1, 2)}
        elif runs >= PACKED_MAX_RUNS:
            kern = {ph: kern[0] for ph in (0, 1, 2)}
        out.append(_t(f'n{n}', mixed(n, seed=n), runs, aid=BIN_EDGE_IDS[n], x_type=i % 3, expect={'kernel': kern}))
    return tuple(out)


def _kern(k, items=1):
    return {'kernel': {2: (k, items)}}


_PH = ({'packed_heavy': 2}, {'packed_heavy': 1}, {'packed_heavy': 0})
_PACKED_RUNS = PACKED_MAX_RUNS - 1


def _table_load_targets():
    full = [('S', S_CAP, S_CAP), ('M', M_CAP, M_CAP), ('L13x512', L_CAP, _PACKED_RUNS), ('Lwide', L_CAP, L_CAP),
            ('L14', 2 * L_CAP, _PACKED_RUNS)]
    out = [_t(f'{k}-full', singles(n), runs, expect={**_kern(k), 'heavy': 0, 'ge_kth': {20: n}}) for k, n, runs in full]
    # one counter at its maximum: n at the cap, one key in every run (packed heavy layouts: 4095 runs, the other records singles)
    out += [_t('S-one-key', one_key(S_CAP), S_CAP, expect={**_kern('S'), 'top_w': {'click_weighted': S_CAP * Q16}}),
            _t('M-one-key', one_key(M_CAP), M_CAP, expect={**_kern('M'), 'top_w': {'click_weighted': M_CAP * Q16}}),
            _t('L13x512-one-key', one_key(_PACKED_RUNS, L_CAP - _PACKED_RUNS), _PACKED_RUNS,
               expect={**_kern('L13x512'), 'top_w': {'click_weighted': _PACKED_RUNS * Q16}}),
            _t('Lwide-one-key', one_key(L_CAP), L_CAP, expect={**_kern('Lwide'), 'top_w': {'click_weighted': L_CAP * Q16}}),
            _t('L14-one-key', one_key(_PACKED_RUNS, 2 * L_CAP - _PACKED_RUNS), _PACKED_RUNS,
               expect={**_kern('L14'), 'top_w': {'click_weighted': _PACKED_RUNS * Q16}})]
    return tuple(out)


def _dense_targets(kernel):
    g = KERNELS[kernel]
    lo = {'M': S_CAP + 1, 'L13x512': M_CAP + 1, 'L14': L_CAP + 1, 'Lwide': PACKED_MAX_RUNS}[kernel]   # fewest records of the kernel's aids
    ds = [g['rcap'], g['ocap'], g['ocap'] + 1, g['cap']]
    if kernel == 'Lwide':
        ds = [g['rcap'], g['ocap']]                    # OCAP = the cap: OCAP + 1 keys need a larger l_cap (case wide-lcap8000)
    out = []
    for d in ds:
        n = max(d, lo + 40)
        counts = dense_counts(d, n, seed=d)
        n = int(counts.sum())
        runs = n if kernel in ('M', 'Lwide') else min(n, _PACKED_RUNS)
        out.append(_t(f'{kernel}-d{d}', counts, runs, expect={**_kern(kernel), 'heavy': 37, 'dense': dense_certain(kernel, d)}))
    return tuple(out)


# (light keys, runs: 'n' = one session per record, 'long' = sessions of 30, else fewer than 4096) that put ~h heavy keys
# among the light ones into each multi-wave instantiation
_MULTI = {'M': (1000, 'long'), 'L13x512': (3100, 'long'), 'L14': (6200, 'long'), 'Lwide': (4200, 'n')}


def _runs_for(n, how):
    return n if how == 'n' else long_runs(n)


def _heavy_first_targets(k):
    out = []
    for kernel, (light, how) in _MULTI.items():
        for h in (k - 1, k, k + 1):
            counts = heavy_and_light(h, light, seed=100 * k + h)
            out.append(_t(f'{kernel}-heavy{h}', counts, _runs_for(int(counts.sum()), how), expect={**_kern(kernel), 'heavy': h}))
    return tuple(out)


def _tie_targets():
    out = [_t('S-384-single-clicks', singles(S_CAP), S_CAP, expect={**_kern('S'), 'heavy': 0, 'ge_kth': {20: S_CAP}}),
           # 257 keys of one cart record outrank 43 keys of one click record in every type-weighted kind
           # (first partner = smallest id: a cart key in the last slot, behind the 256 candidates that fit the list)
           _t('S-257-of-300-tie', np.r_[singles(1, 1), _shuffled(np.r_[singles(CCAP, 1), singles(43)], 7)], 300,
              partner_ids=ids_without_collisions(300, 30000),
              expect={**_kern('S'), 'heavy': CCAP + 1, 'ge_kth': {20: CCAP + 1}})]
    for kernel, (light, how) in _MULTI.items():
        counts = tie_counts(100, 10, light, seed=light)
        out.append(_t(f'{kernel}-110-over-threshold', counts, _runs_for(int(counts.sum()), how),
                      expect={**_kern(kernel), 'heavy': 110, 'ge_kth': {20: 110}}))
    # many more tied keys than EXCAP behind every lane's best: the candidate lists of the two-pass path overflow
    for kernel, two, light, how in (('M', 1400, 200, 'long'), ('L13x512', 1500, 500, 'long')):
        counts = tie_counts(two, 10, light, seed=two)
        out.append(_t(f'{kernel}-{two + 10}-over-threshold', counts, _runs_for(int(counts.sum()), how),
                      expect={**_kern(kernel), 'heavy': two + 10, 'ge_kth': {20: two + 10}}))
    return tuple(out)


_DOMINANT_N, _DOMINANT_KEY = 13000, 12000


def _partition_targets():
    few = few_keys(25, 15000, seed=25)
    dom = np.r_[[[_DOMINANT_KEY, 0, 0]], mixed(_DOMINANT_N - _DOMINANT_KEY, seed=13)]
    return (_t('packed-25-keys', few, _PACKED_RUNS, expect=_kern('L13x512', 4)),
            _t('wide-25-keys', few, 5000, expect=_kern('Lwide', 4)),
            _t('wide-dominant-key', dom, _DOMINANT_N, expect=_kern('Lwide', 4)))


# the dominant key's 12,000 equal records share ONE partition; sized buckets hold bucket_cap(13000, 2) = 6756
assert bucket_cap(_DOMINANT_N, log2_parts(_DOMINANT_N, _DOMINANT_N)) < _DOMINANT_KEY
_PART_OPTIONS = tuple({'guess': g, 'part_sized': p} for g in (1, 0) for p in (1, 0))


def _k_sweep_targets():
    return (_t('S-200-keys', mixed(300, seed=1), 300, expect=_kern('S')),
            _t('S-10-keys', few_keys(10, 200, seed=2), 60, expect=_kern('S')),
            _t('M-many-keys', mixed(1500, seed=3), long_runs(1500), expect=_kern('M')),
            _t('M-15-keys', few_keys(15, 1500, seed=4), 400, expect=_kern('M')),
            _t('L-partitioned-many-keys', mixed(15000, seed=5), 3000, expect=_kern('L13x512', 4)),
            _t('L-partitioned-25-keys', few_keys(25, 15000, seed=6), _PACKED_RUNS, expect=_kern('L13x512', 4)))


_TIME_TOP = 4 * Q16          # 65536 + the largest extra (3 * 65536) per record

CASES = (
    Case('bin-edges-runs-n', _bin_edge_targets(False), option_sets=_PH),
    Case('bin-edges-packed', _bin_edge_targets(True), option_sets=_PH),
    # the partners of the one-key targets have that key's records themselves (aids of one key with a full counter, too)
    Case('table-load', _table_load_targets(), option_sets=({}, {'packed_heavy': 0}), other_max=2 * L_CAP),
    # unpartitioned wide items past the dense list: 7000 keys fill 85 % of the 2^13 slots; 6145 = OCAP + 1 of that kernel
    Case('wide-lcap8000', (_t('Lwide-7000-keys', singles(7000), 7000, expect={**_kern('Lwide'), 'heavy': 0, 'dense': False}),
                           _t('Lwide-d6145', dense_counts(6145, 6145, seed=6145), 6145,
                              expect={**_kern('Lwide'), 'heavy': 37, 'dense': False})),
         option_sets=({'l_cap': 8000},)),
    Case('dense-M', _dense_targets('M')),
    Case('dense-L13x512', _dense_targets('L13x512')),
    Case('dense-L14', _dense_targets('L14')),
    Case('dense-Lwide', _dense_targets('Lwide')),
    Case('heavy-first-k20', _heavy_first_targets(20), option_sets=({'hot': 2}, {'hot': 1}, {'hot': 0})),
    Case('heavy-first-k32', _heavy_first_targets(32), option_sets=({'hot': 2}, {'hot': 1}, {'hot': 0}), ks=(32,)),
    Case('ties', _tie_targets(), option_sets=({}, {'hot': 1})),
    Case('ties-same-ts', _tie_targets(), same_ts=True),
    # the partners of the 25-key targets are M aids themselves (600 runs of three or four partners each)
    Case('partitions', _partition_targets(), option_sets=_PART_OPTIONS, other_max=_DOMINANT_KEY,
         min_retries={i: 1 for i, o in enumerate(_PART_OPTIONS) if o['part_sized']}),
    # every record of the two targets carries the largest time extra: the packed sums reach 4095 * 2^18 and 3072 * 2^18
    Case('time-sum-bound', (_t('anchor', mixed(300, seed=9), 300),
                            _t('L-packed-4095-runs', one_key(_PACKED_RUNS), _PACKED_RUNS, at_ts_max=True,
                               expect={**_kern('L13x512'), 'top_w': {'time_weighted': _PACKED_RUNS * _TIME_TOP}}),
                            _t('M-3072-records', one_key(M_CAP), M_CAP, at_ts_max=True,
                               expect={**_kern('M'), 'top_w': {'time_weighted': M_CAP * _TIME_TOP}})),
         other_max=_PACKED_RUNS),
    Case('k-sweep', _k_sweep_targets(), ks=(1, 20, 32), other_max=M_CAP),
)
assert _PACKED_RUNS * _TIME_TOP < 2 ** 30
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

_streams = {}


def case_stream(case):
    """(Events, {target name: (aid, partner ids)}) of a case, built once."""
    if case.name not in _streams:
        _streams[case.name] = spoke_stream(case.targets, same_ts=case.same_ts)
    return _streams[case.name]
