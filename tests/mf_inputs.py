"""Input builders of the MF edge tests (tests/test_mf_edges_gpu.py). Plain NumPy and the CPU oracle; nothing here touches a
device. ``tests/test_mf_inputs_cpu.py`` asserts every property a GPU test relies on, so that a degenerate input fails on the
CPU before it can hide anything on the GPU.

Kernel geometry restated here (csrc/otto_mf.hip), so that the inputs can be aimed at it:
    a lane group of G = d / 4 lanes owns one sample; a 256-thread block holds gpb = 256 / G = 1024 / d groups;
    every step / eval / BPR kernel loops ``for (b = block * gpb + group; b < B; b += grid * gpb)`` with
    grid = min(ceil(B / gpb), MF_GRID_MAX = 2048); a wave holds 64 / G groups (64 at d = 4, one at d = 256).
"""
import functools
from types import SimpleNamespace

import numpy as np

import mf_oracle as mo
from edge_inputs import dot_bound

F = np.float32
D_ALL = (4, 8, 16, 32, 64, 128, 256)
D_EDGE = (4, 32, 256)
KINDS = ('MSELoss', 'BCEWithLogitsLoss')          # position = OTTO_MF_LOSS_MSE / OTTO_MF_LOSS_BCE
DUPS = ('none', 'pairs', 'one_row', 'zipf', 'self')
MF_GRID_MAX = 2048
LR = 0.05
ZIPF_N1, ZIPF_N2 = 97, 53
NEAR_CANCELLED = 1e-3       # a coalesced gradient row below this fraction of the median row norm is redrawn
LOSS_CONDITION = 1e-5       # a tenth of the 1e-4 band: largest shift a float32 forward may cause in a loss or a sum
SIGMOID_HALF = 2.0 ** -22   # below zero by less than this, float32 1 / (1 + exp(-x)) may still round to 0.5


def gpb(d):
    return 1024 // d


def mf_grid(n, d):
    """``mf_grid`` of the .hip: blocks launched for n lane groups' worth of work."""
    return max(1, min(MF_GRID_MAX, -(-n // gpb(d))))


def trips(B, d):
    """Loop trips of every (block, group) of a kernel launched over B samples: int64 [grid, gpb]."""
    grid, g = mf_grid(B, d), gpb(d)
    b0 = np.arange(grid, dtype=np.int64)[:, None] * g + np.arange(g, dtype=np.int64)[None, :]
    return np.maximum(0, -(-(B - b0) // (grid * g)))


def two_trip(d):
    """The smallest batch with a second, partly filled trip (one sample in it); None where that exceeds 32769 rows."""
    return MF_GRID_MAX * gpb(d) + 1 if d >= 64 else None


def batch_sizes(d):
    g = gpb(d)
    sizes = [1] + ([g - 1] if g - 1 > 0 else []) + [g, g + 1, 3 * g + 2]
    if two_trip(d):
        sizes.append(two_trip(d))
    return sizes


def _zipf(rng, a, B, n):
    return np.minimum(rng.zipf(a, B) - 1, n - 1)


def draw_ids(B, dup, shared, rng):
    """(n1, n2, i1, i2) of one duplicate structure; n1 and n2 depend on (B, dup, shared) only. A shared table has n2 = n1."""
    if dup == 'none':                              # all ids distinct across both columns
        n1 = 2 * B + 3 if shared else B + 5
        n2 = n1 if shared else B + 3
        if shared:
            p = rng.permutation(n1)
            i1, i2 = p[:B], p[B:2 * B]
        else:
            i1, i2 = rng.permutation(n1)[:B], rng.permutation(n2)[:B]
    elif dup == 'pairs':
        # every row occurs exactly twice, so each has exactly one second arriver. A column of odd length cannot hold
        # that: then one row of the column occurs three times (still one second arriver)
        if shared:
            n1 = n2 = B + 4
            p = rng.permutation(np.repeat(rng.permutation(n1)[:B], 2))
            i1, i2 = p[:B], p[B:]
        else:
            if B < 2:
                raise ValueError("'pairs' needs B >= 2 per column")
            n1, n2 = B // 2 + 4, B // 2 + 2

            def col(n):
                rows = rng.permutation(n)[:B // 2]
                return rng.permutation(np.r_[np.repeat(rows, 2), rows[:B % 2]])
            i1, i2 = col(n1), col(n2)
    elif dup == 'one_row':
        n1, n2 = (7, 7) if shared else (7, 5)
        i1, i2 = np.full(B, 3), np.full(B, 1)
    elif dup == 'zipf':
        n1, n2 = (ZIPF_N1, ZIPF_N1) if shared else (ZIPF_N1, ZIPF_N2)
        i1 = rng.permutation(n1)[_zipf(rng, 1.2, B, n1)]       # skewed in both columns, heavy rows unrelated
        i2 = _zipf(rng, 1.3, B, n2)                            # one row holds a large share of the batch
    elif dup == 'self':
        if not shared:
            raise ValueError("'self' needs a shared table")
        n1 = n2 = ZIPF_N1
        i1 = rng.permutation(n1 - 1)[_zipf(rng, 1.2, B, n1 - 1)]
        i2 = _zipf(rng, 1.3, B, n1 - 1)
        at = rng.permutation(B)[:min(B, 8)]
        i2[at] = i1[at]                            # the sample is its own second arriver
        i1[at[0]] = i2[at[0]] = n1 - 1             # ... and this one's row occurs nowhere else
    else:
        raise ValueError(dup)
    return n1, n2, np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64)


def tables(n1, n2, d, shared, rng):
    E1 = (rng.standard_normal((n1, d)) * 0.3).astype(F)
    E2 = E1 if shared else (rng.standard_normal((n2, d)) * 0.3).astype(F)
    return E1, E2


def draw_targets(B, kind, rng):
    return rng.integers(0, 3 if kind == 'MSELoss' else 2, B).astype(np.int64)


def coalesced_row_norms(E1, E2, i1, i2, target, kind, shared):
    """Per table (norms of the coalesced gradient rows, sums of the norms of the occurrences that make each row up, the
    rows' ids), by ``mo.sparse_adam_step``'s own arithmetic. Only rows of the batch are listed."""
    out = mo.forward(E1, E2, i1, i2)
    _, g = mo.loss_and_grad(kind, out, target)
    c = (g / len(i1))[:, None]
    g1, g2 = c * E2[i2].astype(np.float64), c * E1[i1].astype(np.float64)
    d = E1.shape[1]

    def table(n, idx, rows):
        touched, gr = mo._coalesced(n, d, idx, rows)
        parts = np.zeros(n)
        np.add.at(parts, idx, np.linalg.norm(rows, axis=1))
        return np.linalg.norm(gr.astype(np.float64), axis=1), parts[touched], touched
    if shared:
        return [table(E1.shape[0], np.concatenate([i1, i2]), np.concatenate([g1, g2]))]
    return [table(E1.shape[0], i1, g1), table(E2.shape[0], i2, g2)]


def smallest_row_ratio(E1, E2, i1, i2, target, kind, shared):
    """The smaller of: the smallest coalesced gradient row norm over the median row norm of its table; the smallest row
    norm over the summed norms of the row's own occurrences (what the sum kept of what went into it). Near-cancelled rows
    are where Adam's m / (sqrt(v) + eps) amplifies summation order. The second ratio also sees a table of one row."""
    return min(float(r.min()) for r, _ in _row_ratios(E1, E2, i1, i2, target, kind, shared))


def _row_ratios(E1, E2, i1, i2, target, kind, shared):
    return [(np.minimum(nr / np.median(nr), nr / parts), rows)
            for nr, parts, rows in coalesced_row_norms(E1, E2, i1, i2, target, kind, shared)]


def loss_condition(E1, E2, i1, i2, target, kind):
    """Largest relative shift of the batch loss and of the validation sums when the forward is rounded to float32 (the
    oracle's float32 forward against float64 dot products). A loss that cancels (one MSE sample whose output meets its
    target) cannot be compared at 1e-4 relative, whatever computes it; the builders redraw such targets, so a B = 1 MSE
    batch whose loss nearly cancels is never exercised."""
    o32 = mo.forward(E1, E2, i1, i2).astype(np.float64)
    o64 = (E1[i1].astype(np.float64) * E2[i2].astype(np.float64)).sum(axis=-1)
    t = np.asarray(target).astype(np.float64)
    worst = 0.0
    for a, b in zip(_sums(o32, t, kind), _sums(o64, t, kind)):
        worst = max(worst, abs(a - b) / abs(b) if b else np.inf)
    return worst


def _sums(out, t, kind):
    l, _ = mo.loss_and_grad(kind, out, t)
    p = out if kind == 'MSELoss' else 1.0 / (1.0 + np.exp(-out))
    return l.sum(), np.abs(p - t).sum(), ((p - t) ** 2).sum()


def _step_targets(E1, E2, i1, i2, kind, shared, rng, tries=200):
    """Targets of a step. The samples of a near-cancelled gradient row get new targets until no such row is left; a badly
    conditioned loss redraws them all."""
    tg = draw_targets(len(i1), kind, rng)
    for _ in range(tries):
        bad = np.zeros(len(i1), dtype=bool)
        for k, (r, rows) in enumerate(_row_ratios(E1, E2, i1, i2, tg, kind, shared)):
            low = rows[r < NEAR_CANCELLED]
            bad |= (np.isin(i1, low) | np.isin(i2, low)) if shared else np.isin(i2 if k else i1, low)
        if bad.any():
            tg[bad] = draw_targets(int(bad.sum()), kind, rng)
        elif loss_condition(E1, E2, i1, i2, tg, kind) > LOSS_CONDITION:
            tg = draw_targets(len(i1), kind, rng)
        else:
            return tg
    raise AssertionError('no well-conditioned targets found')


def step_case(d, B, dup, shared, rng, kind='MSELoss'):
    """(n1, n2, E1, E2, i1, i2, target) of one first step: tables about 0.3 N(0, 1), targets in {0, 1, 2} (MSE) or {0, 1}
    (BCE), redrawn until no coalesced gradient row is near-cancelled and the loss is well conditioned."""
    n1, n2, i1, i2 = draw_ids(B, dup, shared, rng)
    E1, E2 = tables(n1, n2, d, shared, rng)
    return n1, n2, E1, E2, i1, i2, _step_targets(E1, E2, i1, i2, kind, shared, rng)


@functools.lru_cache(maxsize=None)
def step_sequence(d, kind, shared, plan, seed=0):
    """Consecutive steps t = 1, 2, ... on one pair of tables with the oracle's state after each. ``plan`` is a tuple of
    (B, dup); all of its entries must agree on the table sizes. Every step's targets are drawn against the oracle's tables
    before that step (the guards of ``step_case`` hold at every step, and the loss of an ``eval`` of the same ids after
    the step is well conditioned too). Returns a namespace: n1, n2, E1, E2 (initial; E2 is E1 when shared), steps
    [(i1, i2, target)], before [(E1, E2)], want [(loss, E1, m1, v1, E2, m2, v2)]. Treat it as read-only."""
    rng = np.random.default_rng([seed, d, KINDS.index(kind), int(shared), sum(map(ord, plan[0][1])), plan[0][0], len(plan)])
    n1, n2, E1, E2, i1, i2, first = step_case(d, plan[0][0], plan[0][1], shared, rng, kind)      # step 1 is a step_case
    s = SimpleNamespace(d=d, kind=kind, shared=shared, n1=n1, n2=n2, E1=E1.copy(), steps=[], before=[], want=[])
    s.E2 = s.E1 if shared else E2.copy()
    m1, v1 = np.zeros_like(E1), np.zeros_like(E1)
    m2, v2 = (m1, v1) if shared else (np.zeros_like(E2), np.zeros_like(E2))
    for k, (B, dup) in enumerate(plan):
        if k:
            na, nb, i1, i2 = draw_ids(B, dup, shared, rng)
            assert (na, nb) == (n1, n2), 'the steps of a sequence share their tables'
        for _ in range(50):
            tg, first = (first, None) if first is not None else (_step_targets(E1, E2, i1, i2, kind, shared, rng), None)
            st = [x.copy() for x in (E1, m1, v1)] + ([] if shared else [x.copy() for x in (E2, m2, v2)])
            st = st + st if shared else st
            loss, _ = mo.sparse_adam_step(*st, i1, i2, tg, kind, LR, step=k + 1, shared=shared)
            if loss_condition(st[0], st[3], i1, i2, tg, kind) <= LOSS_CONDITION:
                break
        else:
            raise AssertionError('no well-conditioned targets found')
        s.before.append((E1, E2))
        s.steps.append((i1, i2, tg))
        s.want.append((loss,) + tuple(st))
        E1, m1, v1, E2, m2, v2 = st
    return s


# ---------------------------------------------------------------------------------------------------------------------
# validation sums
# ---------------------------------------------------------------------------------------------------------------------
def threshold_margin(E1, E2, i1, i2, kind):
    """(distance of every sample's float64 output from the hit threshold, band): the threshold is out = 0.5 for MSE
    (p = out) and out = 0 for BCE (p = sigmoid(out)); the band is the float32 dot-product bound of ``edge_inputs.dot_bound``,
    for BCE plus the distance below zero at which a float32 sigmoid still rounds to 0.5."""
    S, bound = dot_bound(E1, E2)
    out, band = S[i1, i2], bound[i1, i2]
    if kind == 'MSELoss':
        return np.abs(out - 0.5), band
    return np.abs(out), band + SIGMOID_HALF


def eval_ids(B, shared, rng):
    n1, n2 = (ZIPF_N1, ZIPF_N1) if shared else (ZIPF_N1, ZIPF_N2)
    return rng.integers(0, n1, B).astype(np.int64), _zipf(rng, 1.3, B, n2).astype(np.int64)


def eval_case(d, B, kind, rng, shared=False, given=None):
    """(n1, n2, E1, E2, i1, i2, target) of one validation batch (``given`` = (E1, E2) reuses a case's tables). Every
    sample's float64 output lies further from the hit threshold than the float32 dot-product bound: samples inside the band
    are redrawn, never skipped, so hits can be compared exactly. Targets are redrawn until the loss and the sums are well
    conditioned."""
    n1, n2 = (ZIPF_N1, ZIPF_N1) if shared else (ZIPF_N1, ZIPF_N2)
    E1, E2 = given if given is not None else tables(n1, n2, d, shared, rng)
    i1, i2 = eval_ids(B, shared, rng)
    for _ in range(200):
        dist, band = threshold_margin(E1, E2, i1, i2, kind)
        inside = np.flatnonzero(dist <= band)
        if not len(inside):
            break
        a, b = eval_ids(len(inside), shared, rng)
        i1[inside], i2[inside] = a, b
    else:
        raise AssertionError('samples stay inside the threshold band')
    for _ in range(200):
        tg = draw_targets(B, kind, rng)
        if loss_condition(E1, E2, i1, i2, tg, kind) <= LOSS_CONDITION:
            return n1, n2, E1, E2, i1, i2, tg
    raise AssertionError('no well-conditioned targets found')


def sums_batches(d):
    """Batch sizes of the three ``eval_sums`` launches of one engine."""
    return (1, gpb(d) + 1, two_trip(d) or 3 * gpb(d) + 2)


@functools.lru_cache(maxsize=None)
def sums_case(d, kind, shared):
    """Three validation batches on one pair of tables, plus a fourth for the plain ``eval`` in between: a namespace with
    n1, n2, E1, E2 and batches [(i1, i2, target)]."""
    rng = np.random.default_rng([11, d, KINDS.index(kind), int(shared)])
    s = SimpleNamespace(batches=[])
    given = None
    for B in sums_batches(d) + (gpb(d) + 1,):
        s.n1, s.n2, s.E1, s.E2, i1, i2, tg = eval_case(d, B, kind, rng, shared, given)
        given = (s.E1, s.E2)
        s.batches.append((i1, i2, tg))
    return s


# ---------------------------------------------------------------------------------------------------------------------
# BPR
# ---------------------------------------------------------------------------------------------------------------------
BPR_NU, BPR_NI = 211, 53
FALLBACK_ROWS = (6543, 13119, 18167)       # seed 1, epoch 0, n_items 2: all 16 draws are 1
# seed 1, epoch 0, n_items 3: (row, positive, negative): 15 draws hit the positive, the 16th is accepted and is NOT
# (pos + 1) % 3 -- a sampler that gives up one attempt early returns another item here
LAST_ATTEMPT = (573527, 1, 0)


def bpr_fallback_rows(seed, epoch, n_rows):
    """Global rows < n_rows whose 16 draws at n_items = 2 are all equal: [(row, value)]. A row whose positive is that value
    takes the sampler's fallback (pos + 1) % n_items."""
    found = []
    base0 = mo.mix64(seed ^ ((epoch * 0xD1342543DE82EF95) & mo.MASK))
    for row in range(n_rows):
        base = base0 ^ ((row * 0xA0761D6478BD642F) & mo.MASK)
        first = mo.mix64(base) >> 63
        if all(mo.mix64(base ^ ((att * 0xE7037ED1A0B428DB) & mo.MASK)) >> 63 == first for att in range(1, 16)):
            found.append((row, int(first)))
    return found


def bpr_case(d, B, rng):
    """(U, V, u, i) of one BPR batch: random users, zipf items."""
    U = (rng.standard_normal((BPR_NU, d)) * 0.2).astype(F)
    V = (rng.standard_normal((BPR_NI, d)) * 0.2).astype(F)
    return U, V, rng.integers(0, BPR_NU, B).astype(np.int64), _zipf(rng, 1.4, B, BPR_NI).astype(np.int64)


RACE_NU, RACE_NI = 1024, 50_000          # the item table is 51.2 MB at d = 256


def race_free_triplets(d, seed, rng):
    """(U, V, u, i, j): distinct users, distinct positives, and the longest prefix of the batch whose positives and sampled
    negatives (sampler ``seed``, epoch 0, row0 0) share no row: hogwild on it has no race and equals the sequential
    oracle. The item count makes the prefix longer than the 64 lane groups of a d = 4 wave."""
    u = rng.permutation(RACE_NU)[:512]           # the ids come first: the same triplets at every d
    i = rng.permutation(RACE_NI)[:512]
    U = (rng.standard_normal((RACE_NU, d)) * 0.2).astype(F)
    V = (rng.standard_normal((RACE_NI, d)) * 0.2).astype(F)
    j = mo.bpr_negatives(seed, 0, 0, i, RACE_NI)
    seen, keep = set(), 0
    for a, b in zip(i.tolist(), j.tolist()):
        if a in seen or b in seen:
            break
        seen.update((a, b))
        keep += 1
    return U, V, u[:keep].astype(np.int64), i[:keep].astype(np.int64), j[:keep]


def race_rng():
    return np.random.default_rng(10)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_mf_edges_gpu.py (shared with the CPU test, which checks every one of them)
# ---------------------------------------------------------------------------------------------------------------------
def matrix_plan(d, dup):
    g = gpb(d)
    return ((3 * g + 2, dup), (3 * g + 2, dup), (g + 1, dup))


MATRIX_CASES = [(d, kind, shared, dup) for d in D_ALL for kind in KINDS for shared in (False, True)
                for dup in (('zipf', 'self') if shared else ('zipf',))]
EDGE_CASES = [(d, B, 'zipf') for d in D_ALL for B in batch_sizes(d)] + [(d, two_trip(d), 'none') for d in D_ALL if two_trip(d)]
IDENTICAL_CASES = [(d, B) for d in D_ALL for B in (1, gpb(d) + 1, two_trip(d)) if B]
DUP_CASES = [(dup, d, shared) for dup in ('none', 'pairs', 'one_row') for d in D_EDGE for shared in (False, True)]
SUMS_CASES = [(d, kind, shared) for d in D_EDGE for kind in KINDS for shared in (False, True)]
BPR_BATCH_CASES = [(d, B) for d in D_ALL for B in (1, gpb(d) + 1, two_trip(d)) if B]


def matrix_seq(d, kind, shared, dup):
    return step_sequence(d, kind, shared, matrix_plan(d, dup), seed=1)


def edge_seq(d, B, dup):
    return step_sequence(d, 'MSELoss', False, ((B, dup),), seed=2)


def dup_seq(dup, d, shared):
    return step_sequence(d, 'MSELoss', shared, ((gpb(d) + 1, dup),) * 2, seed=3)
