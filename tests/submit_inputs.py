"""Inputs of the SPEC-SUBMIT and most-frequent-aid tests, shared by test_submit_cpu.py and test_submit_gpu.py (built once
per process). A submit case is a dict: session_id int32 [S], tables [(top_aid int32 [S, ld], n int32 [S])], types, k, ld."""
import functools

import numpy as np

L = 32                     # OTTO_SUBMIT_LINES: lines per workgroup of the format kernel
SCAN_TILE = 4096           # lines per workgroup of the scan (csrc/scan.h)
# every digit count and its edges
VALUES = sorted({0, (1 << 31) - 1} | {10 ** e - 1 for e in range(1, 10)} | {10 ** e for e in range(1, 10)})
assert VALUES[:5] == [0, 9, 10, 99, 100] and VALUES[-3:] == [10 ** 9 - 1, 10 ** 9, (1 << 31) - 1]


def _case(session_id, tables, types, k):
    session_id = np.asarray(session_id, dtype=np.int32)
    tables = [(np.ascontiguousarray(t, dtype=np.int32), np.asarray(n, dtype=np.int32)) for t, n in tables]
    ld = tables[0][0].shape[1]
    assert all(t.shape == (len(session_id), ld) and n.shape == (len(session_id),) for t, n in tables) and ld >= k
    return dict(session_id=session_id, tables=tables, types=list(types), k=k, ld=ld)


def _random_aids(rng, shape):
    """aids of every digit count: 10^u, u uniform in [0, 9.33)"""
    return np.minimum(np.floor(10.0 ** rng.uniform(0.0, 9.332, shape)) - (rng.random(shape) < 0.1), (1 << 31) - 1).clip(0).astype(np.int64)


def _shape_case(seed, S, T, k, ld, n_choices):
    rng = np.random.default_rng(seed)
    session = _random_aids(rng, S)
    tables = []
    for t in range(T):
        n = np.array([n_choices[(s + t) % len(n_choices)] for s in range(S)], dtype=np.int32)
        top = _random_aids(rng, (S, ld))
        for s in range(S):
            top[s, max(int(n[s]), 0):] = -1                  # the padding is never read as a value
        tables.append((top, n))
    return _case(session, tables, [(2 - t) % 3 for t in range(T)] if T == 3 else [seed % 3], k)


def _digits_case():
    """Every value of VALUES as the session and as the first, a middle and the last aid of a line, for all three suffixes."""
    V = VALUES
    top = np.array([[V[i], V[(i + 1) % len(V)], V[i], V[(i + 2) % len(V)], V[i]] for i in range(len(V))])
    n = np.full(len(V), 5)
    return _case(V, [(top, n)] * 3, [0, 1, 2], 5)


def _lone_case():
    """Mostly skipped sessions, lone 9-byte lines `0_carts,\\n`: workgroups 0, 1, 2 and 4 own 9 bytes each, workgroup 3
    owns nothing, so at some alignments three workgroups meet inside one 16-byte word."""
    S = 5 * L + 3
    n = np.full(S, -1)
    for s in (L - 1, L + 7, 2 * L, 4 * L + 1, 5 * L + 2):
        n[s] = 0
    return _case(np.zeros(S), [(np.full((S, 1), -1), n)], [1], 1)


def lone_case_meetings(first_byte):
    """per 16-byte word of the output, the workgroups that own bytes of it (the lone case at ``first_byte``)"""
    c = case('lone9')
    owners = {}
    at = first_byte
    for s, n in enumerate(c['tables'][0][1]):
        if n >= 0:
            for b in range(at, at + 9):
                owners.setdefault(b // 16, set()).add(s // L)
            at += 9
    return owners


@functools.lru_cache(maxsize=None)
def _specs():
    s = {'digits': _digits_case, 'lone9': _lone_case}
    for k in (1, 20, 64):
        for pad in (0, 3):
            for T in (1, 3):
                # n in {0, 1, k - 1, k} and -1 (no line); 2 L + 5 sessions: more than one workgroup, a ragged last one
                s[f'shape-k{k}-ld{k + pad}-T{T}'] = functools.partial(_shape_case, 100 + 10 * k + pad + T, 2 * L + 5, T, k, k + pad,
                                                                     (0, 1, k - 1, k, -1, k))
    for S in (L - 1, L, L + 1, 2 * L + 1):
        s[f'tile-S{S}'] = functools.partial(_shape_case, 200 + S, S, 1, 20, 20, (20, 19, 0, 20, 3))
    for S in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        s[f'scan-S{S}'] = functools.partial(_shape_case, 300 + S, S, 1, 2, 2, (2, 1, 0, -1, 2))
    s['all-skipped'] = functools.partial(_shape_case, 400, L + 1, 3, 4, 4, (-1,))
    s['no-sessions'] = functools.partial(_shape_case, 401, 0, 3, 20, 20, (20,))
    return s


CASE_NAMES = tuple(_specs())
_built = {}


def case(name):
    if name not in _built:
        _built[name] = _specs()[name]()
    return _built[name]


assert max(len(v) for v in lone_case_meetings(9).values()) >= 3, 'three workgroups in one 16-byte word'


# ---- most frequent aids: name -> (aid uint32 [E], type uint8 [E], n_aids, k, distinct) ------------------------------------
def _freq_random(seed, n_aids, E, k, types=(0, 0, 0, 1, 1, 2), distinct=False):
    rng = np.random.default_rng(seed)
    aid = np.minimum(rng.zipf(1.3, E) - 1, n_aids - 1).astype(np.uint32) if not distinct else None
    if distinct:
        # aid a of the head occurs (H - a) * 3 + type-dependent extra times: the first k + 1 counts of every list differ
        H = min(n_aids, k + 6)
        parts_a, parts_t = [], []
        for a in range(H):
            for t, mult in ((0, 5), (1, 3), (2, 2)):
                reps = (H - a) * mult + (a * (t + 1)) % mult
                parts_a.append(np.full(reps, (a * 7919) % n_aids if n_aids > 7919 else a))
                parts_t.append(np.full(reps, t))
        aid, typ = np.concatenate(parts_a).astype(np.uint32), np.concatenate(parts_t).astype(np.uint8)
        p = rng.permutation(len(aid))
        return aid[p], typ[p], n_aids, k, True
    typ = rng.choice(np.array(types, dtype=np.uint8), E)
    return aid, typ, n_aids, k, False


def _freq_ties():
    """Every aid of [0, 1300) twice as a click, aids 250..262 and 1020..1030 once more: ties across the 64-aid lists, the
    256-aid workgroups and the merge; carts on aids 300 and 5 only, no orders."""
    aid = np.r_[np.repeat(np.arange(1300), 2), np.arange(250, 263), np.arange(1020, 1031), [300, 300, 5, 5]]
    typ = np.r_[np.zeros(2600 + 13 + 11), np.ones(4)]
    p = np.random.default_rng(5).permutation(len(aid))
    return aid[p].astype(np.uint32), typ[p].astype(np.uint8), 1300, 20, False


@functools.lru_cache(maxsize=None)
def freq_cases():
    c = {}
    for n_aids in (1, 63, 64, 65, (1 << 16) + 1):
        c[f'n_aids-{n_aids}'] = _freq_random(n_aids, n_aids, 3000, 20)
    c['distinct-40'] = _freq_random(1, 40, 0, 20, distinct=True)
    c['distinct-65537-k64'] = _freq_random(2, (1 << 16) + 1, 0, 64, distinct=True)
    c['distinct-few'] = _freq_random(3, 9, 0, 20, distinct=True)            # fewer aids than k
    c['no-events'] = (np.zeros(0, np.uint32), np.zeros(0, np.uint8), 100, 20, False)
    c['no-orders'] = _freq_random(4, 500, 2000, 20, types=(0, 0, 1))
    c['one-aid'] = (np.full(50000, 77, np.uint32), np.random.default_rng(6).integers(0, 3, 50000).astype(np.uint8), 100, 20, False)
    c['ties'] = _freq_ties()
    return c


def _assert_distinct():
    from submit_restatement import frequency_counts
    for name, (aid, typ, n_aids, k, distinct) in freq_cases().items():
        if distinct:
            cnt = frequency_counts(aid, typ, n_aids)
            for row in [cnt.sum(axis=0)] + list(cnt):
                head = np.sort(row[row > 0])[::-1][:k + 1]
                assert len(set(head.tolist())) == len(head), (name, head)


_assert_distinct()
