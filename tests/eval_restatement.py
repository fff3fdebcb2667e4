"""SPEC-EVAL (include/otto_eval.h) restated in NumPy and plain Python, one session at a time, with no cleverness: what the
device code is compared against. Nothing here imports the package under test."""
import numpy as np

MASK = (1 << 64) - 1
DENOM_CAP = 20


class Refused(ValueError):
    """What the library answers with OTTO_EINVAL."""


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def check_types(typ):
    if np.any(np.asarray(typ) > 2):
        raise Refused('typ outside 0..2')


def last_click(typ, sess_off):
    check_types(typ)
    out = np.full(len(sess_off) - 1, -1, dtype=np.int32)
    for s in range(len(sess_off) - 1):
        t = typ[sess_off[s]:sess_off[s + 1]]
        for i in range(len(t)):
            if t[i] == 0:
                out[s] = i
    return out


def cutoffs(typ, sess_off, seed):
    """(cutoff int32 [S], number of sessions without a click and with n != 2)."""
    last = last_click(typ, sess_off)
    out = np.zeros(len(last), dtype=np.int32)
    without = 0
    for s in range(len(last)):
        n = int(sess_off[s + 1] - sess_off[s])
        if n != 2 and last[s] < 0:
            without += 1
        if n == 2 or last[s] <= 0:
            continue
        h = mix64(mix64(seed & MASK) ^ ((s * 0xA0761D6478BD642F) & MASK))
        out[s] = ((h >> 32) * int(last[s])) >> 32
    return out, without


def labels_after(aids, types, cutoff):
    """(click list of 0 or 1 aids, carts ascending distinct, orders ascending distinct) over the events after cutoff."""
    click, carts, orders = [], set(), set()
    for i in range(cutoff + 1, len(aids)):
        if types[i] == 0 and not click:
            click.append(int(aids[i]))
        elif types[i] == 1:
            carts.add(int(aids[i]))
        elif types[i] == 2:
            orders.add(int(aids[i]))
    return click, sorted(carts), sorted(orders)


def split(aid, ts, typ, sess_off, cutoff):
    """{'aid', 'ts', 'typ', 'sess_off'} of the kept events and {'clicks': (off, aid), 'carts': ..., 'orders': ...}."""
    check_types(typ)
    S = len(sess_off) - 1
    for s in range(S):
        n = int(sess_off[s + 1] - sess_off[s])
        if not 0 <= int(cutoff[s]) < max(n, 1):
            raise Refused(f'cutoff of session {s}')
    keep = []
    k_off = [0]
    lists = ([], [], [])
    offs = ([0], [0], [0])
    for s in range(S):
        b, e = int(sess_off[s]), int(sess_off[s + 1])
        if e > b:
            keep.extend(range(b, b + int(cutoff[s]) + 1))
        k_off.append(len(keep))
        for lst, off, got in zip(lists, offs, labels_after(aid[b:e], typ[b:e], int(cutoff[s]))):
            lst.extend(got)
            off.append(len(lst))
    keep = np.asarray(keep, dtype=np.int64)
    kept = {'aid': np.asarray(aid)[keep], 'ts': np.asarray(ts)[keep], 'typ': np.asarray(typ)[keep],
            'sess_off': np.asarray(k_off, dtype=np.int64)}
    labels = {name: (np.asarray(off, dtype=np.int64), np.asarray(lst, dtype=np.int32))
              for name, off, lst in zip(('clicks', 'carts', 'orders'), offs, lists)}
    return kept, labels


def rows_padded(pred, n=None):
    return [[int(v) for v in (row if n is None else row[:max(int(n[p]), 0)])] for p, row in enumerate(np.asarray(pred))]


def rows_csr(off, aid):
    return [[int(v) for v in aid[off[p]:off[p + 1]]] for p in range(len(off) - 1)]


def lists_csr(off, aid):
    return rows_csr(off, aid)


def hits(labels, rows, label_session=None, pred_session=None, cap=20):
    """labels: list of label lists per label session; rows: list of prediction rows. (hits int32 [S], denom int32 [S])."""
    S = len(labels)
    ids = list(range(S)) if label_session is None else [int(v) for v in label_session]
    if pred_session is None:
        if len(rows) != S:
            raise Refused('position-aligned rows need P == S')
        row_of = {ids[j]: rows[j] for j in range(S)}
    else:
        row_of = {}
        for p, v in enumerate(pred_session):
            if int(v) not in ids:
                raise Refused(f'prediction session {int(v)} is no label session')
            row_of[int(v)] = rows[p]
    out_h = np.zeros(S, dtype=np.int32)
    out_d = np.zeros(S, dtype=np.int32)
    for j in range(S):
        row = row_of.get(ids[j], [])
        if cap and cap > 0:
            row = row[:cap]
        counted = set(v for v in row if v >= 0)
        out_h[j] = len(counted & set(int(v) for v in labels[j]))
        out_d[j] = min(len(labels[j]), DENOM_CAP)
    return out_h, out_d


def totals(h, d, mask=None):
    m = np.zeros(len(h), dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    return {'hits': int(h.sum()), 'denom': int(d.sum()), 'mask_hits': int(h[m].sum()), 'mask_denom': int(d[m].sum())}
