"""SPEC-SUBMIT (include/otto_submit.h) and the most-frequent-aid lists restated in plain Python / NumPy, written from the
specification: what the device kernels must reproduce byte for byte."""
import json

import numpy as np

SUFFIX = ('_clicks', '_carts', '_orders')
HEADER = b'session_type,labels\n'
ROWS = ('all', 'click', 'cart', 'order')


def line_order(S, T, interleave):
    """(s, t) of every line index in order"""
    if interleave:
        return [(s, t) for s in range(S) for t in range(T)]
    return [(s, t) for t in range(T) for s in range(S)]


def line_bytes(session, code, aids):
    return (str(int(session)) + SUFFIX[code] + ',' + ' '.join(str(int(a)) for a in aids) + '\n').encode()


def violation(session, row, n, k):
    """True when the line (n >= 0) breaks SPEC-SUBMIT"""
    return n > k or session < 0 or any(int(a) < 0 for a in row[:n])


def first_violation(session_id, tables, k, interleave=False):
    """The smallest violating line index, None without one. tables: [(top_aid [S, ld >= k], n [S])]."""
    S, T = len(session_id), len(tables)
    for i, (s, t) in enumerate(line_order(S, T, interleave)):
        top, n = tables[t]
        if n[s] >= 0 and violation(int(session_id[s]), top[s], int(n[s]), k):
            return i
    return None


def submission_lines(session_id, tables, types, interleave=False):
    """One bytes object per line index (b'' for a session with n < 0)."""
    S, T = len(session_id), len(tables)
    out = []
    for s, t in line_order(S, T, interleave):
        top, n = tables[t][0], tables[t][1]
        out.append(b'' if n[s] < 0 else line_bytes(session_id[s], types[t], top[s, :n[s]]))
    return out


def submission_bytes(session_id, tables, types, interleave=False, header=False):
    return (HEADER if header else b'') + b''.join(submission_lines(session_id, tables, types, interleave))


def frequency_counts(aid, typ, n_aids):
    """int64 [3, n_aids]"""
    c = np.zeros((3, n_aids), dtype=np.int64)
    np.add.at(c, (np.asarray(typ, dtype=np.int64), np.asarray(aid, dtype=np.int64)), 1)
    return c


def frequency_lists(counts, k):
    """{'all' | 'click' | 'cart' | 'order': (aids, counts)}: by (count descending, aid ascending), zero counts left out"""
    rows = [counts.sum(axis=0)] + [counts[t] for t in range(3)]
    out = {}
    for name, c in zip(ROWS, rows):
        order = sorted((a for a in range(len(c)) if c[a] > 0), key=lambda a: (-int(c[a]), a))[:k]
        out[name] = (np.array(order, dtype=np.int32), np.array([c[a] for a in order], dtype=np.int64))
    return out


def frequency_json(aids, counts):
    """The reference's file: a JSON object aid -> count in list order, two spaces of indent, no trailing newline."""
    if len(aids) == 0:
        return b'{}'
    return ('{\n' + ',\n'.join(f'  "{int(a)}": {int(c)}' for a, c in zip(aids, counts)) + '\n}').encode()


assert frequency_json([3, 1], [7, 2]) == json.dumps({'3': 7, '1': 2}, indent=2).encode()
