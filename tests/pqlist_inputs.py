"""Input builders of the list-column and label tests (include/otto_pqlist.h, include/otto_labels.h): row mixes of null,
empty, one-element and long lists; the pyarrow writer settings that give every page shape SPEC-PQLIST accepts; a small V1
writer over ``parquet_write.thrift_bytes`` that cuts pages at arbitrary level positions (pyarrow never cuts inside a row)
and takes the edits of the refusal tests; label frames in the shape of ``val_labels.parquet``. Files are written at test
time; nothing is read from outside the test's own directory."""
import struct

import numpy as np

COLUMN = 'ground_truth'
TYPE_CODES = {'clicks': 0, 'carts': 1, 'orders': 2}


def rows(n=600, seed=0, longs=(1024, 2500), n_aids=50000):
    """``n`` rows: None, [], one element, short and long lists in a random mix, then stretches of equal rows (300
    one-element rows, 200 empties, 100 nulls: long RLE runs in both level streams) and the ``longs`` lists in between."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = rng.integers(0, 10)
        if k == 0:
            out.append(None)
        elif k == 1:
            out.append([])
        elif k < 5:
            out.append([int(rng.integers(0, n_aids))])
        elif k < 9:
            out.append(rng.integers(0, n_aids, size=rng.integers(2, 12)).tolist())
        else:
            out.append(rng.integers(0, n_aids, size=rng.integers(30, 300)).tolist())
    out[n // 3:n // 3] = [[int(v)] for v in rng.integers(0, n_aids, size=300)] + [[] for _ in range(200)] + [None] * 100
    for j, ln in enumerate(longs):
        out.insert((j + 1) * len(out) // (len(longs) + 1), rng.integers(0, n_aids, size=ln).tolist())
    return out


def expected(rws, outer_nullable=True):
    """(off int64 [R+1], values int64, null uint8 [R]) of a row list; without a nullable outer group None was written as []"""
    lens = np.array([len(r) if r is not None else 0 for r in rws], dtype=np.int64)
    vals = np.array([v for r in rws if r for v in r], dtype=np.int64)
    null = np.array([r is None and outer_nullable for r in rws], dtype=np.uint8)
    return np.r_[0, np.cumsum(lens)].astype(np.int64), vals, null


def from_pylist(lists):
    return expected(lists, True)


def write(path, rws, elem='int64', outer_nullable=True, elem_nullable=True, item_name=False, **kw):
    """pyarrow-written file with a ``session`` int64 column and the list column; returns the path as str"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    if not outer_nullable:
        rws = [r if r is not None else [] for r in rws]
    et = pa.int64() if elem == 'int64' else pa.int32()
    typ = pa.list_(pa.field('item' if item_name else 'element', et, nullable=elem_nullable))
    schema = pa.schema([pa.field('session', pa.int64()), pa.field(COLUMN, typ, nullable=outer_nullable)])
    tab = pa.table([pa.array(np.arange(len(rws), dtype=np.int64) * 7), pa.array(rws, type=typ)], schema=schema)
    if item_name:
        kw['use_compliant_nested_type'] = False
    pq.write_table(tab, str(path), **kw)
    return str(path)


# name -> (rows, write kwargs): every page shape, value encoding, D and naming SPEC-PQLIST accepts
def cases():
    base = rows()
    small = rows(120, seed=3, longs=())
    return {
        'default': (base, {}),
        'v1_page1k': (base, dict(data_page_size=1024)),
        'v2_page1k': (base, dict(data_page_size=1024, data_page_version='2.0')),
        'none_v1': (base, dict(compression='none', data_page_size=1024)),
        'none_v2': (base, dict(compression='none', data_page_version='2.0')),
        'rowgroups': (base, dict(row_group_size=250, data_page_size=1024)),
        'plain': (base, dict(use_dictionary=False, data_page_size=1024)),
        'delta': (base, dict(use_dictionary=False, column_encoding={COLUMN + '.list.element': 'DELTA_BINARY_PACKED', 'session': 'PLAIN'},
                             data_page_size=1024)),
        'delta_v2': (base, dict(use_dictionary=False, column_encoding={COLUMN + '.list.element': 'DELTA_BINARY_PACKED', 'session': 'PLAIN'},
                                data_page_version='2.0')),
        'int32': (base, dict(elem='int32', data_page_size=1024)),
        'int32_to_int64': (small, dict(elem='int32')),
        'd1': (base, dict(outer_nullable=False, elem_nullable=False, data_page_size=1024)),
        'd2_outer': (base, dict(outer_nullable=True, elem_nullable=False, data_page_size=1024)),
        'd2_elem': (base, dict(outer_nullable=False, elem_nullable=True, data_page_version='2.0', data_page_size=1024)),
        'item_name': (small, dict(item_name=True)),
        'zero_rows': ([], {}),
        'only_empties': ([[] for _ in range(3000)] + [[5]] + [[] for _ in range(3000)], dict(data_page_size=256, use_dictionary=False)),
        'only_nulls': ([None] * 700, {}),
        'one_row': ([[7, 7, 9]], {}),
    }


# ---- the hand writer -------------------------------------------------------------------------------------------------------
def levels_of(rws, outer_optional=True, elem_optional=True):
    """(rep, def, values) of a row list under the three-level LIST form"""
    D = 1 + int(outer_optional) + int(elem_optional)
    rep, dfn, vals = [], [], []
    for r in rws:
        if r is None and outer_optional:
            rep.append(0), dfn.append(0)
        elif not r:
            rep.append(0), dfn.append(int(outer_optional))
        else:
            rep += [0] + [1] * (len(r) - 1)
            dfn += [D] * len(r)
            vals += r
    return np.array(rep, dtype=np.int64), np.array(dfn, dtype=np.int64), np.array(vals, dtype=np.int64)


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def hybrid(levels, width):
    """RLE / bit-packed hybrid of ``levels``: a stretch of >= 8 equal values that starts where no group is open becomes an RLE
    run, everything else bit-packed groups of 8 (the last one zero-padded); consecutive groups share a header."""
    levels = [int(v) for v in levels]
    out, groups, i, n = bytearray(), [], 0, len(levels)

    def flush():
        if groups:
            out.extend(_varint(len(groups) << 1 | 1))
            for g in groups:
                bits = 0
                for k, v in enumerate(g):
                    bits |= v << (k * width)
                out.extend(bits.to_bytes(width, 'little'))
            groups.clear()
    while i < n:
        j = i
        while j < n and levels[j] == levels[i]:
            j += 1
        if j - i >= 8:
            flush()
            out.extend(_varint((j - i) << 1))
            out.extend(levels[i].to_bytes((width + 7) // 8, 'little'))
            i = j
        else:
            g = levels[i:i + 8]
            groups.append(g + [0] * (8 - len(g)))
            i += 8
    flush()
    return bytes(out)


def hand_file(path, rep, dfn, values, cuts, outer_optional=True, elem_optional=True, num_rows=None, declare=None, drop_values=None,
              bump_prefix=None, names=('list', 'element'), level_encodings=(3, 3)):
    """A one-row-group V1 file, uncompressed, PLAIN int64 values, whose only column is the list column; page k holds the level
    entries ``cuts[k] .. cuts[k+1]`` wherever that falls. The edits of the refusal tests: ``num_rows`` (the footer's),
    ``declare`` {page: num_values of its header}, ``drop_values`` {page: values left out at its end}, ``bump_prefix`` {page:
    bytes added to its definition-level length prefix}, ``level_encodings`` (definition, repetition) of the page headers. Returns the
    path as str."""
    from otto_amd.parquet_write import thrift_bytes, T_I32, T_I64, T_BINARY, T_LIST, T_STRUCT, MAGIC
    D = 1 + int(outer_optional) + int(elem_optional)
    wd = 1 if D == 1 else 2
    rep, dfn, values = np.asarray(rep), np.asarray(dfn), np.asarray(values, dtype=np.int64)
    declare, drop_values, bump_prefix = declare or {}, drop_values or {}, bump_prefix or {}
    body = bytearray(MAGIC)
    first = len(body)
    vdone = 0
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        nv = int((dfn[a:b] == D).sum())
        r, d = hybrid(rep[a:b], 1), hybrid(dfn[a:b], wd)
        v = values[vdone:vdone + nv - drop_values.get(k, 0)].astype('<i8').tobytes()
        vdone += nv
        page = struct.pack('<I', len(r)) + r + struct.pack('<I', len(d) + bump_prefix.get(k, 0)) + d + v
        head = thrift_bytes([(1, T_I32, 0), (2, T_I32, len(page)), (3, T_I32, len(page)),
                             (5, T_STRUCT, [(1, T_I32, declare.get(k, b - a)), (2, T_I32, 0), (3, T_I32, level_encodings[0]),
                                            (4, T_I32, level_encodings[1])])])
        body += head + page
    size = len(body) - first
    n_rows = int((rep == 0).sum()) if num_rows is None else num_rows
    meta = [(1, T_I32, 2), (2, T_LIST, (T_I32, [0, 3])), (3, T_LIST, (T_BINARY, [COLUMN, names[0], names[1]])), (4, T_I32, 0),
            (5, T_I64, int(cuts[-1] - cuts[0]) + sum(v - (cuts[k + 1] - cuts[k]) for k, v in declare.items())), (6, T_I64, size), (7, T_I64, size),
            (9, T_I64, first)]
    rg = [(1, T_LIST, (T_STRUCT, [[(2, T_I64, first), (3, T_STRUCT, meta)]])), (2, T_I64, size), (3, T_I64, n_rows)]
    schema = [[(4, T_BINARY, 'schema'), (5, T_I32, 1)],
              [(3, T_I32, int(outer_optional)), (4, T_BINARY, COLUMN), (5, T_I32, 1), (6, T_I32, 3)],
              [(3, T_I32, 2), (4, T_BINARY, names[0]), (5, T_I32, 1)],
              [(1, T_I32, 2), (3, T_I32, int(elem_optional)), (4, T_BINARY, names[1])]]
    foot = thrift_bytes([(1, T_I32, 1), (2, T_LIST, (T_STRUCT, schema)), (3, T_I64, n_rows), (4, T_LIST, (T_STRUCT, [rg])),
                         (6, T_BINARY, b'otto_amd tests')])
    body += foot + struct.pack('<I', len(foot)) + MAGIC
    with open(path, 'wb') as f:
        f.write(bytes(body))
    return str(path)


def footer_file(path, schema):
    """A file of no row groups whose footer holds ``schema``: a list of (name, repetition, physical type or None, children,
    converted type or None) in depth-first order, the root left out"""
    from otto_amd.parquet_write import thrift_bytes, T_I32, T_I64, T_BINARY, T_LIST, T_STRUCT, MAGIC
    els = [[(4, T_BINARY, 'schema'), (5, T_I32, sum(1 for e in schema if e[-1] == 'top'))]]
    for name, rep, phys, kids, conv, *_ in schema:
        el = ([(1, T_I32, phys)] if phys is not None else []) + [(3, T_I32, rep), (4, T_BINARY, name)]
        if kids:
            el.append((5, T_I32, kids))
        if conv is not None:
            el.append((6, T_I32, conv))
        els.append(el)
    foot = thrift_bytes([(1, T_I32, 1), (2, T_LIST, (T_STRUCT, els)), (3, T_I64, 0), (4, T_LIST, (T_STRUCT, [])), (6, T_BINARY, b'otto_amd tests')])
    with open(path, 'wb') as f:
        f.write(MAGIC + foot + struct.pack('<I', len(foot)) + MAGIC)
    return str(path)


def hand_rows(seed=5):
    """701 rows: a random mix with nulls and empties, the stretches of equal rows and a 2,500-value row"""
    return rows(100, seed=seed, longs=(2500,))


def hand_cuts(n_levels, seed=5, pages=13, extra=()):
    rng = np.random.default_rng(seed)
    return sorted({0, n_levels, *extra, *(int(c) for c in rng.choice(np.arange(1, n_levels), size=pages - 1, replace=False))})


def empties_stretch(rws):
    """(first, end) level positions of the first 100 consecutive empty lists of :func:`rows`"""
    lens = np.array([max(len(r), 1) if r is not None else 1 for r in rws])
    at = np.r_[0, np.cumsum(lens)]
    i = next(i for i in range(len(rws)) if all(r == [] for r in rws[i:i + 100]))
    return int(at[i]), int(at[i + 100])


def hand_case(seed=5):
    """(rows, rep, def, values, cuts) of the hand-cut file: 13 random cuts plus a page inside the stretch of empty lists"""
    rws = [[3, 1, 4]] + hand_rows(seed)
    rep, dfn, vals = levels_of(rws)
    a, b = empties_stretch(rws)
    return rws, rep, dfn, vals, hand_cuts(len(rep), seed, extra=(a + 20, b - 20))


def damaged(d):
    """Hand-damaged copies of the hand-cut file, one per device refusal: name -> (path, page, reason code of
    pqlist_restatement or None for the value-count refusal of the value decode)"""
    import pqlist_restatement as R
    rws, rep, dfn, vals, cuts = hand_case()
    page_of = lambda i: int(np.searchsorted(cuts, i, side='right') - 1)
    mixed = next(i for i in range(cuts[6], len(rep)) if rep[i] == 1 and rep[i + 1] == 0 and rep[i - 1] == 1)      # the last element of a list
    out = {}
    rep2, dfn2, vals2 = levels_of(rws, True, False)
    bad = dfn2.copy()
    bad[mixed] = 3
    out['level_above_max'] = (hand_file(d / 'level.parquet', rep2, bad, vals2, cuts, True, False), page_of(mixed), R.LEVEL)
    bad = dfn.copy()
    bad[mixed] = 2
    out['null_element'] = (hand_file(d / 'nullelem.parquet', rep, bad, vals, cuts), page_of(mixed), R.NULL_ELEM)
    bad = dfn.copy()
    bad[mixed] = 1
    out['rep_without_element'] = (hand_file(d / 'repempty.parquet', rep, bad, vals, cuts), page_of(mixed), R.REP_EMPTY)
    n4 = cuts[5] - cuts[4]
    out['stream_short'] = (hand_file(d / 'short.parquet', rep, dfn, vals, cuts, declare={4: n4 + 16}), 4, R.SHORT)
    out['stream_long'] = (hand_file(d / 'long.parquet', rep, dfn, vals, cuts, declare={4: n4 - 16}), 4, R.LONG)
    out['prefix'] = (hand_file(d / 'prefix.parquet', rep, dfn, vals, cuts, bump_prefix={7: 10 ** 6}), 7, R.PREFIX)
    bad = rep.copy()
    bad[0] = 1
    out['chunk_opens_with_rep_1'] = (hand_file(d / 'chunkrep.parquet', bad, dfn, vals, cuts), 0, R.CHUNK_REP)
    out['row_count'] = (hand_file(d / 'rowcount.parquet', rep, dfn, vals, cuts, num_rows=len(rws) + 1), 0, R.ROWS)
    out['value_count'] = (hand_file(d / 'valuecount.parquet', rep, dfn, vals, cuts, drop_values={11: 1}), 11, None)
    return out


# ---- label frames ----------------------------------------------------------------------------------------------------------
def label_rows(n_sessions, seed=0, n_aids=5000, shuffle=True, cart_len=300):
    """(session int64, type uint8, lists) in the shape of val_labels.parquet: per session a random subset of the three types
    (some sessions have none and do not appear), clicks one aid, carts / orders short lists with repeated aids; one cart list
    of ``cart_len`` values; rows in shuffled file order."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(11, 11 + 4 * n_sessions + 1), size=n_sessions, replace=False)).astype(np.int64)
    sess, typ, lists = [], [], []
    for i, s in enumerate(ids):
        present = rng.integers(0, 8)                           # a bit per type; 0: the session has no row
        for t in range(3):
            if present >> t & 1:
                sess.append(int(s)), typ.append(t)
                n = 1 if t == 0 else int(rng.integers(1, 9))
                lists.append(rng.integers(0, min(n_aids, 40 if t else n_aids), size=n).tolist())
    if cart_len and lists:
        k = next((j for j, t in enumerate(typ) if t == 1), None)
        if k is not None:
            lists[k] = rng.integers(0, n_aids, size=cart_len).tolist()
    order = rng.permutation(len(sess)) if shuffle else np.arange(len(sess))
    return (ids, np.array(sess, dtype=np.int64)[order], np.array(typ, dtype=np.uint8)[order], [lists[j] for j in order])


def label_frame(sess, typ, lists):
    import pandas as pd
    names = np.array(['clicks', 'carts', 'orders'])
    return pd.DataFrame({'session': sess, 'type': names[typ], COLUMN: [np.array(l, dtype=np.int64) for l in lists]})
