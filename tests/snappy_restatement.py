"""SPEC-SNAPPY (include/otto_snappy.h) restated in plain Python + NumPy, written from the header's text: a byte string ->
the bytes of its Snappy raw-format stream. Sequential on purpose; the device kernels (csrc/otto_snappy.hip) must produce
these bytes exactly. The parameters are read from the header's ``#define``s, so the two cannot drift apart; every function
takes them as arguments too, which is how the table in the header comment was measured (``python tests/snappy_restatement.py``)."""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'otto_snappy.h')


def header_defines(path=HEADER):
    """``{name: int}`` of the ``#define OTTO_SNAPPY_* <integer>`` lines of the header."""
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define\s+(OTTO_SNAPPY_\w+)\s+(\d+)\b', f.read(), flags=re.M)}


_D = header_defines()
FRAGMENT = _D['OTTO_SNAPPY_FRAGMENT']
MIN_MATCH = _D['OTTO_SNAPPY_MIN_MATCH']
HASH_BYTES = _D['OTTO_SNAPPY_HASH_BYTES']
HASH_BITS = _D['OTTO_SNAPPY_HASH_BITS']
BATCH = _D['OTTO_SNAPPY_BATCH']
MAX_MATCH = _D['OTTO_SNAPPY_MAX_MATCH']
HASH_MUL = 0x9E3779B97F4A7C15
NEAR = (1, 4, 8)           # the fixed-distance candidates, in the order of the spec


def bound(n):
    """otto_snappy_bound"""
    return 32 + n + n // 6


def uleb128(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _common(x, a, b, limit):
    if x[a] != x[b]:
        return 0
    if x[a:a + limit] == x[b:b + limit]:       # never true for an overlapping pair unless the whole stretch repeats
        return limit
    n = 1
    while x[a + n] == x[b + n]:
        n += 1
    return n


def _slots(x, hash_bytes, hash_bits):
    """The slot of every position p with p + hash_bytes <= len(x)."""
    m = len(x) - hash_bytes + 1
    if m <= 0:
        return np.zeros(0, dtype=np.int64)
    a = np.frombuffer(x, dtype=np.uint8).astype(np.uint64)
    v = np.zeros(m, dtype=np.uint64)
    for i in range(hash_bytes):
        v |= a[i:i + m] << np.uint64(8 * i)
    return ((v * np.uint64(HASH_MUL)) >> np.uint64(64 - hash_bits)).astype(np.int64)


def tokens(x, min_match=MIN_MATCH, hash_bytes=HASH_BYTES, hash_bits=HASH_BITS, near=NEAR):
    """The match finder and the greedy selection of one fragment: a list of ints (a literal byte) and (length, distance)."""
    x = bytes(x)
    m = len(x)
    slot = _slots(x, hash_bytes, hash_bits)
    table = np.full(1 << hash_bits, -1, dtype=np.int64)
    out = []
    p = 0
    for base in range(0, m, BATCH):
        top = min(base + BATCH, m)
        s = slot[base:top]                                   # the positions of the batch that have a slot
        seen = table[s].tolist()                             # what the batch sees: earlier batches only
        table[s] = np.arange(base, base + len(s))            # ascending, the last assignment stays: the largest position
        while p < top:
            limit = min(MAX_MATCH, m - p)
            length, dist = 0, 0
            cands = [p - d for d in near if p - d >= 0]
            if p - base < len(seen) and seen[p - base] >= 0:
                cands.append(seen[p - base])
            for c in cands:
                n = _common(x, c, p, limit)
                if n > length:                               # a tie stays with the earlier candidate
                    length, dist = n, p - c
            if length >= min_match:
                out.append((length, dist))
                p += length
            else:
                out.append(x[p])
                p += 1
    return out


def literal_element(data):
    n = len(data)
    if n <= 60:
        return bytes([(n - 1) << 2]) + data
    if n <= 256:
        return bytes([60 << 2, n - 1]) + data
    return bytes([61 << 2, (n - 1) & 0xFF, (n - 1) >> 8]) + data


def copy_element(length, dist):
    if 4 <= length <= 11 and dist < 2048:
        return bytes([1 | (length - 4) << 2 | (dist >> 8) << 5, dist & 0xFF])
    return bytes([2 | (length - 1) << 2, dist & 0xFF, dist >> 8])


def fragment(x, **kw):
    """The elements of one fragment."""
    x = bytes(x)
    out, run, p = bytearray(), 0, 0
    for t in tokens(x, **kw):
        if isinstance(t, tuple):
            if run:
                out += literal_element(x[p - run:p])
                run = 0
            out += copy_element(*t)
            p += t[0]
        else:
            run += 1
            p += 1
    if run:
        out += literal_element(x[p - run:p])
    return bytes(out)


def compress(x, **kw):
    """One Snappy raw-format stream of the bytes ``x``."""
    x = bytes(x)
    return uleb128(len(x)) + b''.join(fragment(x[i:i + FRAGMENT], **kw) for i in range(0, len(x), FRAGMENT))


def _table():
    """The table of the header comment: the sizes of the column inputs for a handful of settings, beside pyarrow's."""
    import pyarrow as pa
    import snappy_inputs
    cols = snappy_inputs.columns()
    codec = pa.Codec('snappy')
    print('H / MIN_MATCH / bits / near       ' + ''.join(f'{n:>10}' for n in cols))
    print('raw bytes                         ' + ''.join(f'{len(v):>10}' for v in cols.values()))
    print("pyarrow Codec('snappy')           " + ''.join(f'{len(codec.compress(v, asbytes=True)):>10}' for v in cols.values()))
    for h, mm, bits, near in ((4, 4, 12, NEAR), (5, 5, 12, NEAR), (6, 6, 12, NEAR), (8, 8, 12, NEAR), (4, 6, 12, NEAR), (6, 6, 11, NEAR),
                              (6, 6, 10, NEAR), (6, 6, 13, NEAR), (6, 6, 12, (1,))):
        sizes = [len(compress(v, min_match=mm, hash_bytes=h, hash_bits=bits, near=near)) for v in cols.values()]
        print(f'{h} / {mm} / {bits} / {",".join(map(str, near)):<20}' + ''.join(f'{s:>10}' for s in sizes))


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _table()
