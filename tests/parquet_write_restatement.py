"""SPEC-PQWRITE (include/otto_pqwrite.h) restated in NumPy and Python integers: the bytes of a PLAIN and of a
DELTA_BINARY_PACKED page body. It is the byte oracle of tests/test_parquet_write_cpu.py and tests/test_parquet_write_gpu.py and
shares no code with otto_amd/parquet_write.py or csrc/parquet_encode.h."""
import numpy as np

PLAIN, DELTA = 0, 5
BLOCK, MINIBLOCKS, MINI = 128, 4, 32


def stored(a):
    """The stored values of a column: int32 / int64 / float32 / float64, as the table of the spec says."""
    a = np.asarray(a)
    if a.dtype.kind == 'f':
        if a.dtype.itemsize not in (4, 8):
            raise ValueError(a.dtype)
        return a
    if a.dtype.kind not in 'iu':
        raise ValueError(a.dtype)
    if a.dtype.itemsize == 8:
        return a.view(np.int64)
    if a.dtype.itemsize == 4:
        return a.view(np.int32)
    return a.astype(np.int32)                 # sign- or zero-extension by the element's own kind


def plain_body(a):
    return stored(a).astype(stored(a).dtype.newbyteorder('<')).tobytes()


def uleb(v):
    assert v >= 0
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def zigzag(v):
    return 2 * v if v >= 0 else -2 * v - 1


class DomainError(ValueError):
    def __init__(self, row):
        super().__init__(f'row {row}: outside the domain of the delta encoding')
        self.row = row


def delta_body(a):
    s = stored(a)
    if s.dtype.kind == 'f':
        raise ValueError('DELTA_BINARY_PACKED is for integer columns')
    limit = 1 << 31 if s.dtype.itemsize == 4 else 1 << 62
    v = [int(x) for x in s]
    for i, x in enumerate(v):
        if not 0 <= x < limit:
            raise DomainError(i)
    n = len(v)
    out = bytearray(uleb(BLOCK) + uleb(MINIBLOCKS) + uleb(n) + uleb(zigzag(v[0] if n else 0)))
    deltas = [v[i] - v[i - 1] for i in range(1, n)]
    for b0 in range(0, len(deltas), BLOCK):
        block = deltas[b0:b0 + BLOCK]
        m = min(block)
        minis = [[d - m for d in block[j:j + MINI]] for j in range(0, len(block), MINI)]
        widths = [max(mb).bit_length() for mb in minis]
        out += uleb(zigzag(m)) + bytes(widths + [0] * (MINIBLOCKS - len(widths)))
        for mb, w in zip(minis, widths):
            acc = 0
            for i, r in enumerate(mb):            # positions past the last delta stay 0: the padding
                acc |= r << (i * w)
            out += acc.to_bytes(4 * w, 'little')
    return bytes(out)


def page_body(a, encoding):
    return delta_body(a) if encoding == DELTA else plain_body(a)


# ---- the case lists both test modules use -------------------------------------------------------------------------------
EDGE_ROWS = (0, 1, 2, 33, 34, 129, 130, 255, 256, 257, 512, 513, 1025)
N_AIDS = 1855603


def pattern(name, n, seed=0):
    """The value patterns both test modules encode, ``n`` rows each; the dtype is part of the pattern."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if name == 'constant':
        return np.full(n, 77, dtype=np.int32)
    if name == 'plus_one':
        return (i + 5).astype(np.int32)
    if name == 'runs_of_20':
        return np.repeat(np.sort(rng.choice(N_AIDS, size=n // 20 + 1, replace=False)), 20)[:n].astype(np.int32)
    if name == 'alt_int32':
        return np.where(i % 2 == 0, 0, 2 ** 31 - 1).astype(np.int32)
    if name == 'alt_int64':
        return np.where(i % 2 == 0, 0, 2 ** 62 - 1).astype(np.int64)
    if name == 'w0_beside_w32':
        # every delta is -1 but one: 40 steps down to 0, a jump to 2^31 - 1, steps down again. In block 0 m = -1, miniblock 1
        # holds the jump (relative delta 2^31, width 32), miniblocks 0, 2 and 3 have width 0
        v = np.where(i <= 40, 40 - i, 2 ** 31 - 1 - (i - 41))
        return v.astype(np.int32)
    if name == 'random_aids':
        return rng.integers(0, N_AIDS, size=n).astype(np.int32)
    raise KeyError(name)


PATTERNS = ('constant', 'plus_one', 'runs_of_20', 'alt_int32', 'alt_int64', 'w0_beside_w32', 'random_aids')
PATTERN_ROWS = (130, 257)


def width_block(w, dtype):
    """129 values whose 128 deltas alternate +a, -b with a + b = 2^w - 1 (a = 2^(w-1), b = a - 1), so m = -b and the largest
    relative delta of every miniblock is 2^w - 1: a block of four width bytes w. At the top width of a type (32 for INT32, 63
    for INT64) the domain allows 2^w - 2 at the most (a = b = the largest value), which still has w bits."""
    top = int(np.iinfo(dtype).max) if np.dtype(dtype).itemsize == 4 else 2 ** 62 - 1
    a = 1 << (w - 1) if w else 0
    b = a - 1 if w else 0
    if a > top:
        a = b = top
    v = [0]
    for k in range(BLOCK):
        v.append(v[-1] + (a if k % 2 == 0 else -b))
    return np.array(v, dtype=dtype)


def width_cases():
    """(w, values) for every w in 0..32 as INT32 and 33..63 as INT64."""
    return [(w, width_block(w, np.int32 if w <= 32 else np.int64)) for w in range(0, 64)]


PLAIN_DTYPES = ('int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64')
PLAIN_ROWS = (0, 1, 257, 1025)


def plain_column(dtype, n, seed=0):
    """Values over the whole range of the element type: negative ones, and ones at and above 2^31."""
    rng = np.random.default_rng(seed + 1)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return (rng.standard_normal(n) * 1e3).astype(dt)
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    if n:
        a[0] = info.max
    if n > 1:
        a[1] = info.min
    return a
