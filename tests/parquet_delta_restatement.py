"""DELTA_BINARY_PACKED page bodies in Python integers (SPEC-PARQUET, "Delta pages", include/otto_parquet.h): an encoder
and a decoder for any block shape ``(B, M)``. Shares no code with the product; pyarrow is the oracle for both (the tests
read the files assembled from :func:`encode` with ``pq.read_table`` and decode pyarrow-written pages with :func:`decode`).

A body is what lies behind the levels of a data page. :func:`decode` gives the values or the refusal code the product
must give (``REASONS``: the ``PQ_E_DELTA_*`` of csrc/parquet_decode.h, by their ``otto_parquet_reason`` texts)."""
import numpy as np

SHAPES = ((128, 4), (256, 4), (256, 8), (512, 2))
VARINT, SHAPE, COUNT, WIDTH, TRUNC, TRAILING = 12, 13, 14, 15, 16, 17
REASONS = {VARINT: 'delta: a varint of more than 10 bytes or 64 bits',
           SHAPE: 'delta: block shape (values per block, miniblocks per block) is not accepted',
           COUNT: "delta: the header's value count differs from the page's",
           WIDTH: "delta: miniblock width above the physical type's bits",
           TRUNC: 'delta: the stream runs past the page body',
           TRAILING: 'delta: bytes behind the last miniblock'}


class Refused(Exception):
    def __init__(self, code):
        super().__init__(REASONS[code])
        self.code = code


def uleb(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v, bits=64):
    """zigzag ULEB128 of the signed value ``v`` (taken modulo 2^bits into the signed range first)"""
    v &= (1 << bits) - 1
    if v >> (bits - 1):
        v -= 1 << bits
    return uleb((v << 1) ^ (v >> 63) if v >= 0 else ((-v) << 1) - 1)


def stored(a):
    """the values as Python integers in the signed range of the physical type, and the type's bits"""
    a = np.asarray(a)
    bits = 64 if a.dtype.itemsize == 8 else 32
    signed = a.astype(np.int64 if bits == 64 else np.int32) if a.dtype.kind == 'i' else a.astype(np.uint64 if bits == 64 else np.uint32).view(
        np.int64 if bits == 64 else np.int32)
    return [int(x) for x in signed], bits


def encode(values, bits, B=128, M=4, garbage=None, header_n=None):
    """The body of one delta page of the signed integers ``values`` of a ``bits``-bit physical type: deltas modulo 2^bits
    as signed numbers, min_delta per block, the bit length of the largest relative delta per miniblock. ``garbage``: the
    width byte of the miniblocks that hold no value (the format lets it be anything; default 0). ``header_n``: a value
    count to state instead of the true one."""
    assert B % 128 == 0 and B % M == 0 and (B // M) % 32 == 0
    mv, mask, n = B // M, (1 << bits) - 1, len(values)

    def signed(x):
        x &= mask
        return x - (1 << bits) if x >> (bits - 1) else x
    out = bytearray(uleb(B) + uleb(M) + uleb(n if header_n is None else header_n) + zigzag(values[0] if n else 0, bits))
    deltas = [signed(values[i + 1] - values[i]) for i in range(n - 1)]
    for b0 in range(0, len(deltas), B):
        blk = deltas[b0:b0 + B]
        m = min(blk)
        rel = [(d - m) & mask for d in blk]
        out += zigzag(m, bits)
        widths, packed = [], bytearray()
        for j in range(M):
            mini = rel[j * mv:(j + 1) * mv]
            if not mini:
                widths.append(0 if garbage is None else garbage)
                continue
            w = max(x.bit_length() for x in mini)
            widths.append(w)
            acc = 0
            for i, x in enumerate(mini):
                acc |= x << (i * w)
            packed += acc.to_bytes(mv * w // 8, 'little')
        out += bytes(widths) + packed
    return bytes(out)


def _varint(body, pos):
    v = 0
    for i in range(10):
        if pos >= len(body):
            raise Refused(TRUNC)
        b = body[pos]
        pos += 1
        if i == 9 and b & 0xFE:
            raise Refused(VARINT)
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return v, pos
    raise Refused(VARINT)


def _unzigzag(u):
    return (u >> 1) ^ -(u & 1)


def decode(body, num_values, bits):
    """The ``num_values`` values of the body as unsigned integers modulo 2^bits, or :class:`Refused`."""
    body = bytes(body)
    mask = (1 << bits) - 1
    B, pos = _varint(body, 0)
    M, pos = _varint(body, pos)
    n, pos = _varint(body, pos)
    first, pos = _varint(body, pos)
    if B < 128 or B > 65536 or B % 128 or M < 1 or B % M or (B // M) % 32:
        raise Refused(SHAPE)
    if n != num_values:
        raise Refused(COUNT)
    mv = B // M
    out = [_unzigzag(first) & mask] if n else []
    left = max(n - 1, 0)
    while left:
        md, pos = _varint(body, pos)
        md = _unzigzag(md)
        if pos + M > len(body):
            raise Refused(TRUNC)
        widths = body[pos:pos + M]
        pos += M
        take = min(left, B)
        for j in range(-(-take // mv)):
            w = widths[j]
            if w > bits:
                raise Refused(WIDTH)
            nb = mv * w // 8
            if pos + nb > len(body):
                raise Refused(TRUNC)
            acc = int.from_bytes(body[pos:pos + nb], 'little')
            pos += nb
            for i in range(min(mv, take - j * mv)):
                out.append((out[-1] + md + ((acc >> (i * w)) & ((1 << w) - 1))) & mask)
        left -= take
    if pos != len(body):
        raise Refused(TRAILING)
    return out


def as_array(values, dtype):
    """decoded values (unsigned, modulo 2^bits) as a NumPy array of ``dtype`` (same width: the bits)"""
    dtype = np.dtype(dtype)
    u = np.array(values, dtype=np.uint64 if dtype.itemsize == 8 else np.uint32)
    return u.view(dtype) if u.size else u.astype(dtype)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def counts(B):
    """value counts with the last miniblock partly filled, around the block edges of block size B"""
    return sorted({0, 1, 2, 33, 128, 129, 130, 257, B + 1, B + 2, 2 * B + 1})


def every_width(bits, B, M, seed=0):
    """A column in which miniblock j (of ``B // M`` values) has width j % (bits + 1) exactly, over enough blocks for every
    width 0..bits. Every block's min_delta is the type's minimum, so min_delta + relative delta never leaves the signed
    range and the writer's widths are the ones chosen here; each miniblock holds the largest relative delta of its width
    (2^w - 1) and a 0. The values wrap modulo 2^bits."""
    rng = np.random.default_rng(seed)
    mv, mask, lo = B // M, (1 << bits) - 1, -(1 << (bits - 1))
    v = int(rng.integers(0, 1000))
    vals = [v]
    for j in range(-(-(bits + 1) // M) * M):
        w = j % (bits + 1)
        rel = [int(rng.integers(0, 1 << 62)) & ((1 << w) - 1) for _ in range(mv)]
        if w == 64:
            rel = [r | int(rng.integers(0, 4)) << 62 for r in rel]
        rel[0], rel[1] = (1 << w) - 1, 0
        for r in rel:
            v = (v + lo + r) & mask
            vals.append(v)
    signed = [x - (1 << bits) if x >> (bits - 1) else x for x in vals]
    return np.array(signed, dtype=np.int64 if bits == 64 else np.int32)


def widths_seen(body, num_values):
    """the widths of the miniblocks of a valid body that hold a value"""
    body = bytes(body)
    B, pos = _varint(body, 0)
    M, pos = _varint(body, pos)
    _, pos = _varint(body, pos)
    _, pos = _varint(body, pos)
    mv, left, seen = B // M, max(num_values - 1, 0), set()
    while left:
        _, pos = _varint(body, pos)
        widths = body[pos:pos + M]
        pos += M
        take = min(left, B)
        for j in range(-(-take // mv)):
            seen.add(widths[j])
            pos += mv * widths[j] // 8
        left -= take
    return seen


def wrap_around(bits, n):
    """values that alternate between the type's extremes (and 0 / -1): every delta wraps"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    pat = [lo, hi, hi, lo, 0, -1, hi, -1, lo, 1]
    return np.array([pat[i % len(pat)] for i in range(n)], dtype=np.int64 if bits == 64 else np.int32)


def random_column(bits, n, seed, kind='walk'):
    rng = np.random.default_rng(seed)
    dt = np.int64 if bits == 64 else np.int32
    if kind == 'walk':                                        # small mixed-sign steps
        return np.cumsum(rng.integers(-50, 1000, size=n)).astype(dt)
    if kind == 'sorted':
        return np.sort(rng.integers(0, 1 << 21, size=n)).astype(dt)
    return rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, size=n, dtype=np.int64).astype(dt)
