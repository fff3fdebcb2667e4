"""Inputs of the SPEC-DEFLATE tests, shared by test_deflate_cpu.py and test_deflate_gpu.py, all seeded. A case is
(bytes, block_bytes); ``expected(name)`` is the restatement's output, computed once per process."""
import functools

import numpy as np

import deflate_restatement as dr

MIN_MATCH = dr.MIN_MATCH
TILE = 64                  # items per round of the emit kernel: the tokens and end-of-block
N_AIDS = 1855603
FIRST_SESSION = 12899779
SUFFIX = ('clicks', 'carts', 'orders')


# ---- the submission texts -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _popularity():
    """cumulated weights of the aids: a lognormal popularity law, median 20, sigma 1.88"""
    return np.cumsum(np.exp(np.random.default_rng(0).normal(np.log(20.0), 1.88, N_AIDS)))


def _lists(rng, lines, k=20):
    cum = _popularity()
    return np.minimum(np.searchsorted(cum, rng.random((lines, k)) * cum[-1]), N_AIDS - 1)


def _line(session, t, aids):
    return f'{session}_{SUFFIX[t]},{" ".join(str(int(a)) for a in aids)}\n'


@functools.lru_cache(maxsize=None)
def text_a(lines=700, seed=1):
    """three blocks of independent lists (the blend script's order)"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(3):
        lists = _lists(rng, lines)
        out += [_line(FIRST_SESSION + s, t, lists[s]) for s in range(lines)]
    return ''.join(out).encode()


@functools.lru_cache(maxsize=None)
def text_b(lines=700, seed=2):
    """interleaved, 60 % of a session's order lists equal to its cart list (the covisitation script)"""
    rng = np.random.default_rng(seed)
    lists = [_lists(rng, lines) for _ in range(3)]
    same = rng.random(lines) < 0.6
    out = []
    for s in range(lines):
        for t in range(3):
            out.append(_line(FIRST_SESSION + s, t, lists[1][s] if t == 2 and same[s] else lists[t][s]))
    return ''.join(out).encode()


# ---- building blocks ------------------------------------------------------------------------------------------------------
def _random(seed, n, values=256):
    return bytes(np.random.default_rng(seed).integers(0, values, n, dtype=np.uint8))


def _distinct(n, first=0):
    """n bytes without any repeated byte pair: no match of any length >= 2 (n <= 256)"""
    assert n <= 256
    return bytes((first + 7 * i) % 256 for i in range(n))


def _shuffled(seed, counts):
    """symbol -> count, shuffled"""
    a = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in counts.items()])
    np.random.default_rng(seed).shuffle(a)
    return bytes(a)


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _fibonacci(k=22, period=5):
    """Literal counts 1, 1, 2, 3, 5, ... of k byte values, which take the unlimited code to 16 bits. Every period-th byte
    is a separator that changes from one to the next, so that matches stay too few to flatten the counts."""
    pay = np.frombuffer(_shuffled(6, dict(enumerate(_fib(k)))), dtype=np.uint8)
    n = len(pay) // (period - 1)
    x = np.empty((n, period), dtype=np.uint8)
    x[:, :period - 1] = pay[:n * (period - 1)].reshape(n, period - 1)
    i = np.arange(n)
    x[:, period - 1] = 128 + (i * 37 + i // 128) % 128
    return bytes(x.ravel())


def _seam():
    """A repeat token (symbol 16) that starts at the last literal/length code and runs on over the first two distance
    codes: symbols 284 and 285 eight times each beside 13 other symbols of count 1, so both get 2 bits, and the distance
    symbols 0, 1, 3 and 4 four times each, 2 bits too. Four times: a run (a literal and a distance-1 match of 253 or 248)
    that ends 2 bytes before a batch of the match finder starts, then a pattern of period 2 whose matches of 258, 258 and
    257 start 0, 2 and 4 bytes into a batch and so find the distances 2, 4 and 6."""
    out = bytearray()
    for u in range(4):
        out += bytes([ord('a') + u]) * (1 + (253 if u == 0 else 248))
        assert len(out) % dr.BATCH == dr.BATCH - 2
        out += (bytes([ord('K') + 2 * u, ord('L') + 2 * u]) * 400)[:2 + 258 + 258 + 257]
    return bytes(out)


def _equal_counts(seed, values, count):
    """every byte value below ``values`` ``count`` times, shuffled: no match, code lengths of floor and ceil of log2"""
    return _shuffled(seed, {v: count for v in range(values)})


def crossing_repeat(plan):
    """does a symbol-16 token of the plan's run-length tokens cover code lengths on both sides of HLIT?"""
    i = 0
    for s, _, v in plan['rl']:
        t = {16: v + 3, 17: v + 3, 18: v + 11}.get(s, 1)
        if s == 16 and i < plan['hlit'] < i + t:
            return True
        i += t
    return False


def _used(values, seed, n=400):
    """n bytes over exactly the given byte values"""
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.array(values, dtype=np.uint8), rng.choice(np.array(values, dtype=np.uint8), n - len(values))])
    rng.shuffle(a)
    return bytes(a)


def _gaps(gaps):
    """byte values whose consecutive distances leave the given runs of unused values"""
    out, v = [0], 0
    for g in gaps:
        v += g + 1
        out.append(v)
    assert v <= 255
    return out


def _build():
    M, B = MIN_MATCH, dr.BLOCK_MAX
    text = text_a()
    s20 = bytes(97 + v for v in _random(11, 20, 25))         # letters a..y; 'z' is the filler below
    c = {}
    # sizes
    for n in (0, 1, 2, 3):
        c[f'n{n}'] = (text[:n], B)
    for bb, m in ((1, 3), (7, 3), (64, 3), (65, 3), (4096, 2), (65535, 1), (65536, 1)):
        for d in (-1, 0, 1):
            n = m * bb + d
            c[f'size-bb{bb}-{"m" if d < 0 else "p"}{abs(d)}'] = (text[1000:1000 + n], bb)
    # alphabet
    c['one-byte'] = (b'a' * 1000, B)                          # distance-1 overlapping matches, one distance symbol
    c['two-bytes'] = (_random(3, 2000, 2), B)
    c['all-256-once'] = (bytes(np.random.default_rng(4).permutation(256).astype(np.uint8)), B)
    c['all-256-equal'] = (b''.join(bytes(np.random.default_rng(5 + i).permutation(256).astype(np.uint8)) for i in range(4)), B)
    c['no-match'] = (_distinct(200), B)
    c['one-match'] = (_distinct(100) + _distinct(10), B)      # its first 10 bytes again
    c['fibonacci'] = (_fibonacci(), B)
    # header coding
    c['zero-runs-a'] = (_used(_gaps((1, 2, 3, 10, 11, 138)), 7), B)
    c['zero-runs-b'] = (_used(_gaps((139, 10, 3)), 8), B)
    counts, base = {}, 10
    for k in (4, 7, 8):                                      # 4, 7 and 8 neighbours of equal counts
        counts.update({base + j: 8 for j in range(k)})
        base += k + 5
    c['repeat-runs'] = (_shuffled(9, counts), B)
    c['seam-repeat'] = (_seam(), B)
    c['hclen-6'] = (_equal_counts(21, 192, 16), B)             # lengths 7 and 8 alone: the shortest header that is emitted
    c['hclen-5-stored'] = (_equal_counts(21, 255, 12), B)     # length 8 alone: HCLEN 5 in the plan, but stored is no larger
    c['top-285'] = (_distinct(30) + b'q' * 300, B)            # a match of 258: the last literal/length symbol
    c['top-lowest-length'] = (_distinct(30) + b'q' * (1 + M), B)        # one match of MIN_MATCH: symbol 254 + MIN_MATCH
    # matches
    c['len-min-1'] = (b'abc' + b'x' * M + b'def', B)          # the run gives a match of MIN_MATCH - 1: literals
    c['len-min'] = (b'abc' + b'x' * (M + 1) + b'def', B)
    c['len-min-far'] = (_distinct(64) + _distinct(M) + b'\xff\xfe', B)   # found through the table, exactly MIN_MATCH
    c['len-258'] = (b'ab' + b'x' * 259 + b'cd', B)
    c['len-259'] = (b'ab' + b'x' * 260 + b'cd', B)
    c['len-258+min'] = (b'ab' + b'x' * (259 + M) + b'cd', B)
    c['match-to-end'] = (_distinct(70) + _distinct(17), B)
    c['dist-32768'] = (s20 + b'z' * (32768 - 20) + s20 + b'!', B)
    c['dist-32769'] = (s20 + b'z' * (32769 - 20) + s20 + b'!', B)
    c['across-cut'] = (_distinct(44) + s20 + s20 + _distinct(44, 3), 64)     # the second copy opens block 1
    # bit packing
    c['ragged'] = (text[5000:8000], 37)
    for n in (TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 2, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        c[f'tile-{n}'] = (_distinct(n, n), B)                 # n literals and end-of-block
    # stored fallback
    c['stored-65535'] = (_random(12, 65535), B)
    c['stored-65536'] = (_random(13, 65536), B)
    c['stored-small'] = (_random(14, 50), B)
    c['dynamic-equals-stored'] = (bytes(np.random.default_rng(69).integers(0, 26, 25, dtype=np.uint8)), B)
    # texts
    c['text-a'] = (text_a(), B)
    c['text-b'] = (text_b(), B)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


CASE_NAMES = tuple(cases().keys())


def case(name):
    return cases()[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    data, bb = case(name)
    return dr.gzip_members(data, bb)


@functools.lru_cache(maxsize=None)
def plans(name):
    """the restatement's plan of every non-empty block"""
    data, bb = case(name)
    return [dr.plan(data[lo:lo + bb]) for lo in range(0, len(data), bb)]


def zlib_size(data, level, strategy=0, block_bytes=dr.BLOCK_MAX):
    """bytes of zlib's gzip members over the same cut"""
    import zlib
    total = 0
    for lo in range(0, len(data), block_bytes):
        z = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
        total += len(z.compress(data[lo:lo + block_bytes]) + z.flush())
    return total
