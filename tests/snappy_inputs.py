"""Named inputs of the Snappy encoder tests (SPEC-SNAPPY, include/otto_snappy.h): every length and content at which the
match finder, the element forms or the fragment cut take another path, and the synthetic columns the parameter table of the
header comment is measured on. Each is a few hundred KB at most. ``inputs()`` -> ``{name: bytes}``, built once."""
import functools

import numpy as np

FRAGMENT = 65536
HASH_BYTES = 6             # the lengths H - 1, H, H + 1 below; test_snappy_cpu.py checks it against the header
ROWS = 40000


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _planted(rng, n, src, dst, length):
    """Random bytes in which [dst, dst + length) repeats [src, src + length) and the bytes around both differ."""
    a = bytearray(_rand(rng, n))
    a[dst:dst + length] = a[src:src + length]
    for s, d in ((src - 1, dst - 1), (src + length, dst + length)):      # exactly `length`: no accidental extension
        if 0 <= s and d < n and a[s] == a[d]:
            a[d] ^= 0x55
    return bytes(a)


@functools.lru_cache(maxsize=None)
def columns():
    """The chunk-writer columns and the covisitation weight column of about 40,000 rows, as the bytes of a PLAIN page."""
    rng = np.random.default_rng(20240607)
    lengths = np.minimum(rng.geometric(0.18, ROWS), 200)
    lengths = lengths[np.cumsum(lengths) <= ROWS]
    n = int(lengths.sum())
    session = np.repeat(11_098_528 + np.arange(len(lengths)), lengths).astype(np.int32)
    aid = np.minimum(rng.zipf(1.25, n) * 37 % 1_855_603, 1_855_602).astype(np.int32)
    start = 1_661_724_000 + np.sort(rng.integers(0, 7 * 86400, len(lengths)))
    ts = (np.repeat(start, lengths) + np.concatenate([np.cumsum(rng.integers(1, 600, k)) for k in lengths])).astype(np.int64)
    typ = rng.choice(3, n, p=[0.9, 0.07, 0.03]).astype(np.int32)
    wgt = (rng.geometric(0.35, n) + 0.5 * (rng.random(n) < 0.3)).astype(np.float32)
    return {'session': session.tobytes(), 'aid': aid.tobytes(), 'ts': ts.tobytes(), 'type': typ.tobytes(), 'wgt': wgt.tobytes()}


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(7)
    H = HASH_BYTES
    out = {}
    for n in (0, 1, 3, H - 1, H, H + 1, 59, 60, 61, 63, 64, 65, 256, 257, FRAGMENT - 1, FRAGMENT, FRAGMENT + 1, 2 * FRAGMENT + 1):
        out[f'random_{n}'] = _rand(rng, n)                   # all literals: the literal header forms, the fragment cut
    for n in (1, 3, H, 61, 64, 65, 257, FRAGMENT + 1):
        out[f'zeros_{n}'] = bytes(n)
    out['period4'] = bytes([1, 0, 0, 0]) * 5000 + b'\x07\x07'
    out['period8'] = bytes([1, 2, 3, 4, 5, 6, 7, 8]) * 3000 + b'\x01\x02\x09'
    out['int64_ramp'] = np.arange(3000, dtype=np.int64).tobytes()[:23999]
    out['period4_values'] = np.repeat(np.arange(700, dtype=np.int32), 9).tobytes()
    for length in (3, 4, 11, 12, 64, 65):                    # around MIN_MATCH, the 1-byte-offset form and the cap
        out[f'match_len_{length}'] = _planted(rng, 1000, 100, 600, length)
        out[f'match_len_{length}_near'] = _planted(rng, 1000, 592, 600, length) if length <= 8 else _planted(rng, 1000, 300, 600, length)
    for dist in (2047, 2048):                                # 40 repeats each: a slot that another position took since loses some
        a = bytearray(_rand(rng, 27000))
        for k in range(40):
            src, length = k * 600 + 50, (7, 11, 12)[k % 3]
            a[src + dist:src + dist + length] = a[src:src + length]
            if a[src + length] == a[src + dist + length]:
                a[src + dist + length] ^= 0x55
        out[f'match_dist_{dist}'] = bytes(a)
    out['match_to_fragment_end'] = _planted(rng, FRAGMENT + 300, FRAGMENT - 120, FRAGMENT - 20, 20)
    out['match_to_stream_end'] = _planted(rng, 5000, 4870, 4970, 30)
    a = bytearray(_rand(rng, FRAGMENT + 500))                # a repeat over the cut: only its two halves may match, each in its fragment
    a[FRAGMENT - 40:FRAGMENT + 40] = a[FRAGMENT - 140:FRAGMENT - 100] + a[FRAGMENT - 140:FRAGMENT - 100]
    out['repeat_straddles_cut'] = bytes(a)
    out['zeros_straddle_cut'] = _rand(rng, FRAGMENT - 100) + bytes(200) + _rand(rng, 300)
    words = [_rand(rng, int(k)) for k in rng.integers(5, 40, 50)]
    out['text_like'] = b''.join(words[i] for i in rng.integers(0, 50, 6000))[:150000]
    out.update({f'column_{k}': v for k, v in columns().items()})
    return out
