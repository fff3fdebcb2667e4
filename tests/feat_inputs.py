"""Seeded event sets for the feature-table tests (tests/test_feat_cpu.py, tests/test_feat_gpu.py)."""
import numpy as np

SUNDAY = 1659304800 - 86400      # 2022-07-30 22:00 UTC: a Sunday 00:00 in the reference's clock (ts + 2 h), ISO week 30


def events(aid_counts, n_days, seed, long_session=0, n_aids=None, max_len=20):
    """Events whose aid a occurs exactly aid_counts[a] times, cut into sessions of 1 .. max_len events (the first one of
    ``long_session`` events when given), every session inside [SUNDAY, SUNDAY + n_days days), ts distinct per session.
    Returns aid int32, ts int32, type uint8, sess_off int64, n_aids."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(np.repeat(np.arange(len(aid_counts)), aid_counts))
    lengths = [long_session] if long_session else []
    left = len(pool) - sum(lengths)
    while left > 0:
        n = min(int(rng.integers(1, max_len + 1)), left)
        lengths.append(n)
        left -= n
    off = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    ts = np.empty(len(pool), dtype=np.int64)
    for s, n in enumerate(lengths):
        span = 2 if n_days >= 2 and n > 1 else 1
        day = int(rng.integers(0, n_days - span + 1))
        ts[off[s]:off[s + 1]] = SUNDAY + day * 86400 + np.sort(rng.choice(span * 86400, n, replace=False))
    typ = rng.choice(3, len(pool), p=[0.8, 0.15, 0.05]).astype(np.uint8)
    return pool.astype(np.int32), ts.astype(np.int32), typ, off, int(n_aids or len(aid_counts))


def edge_events():
    """Aid segments of 1, 63, 64, 65, 1,025 and 4,097 events, 71 aids of which 12 are absent, tied small counts, one
    session of 512 events and sessions of one, 64 days = 10 ISO weeks."""
    rng = np.random.default_rng(5)
    counts = [1, 63, 64, 65, 1025, 4097] + [0, 0] + rng.integers(1, 6, 51).tolist() + [0] * 10 + [2, 2]
    return events(counts, 64, seed=6, long_session=512)


def same(a, b):
    """Bit-equal, with any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def ulps(a, b):
    """Largest distance in float32 steps over the entries that are numbers in both; NaN must match NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    if not ok.any():
        return 0
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return int(np.abs(key(a[ok]) - key(b[ok])).max())
