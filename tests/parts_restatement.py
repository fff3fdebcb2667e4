"""SPEC-ROWS (include/otto_rows.h) in NumPy and Python loops: rows -> padded top-k arrays, the refusals with the smallest
offending row and its first reason, and the inputs of tests/test_parts_gpu.py. Shares no code with the product."""
import numpy as np

AID_X, AID_Y, ORDER, RUN = 1, 2, 3, 4
REASONS = {AID_X: 'aid_x outside [0, n_aids)', AID_Y: 'aid_y outside [0, n_aids)', ORDER: "aid_x below the previous row's",
           RUN: 'a run longer than k'}


class Refused(Exception):
    def __init__(self, row, code):
        super().__init__(f'row {row}: {REASONS[code]}')
        self.row, self.code = row, code


def rows_to_topk(aid_x, aid_y, wgt, n_aids, k):
    y = np.full((n_aids, k), -1, dtype=np.int32)
    w = np.zeros((n_aids, k), dtype=np.float32)
    n = np.zeros(n_aids, dtype=np.int32)
    pos = 0
    for r in range(len(aid_x)):
        x, a = int(aid_x[r]), int(aid_y[r])
        pos = pos + 1 if r and x == int(aid_x[r - 1]) else 0
        if not 0 <= x < n_aids:
            raise Refused(r, AID_X)
        if not 0 <= a < n_aids:
            raise Refused(r, AID_Y)
        if r and x < int(aid_x[r - 1]):
            raise Refused(r, ORDER)
        if pos >= k:
            raise Refused(r, RUN)
        y[x, pos], w[x, pos], n[x] = a, wgt[r], pos + 1
    return y, w, n


def rows(lengths, n_aids, seed, aids=None):
    """rows whose runs have the given lengths, on ascending aids (``aids``, or drawn), with random aid_y and weights"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    if aids is None:
        aids = np.sort(rng.choice(n_aids, size=len(lengths), replace=False))
    aid_x = np.repeat(np.asarray(aids), lengths).astype(np.int32)
    aid_y = rng.integers(0, n_aids, size=len(aid_x)).astype(np.int32)
    wgt = (rng.integers(1, 1 << 20, size=len(aid_x)) / 65536).astype(np.float32)
    return aid_x, aid_y, wgt


def edge_lengths(k):
    """run lengths that put runs across and exactly on the 64-row boundaries, with look-backs of 1 .. k - 1 and k rows:
    runs of exactly k throughout, and fillers chosen so that some run starts on row 64, 128, ... and some run's row k - 1 (its
    last) is the first row of a wave"""
    out, at = [], 0

    def add(n):
        nonlocal at
        out.append(n)
        at += n
    add(k)                                                   # rows 0 .. k - 1
    while at % 64:                                           # single rows up to the boundary: the next run starts exactly on it
        add(1)
    add(k)                                                   # a run of k that starts on a 64-row boundary
    while (at + k - 1) % 64:                                 # the next run's last row is a wave's first: a look-back of k - 1
        add(1)
    add(k)
    for back in range(1, k):                                 # every look-back below k once
        while (at + back) % 64:
            add(1)
        add(min(k, back + 1 + (back % 3)))
    add(k)
    add(1)
    return out
