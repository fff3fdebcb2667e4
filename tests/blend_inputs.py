"""Inputs of the SPEC-BLEND tests, shared by test_blend_cpu.py and test_blend_gpu.py (drawn once per process)."""
import functools

import numpy as np

from blend_restatement import CART_WEIGHTS, CLICK_WEIGHTS

SCALE_SIZES = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 1000, 1001, 1002, 1003, 65539, 1048577)
SCALE_FAMILIES = ('normal', 'ties', 'lowdigit', 'third_nan', 'constant', 'zeros')


def scale_input(family, n):
    rng = np.random.default_rng(1000 * SCALE_FAMILIES.index(family) + n % 997)
    if family == 'normal':
        return rng.standard_normal(n) * 4.0 - 1.0
    if family == 'ties':
        return np.round(rng.standard_normal(n) * 2.0) / 2.0
    if family == 'lowdigit':
        return rng.permutation(1.0 + np.arange(n) * 2.0 ** -52)
    if family == 'third_nan':
        x = rng.lognormal(0.0, 1.5, n)
        x[rng.random(n) < 1 / 3] = np.nan
        if np.isnan(x).all():
            x[0] = 1.5
        return x
    if family == 'constant':
        return np.full(n, -2.625)
    if family == 'zeros':
        return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]), n)
    raise KeyError(family)


def _models(seed, M, n_keys, frac, n_sessions, hi_ids=False):
    """M models over a universe of n_keys distinct (session, aid) keys; each model holds about frac of them."""
    rng = np.random.default_rng(seed)
    per = max(1, -(-n_keys // n_sessions))
    k = np.arange(n_keys)
    ses, aid = (k // per).astype(np.int64) * 7 + 3, (k % per).astype(np.int64) * 3 + 1
    if hi_ids:
        ses, aid = (1 << 31) - 1 - (k // per).astype(np.int64) * 7, (1 << 31) - 1 - (k % per).astype(np.int64) * 3
    out = []
    for m in range(M):
        take = rng.permutation(n_keys)[:max(0, int(round(frac * n_keys)))] if frac < 1 else rng.permutation(n_keys)
        out.append((ses[take].astype(np.int32), aid[take].astype(np.int32), rng.standard_normal(take.size).astype(np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def join_cases():
    """name -> (models, weights, left_of_base)"""
    c = {}
    c['M1'] = (_models(1, 1, 300, 1.0, 20), (0.75,), None)
    a, b = _models(2, 2, 400, 1.0, 30)
    c['M2_disjoint'] = ([tuple(x[:200] for x in a), tuple(x[200:] for x in a)], (0.3, 0.7), None)
    c['M2_identical'] = ([a, (a[0][::-1].copy(), a[1][::-1].copy(), b[2])], (0.3, 0.7), None)
    c['M4_click'] = (_models(3, 4, 3000, 0.7, 100), CLICK_WEIGHTS, (0, 1, 0, 0))
    c['M5_cart'] = (_models(4, 5, 3000, 0.6, 100), CART_WEIGHTS, (0, 1, 0, 0, 0))
    m = _models(5, 3, 500, 0.8, 40)
    m[1] = tuple(x[:0] for x in m[1])
    c['one_empty'] = (m, (0.5, 0.25, 0.25), (0, 0, 1))
    m = _models(6, 3, 500, 0.8, 40)
    m[0] = tuple(x[:0] for x in m[0])
    c['empty_base'] = (m, (0.5, 0.25, 0.25), (0, 1, 0))
    # concatenated totals around the wave (64), the sort's tile (4096) and its workgroup span (16384); the keys of the two
    # models overlap, so equal keys of different models meet across the edge
    for tot in (1, 63, 64, 65, 257, 4095, 4096, 4097, 16383, 16384, 16385):
        m = _models(10 + tot, 2, tot, 1.0, 5)
        cut = tot // 3
        c[f'total_{tot}'] = ([tuple(x[:tot - cut] for x in m[0]), tuple(x[:cut] for x in m[1])], (0.6, 0.4), None)
    c['straddle_200001'] = (_models(7, 3, 66667, 1.0, 5000), (0.2, 0.3, 0.5), (0, 1, 0))     # every key in all 3 models
    c['one_session'] = (_models(8, 3, 2000, 0.7, 1), (0.2, 0.3, 0.5), None)
    c['single_row_sessions'] = (_models(9, 3, 2000, 0.7, 2000), (0.2, 0.3, 0.5), (0, 0, 1))
    c['ids_to_int32_max'] = (_models(10, 3, 1500, 0.7, 50, hi_ids=True), (0.2, 0.3, 0.5), None)
    c['every_digit_varies'] = (_wide_models(11, 3, 500, 10), (0.2, 0.3, 0.5), (0, 0, 1))      # no pass of the sort is a copy
    one = (np.array([12345], np.int32), np.array([678], np.int32))
    c['single_key'] = ([one + (np.array([v], np.float32),) for v in (0.5, -1.25, 2.0)], (0.2, 0.3, 0.5), None)   # every pass is a copy
    return c


def _wide_models(seed, M, n_sessions, per):
    """M models over n_sessions * per keys whose sessions and aids spread over all of [0, 2^31): every byte of the
    (session << 32 | aid) key varies. Each model holds about 0.7 of the keys."""
    rng = np.random.default_rng(seed)
    top = (1 << 31) - 1
    ses = np.unique(np.concatenate([[0, top], rng.integers(0, 1 << 31, n_sessions - 2)]))
    keys = []
    for s in ses:
        aids = np.unique(np.concatenate([[0, top], rng.integers(0, 1 << 31, per - 2)]))
        keys += [(int(s), int(a)) for a in aids]
    keys = np.array(keys, dtype=np.int64)
    out = []
    for m in range(M):
        take = rng.permutation(len(keys))[:int(round(0.7 * len(keys)))]
        out.append((keys[take, 0].astype(np.int32), keys[take, 1].astype(np.int32), rng.standard_normal(take.size).astype(np.float32)))
    return out


def key_bits(models):
    """(OR, AND) of the (session << 32 | aid) keys of all models"""
    k = np.concatenate([(m[0].astype(np.int64) << 32) | m[1].astype(np.int64) for m in models])
    return int(np.bitwise_or.reduce(k)), int(np.bitwise_and.reduce(k))


def duplicate_cases():
    """name -> (models, weights): one (session, aid) twice inside one model"""
    out = {}
    for name, (i, j) in (('adjacent', (10, 11)), ('first_and_last', (0, -1))):
        m = [tuple(x.copy() for x in t) for t in _models(20, 3, 900, 0.8, 30)]
        m[1][0][j], m[1][1][j] = m[1][0][i], m[1][1][i]
        out[name] = (m, (0.2, 0.3, 0.5))
    return out


def negative_cases():
    out = {}
    for name, col in (('session', 0), ('aid', 1)):
        m = [tuple(x.copy() for x in t) for t in _models(21, 2, 300, 0.8, 10)]
        m[1][col][17] = -1
        out[name] = (m, (0.5, 0.5))
    return out


def inf_cases():
    out = {}
    for name, v in (('plus_inf', np.inf), ('minus_inf', -np.inf)):
        x = scale_input('normal', 1001).copy()
        x[500] = v
        out[name] = x
    return out


@functools.lru_cache(maxsize=None)
def topk_case():
    """Raw (unscaled) float64 scores of 3 models: ties inside sessions (quantised scores), a session with one row,
    NaN scores in model 2."""
    rng = np.random.default_rng(33)
    m = _models(34, 3, 4000, 0.75, 60)
    out = []
    for i, (s, a, v) in enumerate(m):
        v = np.round(rng.standard_normal(v.size) * 2.0) / 2.0        # few distinct values: tied predictions
        if i == 2:
            v[::11] = np.nan
        out.append((s, a, v.astype(np.float64)))
    lone = (np.array([900000], dtype=np.int32), np.array([5], dtype=np.int32), np.array([0.5]))
    out[0] = tuple(np.concatenate([x, y]) for x, y in zip(out[0], lone))
    return out, (0.25, 0.5, 0.25), (0, 1, 0)
