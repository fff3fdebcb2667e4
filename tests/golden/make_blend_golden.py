"""Writes blend_golden.npz: what scikit-learn's RobustScaler and a pandas left / outer / outer merge compute on small
inputs, so that GPU tests can compare against them where neither library is installed.

    python tests/golden/make_blend_golden.py        (needs scikit-learn and pandas)

scale_<i>_x float64 input, _center / _scale the fitted center_ / scale_, _out the transformed column as float32.
join_m<m>_{session,aid,score}: four models; model 1 is left-joined onto model 0, models 2 and 3 are outer-joined;
join_out_{session,aid} the merged key set in (session, aid) order, join_out_cols float32 [4, R] the zero-filled columns.
"""
import os

import numpy as np
import pandas as pd
from sklearn.preprocessing import RobustScaler

HERE = os.path.dirname(os.path.abspath(__file__))


def scale_inputs():
    rng = np.random.default_rng(20240917)
    xs = []
    for n in (1, 2, 3, 4, 5, 8, 9, 64, 65, 1000, 1001, 1002, 1003):
        xs.append(rng.standard_normal(n) * 3.0 - 0.5)
    xs.append(np.round(rng.standard_normal(1001) * 2.0) / 2.0)                 # heavy ties
    x = rng.lognormal(0.0, 1.5, 1002)
    x[rng.random(1002) < 1 / 3] = np.nan                                        # a third NaN
    xs.append(x)
    xs.append(np.full(257, 0.375))                                              # constant: scale_ becomes 1.0
    xs.append(rng.permutation(1.0 + np.arange(1003) * 2.0 ** -52))              # differ in the lowest digit only
    xs.append(rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), 1000))               # mixed zeros
    return xs


def join_inputs():
    rng = np.random.default_rng(7)
    models = []
    for m, n in enumerate((300, 260, 340, 200)):
        key = rng.choice(40 * 64, n, replace=False)
        models.append(((key // 64).astype(np.int32) * 3 + 1, (key % 64).astype(np.int32) * 5, rng.standard_normal(n).astype(np.float32)))
    return models


def main():
    out = {}
    xs = scale_inputs()
    out['n_scale'] = np.int64(len(xs))
    for i, x in enumerate(xs):
        sc = RobustScaler()
        y = sc.fit_transform(x.reshape(-1, 1).copy())
        out[f'scale_{i}_x'] = x
        out[f'scale_{i}_center'] = np.float64(sc.center_[0])
        out[f'scale_{i}_scale'] = np.float64(sc.scale_[0])
        out[f'scale_{i}_out'] = y[:, 0].astype(np.float32)
    models = join_inputs()
    frames = []
    for m, (s, a, v) in enumerate(models):
        out[f'join_m{m}_session'], out[f'join_m{m}_aid'], out[f'join_m{m}_score'] = s, a, v
        frames.append(pd.DataFrame({'session': s, 'aid': a, f'p{m}': v}))
    df = frames[0].merge(frames[1], how='left', on=['session', 'aid'])
    df = df.merge(frames[2], how='outer', on=['session', 'aid']).merge(frames[3], how='outer', on=['session', 'aid'])
    df = df.fillna(0).sort_values(['session', 'aid']).reset_index(drop=True)
    out['join_out_session'] = df['session'].to_numpy().astype(np.int64)
    out['join_out_aid'] = df['aid'].to_numpy().astype(np.int64)
    out['join_out_cols'] = np.stack([df[f'p{m}'].to_numpy().astype(np.float32) for m in range(4)])
    np.savez_compressed(os.path.join(HERE, 'blend_golden.npz'), **out)


if __name__ == '__main__':
    main()
