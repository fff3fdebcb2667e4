"""Generates tests/golden/feat_golden.npz by RUNNING THE REFERENCE'S OWN SCRIPTS in this container:
``/root/reference/src/ranker/aid_feature_engineering.py`` and ``session_feature_engineering.py`` in ``validation`` mode,
through ``runpy``, over a synthetic split written to a temporary directory. ``settings`` (a hard-coded data path) is
replaced by a stand-in module that points at that directory. Only data is written to the fixture -- the input events and
the 43 columns the shipped models read, plus the three intermediates the session script reads -- no reference source.

The synthetic input (about 150 sessions, 40 aids, four ISO weeks) is built so that:
  * ts is distinct inside every session (the reference's sort_values is not stable);
  * the weeks first appear in the order 32, 34, 31, 33: neither ascending nor ending on the maximum week;
  * aid 38 is ordered only in the first week slot (0/0 changes follow and are skipped), aid 39 is carted only in the
    last slot (x/0), aid 37 has no event in the last (maximum) week, the last session holds carts only.
"""
import os
import pathlib
import runpy
import sys
import tempfile
import types
import warnings

import numpy as np
import pandas as pd

sys.dont_write_bytecode = True
warnings.filterwarnings('ignore')
REF = '/root/reference/src/ranker'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import feat_restatement as fr  # noqa: E402

T0 = 1659304800          # 2022-07-31 22:00 UTC: Monday of ISO week 31 in the reference's shifted clock
WEEK = 7 * 86400


def synth():
    rng = np.random.default_rng(20221101)
    rows = []
    first_weeks = [1, 3, 0, 2]                         # sessions 0..3 fix the order of first appearance: 32, 34, 31, 33
    for s in range(150):
        n = int(rng.integers(1, 14))
        w = first_weeks[s] if s < 4 else int(rng.integers(0, 4))
        lo = T0 + w * WEEK + int(rng.integers(0, 5 * 86400))
        span = 86400 if s < 4 else 2 * 86400           # the first four sessions stay inside their week
        ts = lo + np.sort(rng.choice(span, n, replace=False))
        for t in ts:
            rows.append([s, int(min(rng.zipf(1.4) - 1, 36)), int(t), int(rng.choice([0, 0, 0, 0, 1, 1, 2]))])
    rows[0][1], rows[0][3] = 38, 2                     # week 32 = slot 0: the only order of aid 38
    for r in rows:
        if r[0] == 3 and r[1] != 38:
            r[1], r[3] = 39, 1                         # week 33 = the last slot: the only carts of aid 39
            break
    rows.append([150, 37, T0 + 3 * 86400, 0])           # aid 37: week 31 only
    rows.append([150, 37, T0 + 3 * 86400 + 50, 1])
    rows.append([151, 5, T0 + 2 * WEEK + 1000, 1])      # a session of carts only
    rows.append([151, 6, T0 + 2 * WEEK + 1500, 1])
    df = pd.DataFrame(rows, columns=['session', 'aid', 'ts', 'type'])
    df = df.astype({'session': np.int32, 'aid': np.int32, 'ts': np.int64, 'type': np.uint8})
    assert not df.duplicated(['session', 'ts']).any()
    return df


def main():
    df = synth()
    with tempfile.TemporaryDirectory() as tmp:
        data = pathlib.Path(tmp)
        (data / 'splits').mkdir()
        sys.modules['settings'] = types.SimpleNamespace(DATA=data, MODELS=data)
        half = len(df) // 2
        df.iloc[:half].to_parquet(data / 'splits' / 'train.parquet')
        df.iloc[half:].to_parquet(data / 'splits' / 'val.parquet')
        for name in ('aid_feature_engineering', 'session_feature_engineering'):
            sys.argv = [name, 'validation']
            runpy.run_path(f'{REF}/{name}.py', run_name='__main__')
        fa = pd.read_pickle(data / 'feature_engineering' / 'train_aid_features.pkl')
        fs = pd.read_pickle(data / 'feature_engineering' / 'train_session_features.pkl')
    ev = df.sort_values(['session', 'ts']).reset_index(drop=True)
    sess_ids, counts = np.unique(ev['session'].to_numpy(), return_counts=True)
    sess_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    week = fr.calendar(ev['ts'].to_numpy())[3]
    assert fr.week_slots(week) == [32, 34, 31, 33], fr.week_slots(week)
    assert not ((ev['aid'] == 37) & (week == 34)).any()
    fa = fa.sort_values('aid').reset_index(drop=True)
    fs = fs.sort_values('session').reset_index(drop=True)
    assert np.array_equal(fs['session'].to_numpy(), sess_ids)
    out = {'aid': ev['aid'].to_numpy(np.int32), 'ts': ev['ts'].to_numpy(np.int32), 'type': ev['type'].to_numpy(np.uint8),
           'sess_off': sess_off, 'aid_ids': fa['aid'].to_numpy(np.int32),
           'aid_columns': np.stack([fa[c].to_numpy(np.float64) for c in fr.AID_COLUMNS], axis=1),
           'session_columns': np.stack([fs[c].to_numpy(np.float64) for c in fr.SESSION_COLUMNS], axis=1)}
    # float64 holds every recorded dtype (float32, float64, uint8, uint32, int64 counts) exactly
    path = os.path.join(HERE, 'feat_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(ev), 'events,', len(sess_ids), 'sessions,', len(fa), 'aids')


if __name__ == '__main__':
    main()
