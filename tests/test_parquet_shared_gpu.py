"""The staging pipeline ``read_columns`` and ``read_lists`` share (otto_amd/parquet.py), refused late: three files with
``batch_bytes=1`` make three batches, so the refusal comes from the third batch, after both staging sets were used and
while the first one is being reused. The error names the third file, ``out`` keeps its canary, and the next call on the
same device with the same ``out`` is sound."""
import os

import numpy as np
import pytest
import torch

import parquet_inputs as pi
import pqlist_inputs as I

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('damage', ['bad_index', 'null_v1'])
def test_read_columns_refused_in_the_third_batch(gpu_device, tmp_path, damage):
    from otto_amd import _lib, parquet
    good = [pi._write(tmp_path / f'good{k}.parquet', {'aid': (np.arange(n, dtype=np.int32) * (k + 3)) % 977}, data_page_size=300)[0]
            for k, n in enumerate((1000, 1000, 3000))]
    bad, page = (pi.bad_index_file if damage == 'bad_index' else pi.null_v1_file)(tmp_path)       # 3000 rows, as good[2]
    reason = "dictionary index not below the dictionary's size" if damage == 'bad_index' else 'a null'
    assert all(len(parquet.read_metadata(p).row_groups) == 1 for p in good + [bad])              # one batch per file
    out = (torch.full((5000,), -7, dtype=torch.int32, device=gpu_device),)
    with pytest.raises(_lib.OttoError) as e:
        parquet.read_columns(good[:2] + [bad], ['aid'], gpu_device, out=out, batch_bytes=1)
    assert f"{bad}: column 'aid', row group 0, page {page}: " in str(e.value) and reason in str(e.value), str(e.value)
    assert not any(os.path.basename(p) in str(e.value) for p in good)
    assert bool((out[0] == -7).all())
    got = parquet.read_columns(good, ['aid'], gpu_device, out=out, batch_bytes=1)
    assert got[0] is out[0] and np.array_equal(out[0].cpu().numpy(), pi.expected(good, ['aid'])['aid'])


@pytest.mark.parametrize('damage', ['null_element', 'value_count'])
def test_read_lists_refused_in_the_third_batch(gpu_device, tmp_path, damage):
    import pyarrow.parquet as pq
    import pqlist_restatement as R
    from otto_amd import _lib, parquet
    cases = I.cases()
    good = [I.write(tmp_path / f'{name}.parquet', cases[name][0], **cases[name][1]) for name in ('v1_page1k', 'none_v2')]
    rws, rep, dfn, vals, cuts = I.hand_case()
    good.append(I.hand_file(tmp_path / 'hand.parquet', rep, dfn, vals, cuts))                    # what the damaged copies were made from
    bad, page, code = I.damaged(tmp_path)[damage]
    reason = R.REASONS[code] if code else 'the value stream does not hold the 571 values its definition levels announce'
    assert all(len(parquet.read_list_metadata(p, I.COLUMN).row_groups) == 1 for p in good + [bad])
    want = [I.from_pylist(pq.read_table(p)[I.COLUMN].to_pylist()) for p in good]
    rows, values = sum(len(w[2]) for w in want), sum(len(w[1]) for w in want)
    out = (torch.full((rows + 1,), -3, dtype=torch.int64, device=gpu_device), torch.full((values,), -3, dtype=torch.int64, device=gpu_device),
           torch.full((rows,), 3, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(_lib.OttoError) as e:
        parquet.read_lists(good[:2] + [bad], I.COLUMN, gpu_device, out=out, batch_bytes=1)
    assert f"{bad}: column '{I.COLUMN}', row group 0, page {page}: {reason}" in str(e.value), str(e.value)
    assert not any(os.path.basename(p) in str(e.value) for p in good)
    assert all(bool((o == (-3 if o.dtype == torch.int64 else 3)).all()) for o in out)
    got = parquet.read_lists(good, I.COLUMN, gpu_device, out=out, batch_bytes=1)
    assert all(g is o for g, o in zip(got, out))
    base = np.cumsum([0] + [len(w[1]) for w in want])
    assert np.array_equal(out[0].cpu().numpy(), np.concatenate([[0]] + [w[0][1:] + b for w, b in zip(want, base)]))
    assert np.array_equal(out[1].cpu().numpy(), np.concatenate([w[1] for w in want]))
    assert np.array_equal(out[2].cpu().numpy(), np.concatenate([w[2] for w in want]))
