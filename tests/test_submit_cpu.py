"""SPEC-SUBMIT and the most-frequent-aid lists without a GPU: the restatement against pandas (the reference's row
expression + ``to_csv``, its ``groupby`` / ``sort_values`` / ``head`` / ``to_dict`` + ``json.dump``), and the host side of
``submission.write_csv``."""
import gzip
import io
import json

import numpy as np
import pandas as pd
import pytest

import submit_inputs as si
import submit_restatement as sr


def _frame_csv(c, interleave):
    """the reference's frame: one dict per line, session_type and labels as strings"""
    rows = []
    for s, t in sr.line_order(len(c['session_id']), len(c['tables']), interleave):
        top, n = c['tables'][t]
        if n[s] < 0:
            continue
        rows.append({'session_type': str(int(c['session_id'][s])) + '_' + ('clicks', 'carts', 'orders')[c['types'][t]],
                     'labels': ' '.join([str(int(a)) for a in top[s, :n[s]]])})
    df = pd.DataFrame(rows, columns=['session_type', 'labels'])
    return df.to_csv(index=False).encode()


@pytest.mark.parametrize('interleave', [False, True])
@pytest.mark.parametrize('name', si.CASE_NAMES)
def test_restatement_equals_pandas_to_csv(name, interleave):
    c = si.case(name)
    assert sr.first_violation(c['session_id'], c['tables'], c['k'], interleave) is None
    got = sr.submission_bytes(c['session_id'], c['tables'], c['types'], interleave, header=True)
    assert got == _frame_csv(c, interleave)


def test_inputs_cover_the_digit_counts_and_the_row_shapes():
    c = si.case('digits')
    text = sr.submission_bytes(c['session_id'], c['tables'], c['types']).decode()
    for v in si.VALUES:
        assert f'\n{v}_carts,{v} ' in '\n' + text and f' {v} ' in text and f' {v}\n' in text
    seen = set()
    for name in si.CASE_NAMES:
        if name.startswith('shape-'):
            c = si.case(name)
            for _, n in c['tables']:
                seen |= {(c['k'], int(v)) for v in n}
    for k in (1, 20, 64):
        assert {(k, 0), (k, 1), (k, k - 1), (k, k), (k, -1)} <= seen
    assert sr.submission_bytes(**{k: v for k, v in si.case('lone9').items() if k in ('session_id', 'tables', 'types')}) == b'0_carts,\n' * 5
    assert sr.submission_bytes(si.case('no-sessions')['session_id'], si.case('no-sessions')['tables'], [0, 1, 2]) == b''


def test_violations_are_found_at_the_smallest_line():
    c = si.case('shape-k20-ld23-T3')
    sid = c['session_id'].copy()
    tables = [(t.copy(), n.copy()) for t, n in c['tables']]
    assert sr.first_violation(sid, tables, 20) is None
    tables[1][1][7] = 21                                     # n > k in table 1, session 7
    assert sr.first_violation(sid, tables, 20) == len(sid) + 7 and sr.first_violation(sid, tables, 20, True) == 7 * 3 + 1
    tables[0][0][3, 0] = -5                                  # session 3 of table 0 has n = 20: aid 0 is inside
    assert tables[0][1][3] == 20 and sr.first_violation(sid, tables, 20) == 3


def _pandas_lists(aid, typ, k):
    df = pd.DataFrame({'aid': aid.astype(np.int64), 'type': typ.astype(np.int64)})
    out = {}
    for name, frame in (('all', df), ('click', df[df['type'] == 0]), ('cart', df[df['type'] == 1]), ('order', df[df['type'] == 2])):
        counts = frame.groupby('aid')[['aid']].count().rename(columns={'aid': 'count'}).reset_index()
        counts = counts.sort_values(by='count', ascending=False)
        out[name] = counts.set_index('aid').head(k).to_dict()['count']
    return out


@pytest.mark.parametrize('name', [n for n, c in si.freq_cases().items() if c[4]])
def test_frequency_restatement_equals_pandas(name):
    aid, typ, n_aids, k, _ = si.freq_cases()[name]
    lists = sr.frequency_lists(sr.frequency_counts(aid, typ, n_aids), k)
    want = _pandas_lists(aid, typ, k)
    for row in sr.ROWS:
        buf = io.StringIO()
        json.dump(want[row], buf, indent=2)
        assert sr.frequency_json(*lists[row]) == buf.getvalue().encode(), row
        assert [int(a) for a in json.loads(buf.getvalue()).keys()] == lists[row][0].tolist()


def test_frequency_ties_go_by_ascending_aid():
    aid, typ, n_aids, k, _ = si.freq_cases()['ties']
    lists = sr.frequency_lists(sr.frequency_counts(aid, typ, n_aids), k)
    assert lists['click'][0].tolist() == list(range(250, 263)) + list(range(1020, 1027))
    assert lists['click'][1].tolist() == [3] * 20
    assert lists['all'][0].tolist() == [5, 300] + list(range(250, 263)) + list(range(1020, 1025))
    assert lists['cart'][0].tolist() == [5, 300] and lists['order'][0].tolist() == []


def test_write_json_names_and_bytes(tmp_path):
    from otto_amd import frequency
    aid, typ, n_aids, k, _ = si.freq_cases()['distinct-40']
    lists = sr.frequency_lists(sr.frequency_counts(aid, typ, n_aids), k)
    paths = frequency.write_json(tmp_path / 'aid_frequencies', 'test', lists)
    names = ['test_20_most_frequent_aids.json'] + [f'test_20_most_frequent_{t}_aids.json' for t in ('click', 'cart', 'order')]
    assert [p.split('/')[-1] for p in paths] == names
    for p, row in zip(paths, sr.ROWS):
        assert open(p, 'rb').read() == sr.frequency_json(*lists[row])
        assert [int(a) for a in json.load(open(p)).keys()] == lists[row][0].tolist()        # what the consumers read


def _parts():
    c = si.case('shape-k20-ld20-T3')
    text = sr.submission_bytes(c['session_id'], c['tables'], c['types'], True)
    cut = len(text) // 3
    return [sr.HEADER, text[:cut], np.frombuffer(text[cut:2 * cut], dtype=np.uint8), bytearray(text[2 * cut:]), b''], sr.HEADER + text


@pytest.mark.parametrize('chunk_bytes', [1, 7, 1 << 20])
@pytest.mark.parametrize('suffix', ['.csv', '.csv.gz'])
def test_write_csv_from_host_parts(tmp_path, suffix, chunk_bytes):
    from otto_amd import submission
    parts, whole = _parts()
    if chunk_bytes == 1:                                     # one gzip member per byte: a short file is enough
        whole = whole[:whole.index(b'\n', 300) + 1]
        parts = [whole]
    a, b = tmp_path / ('a' + suffix), tmp_path / ('b' + suffix)
    stats = submission.write_csv(a, parts, chunk_bytes=chunk_bytes, threads=3)
    submission.write_csv(b, parts, chunk_bytes=chunk_bytes, threads=40)
    raw = open(a, 'rb').read()
    assert raw == open(b, 'rb').read()                       # two runs, two pool sizes: identical files
    assert stats['bytes'] == len(whole) and stats['file_bytes'] == len(raw)
    assert (gzip.decompress(raw) if suffix == '.csv.gz' else raw) == whole
    if suffix == '.csv.gz':
        assert raw.count(b'\x1f\x8b\x08') >= -(-len(whole) // chunk_bytes)      # one member per chunk
    df = pd.read_csv(a)
    want = pd.read_csv(io.BytesIO(whole))
    assert list(df.columns) == ['session_type', 'labels'] and df.equals(want) and len(df) == whole.count(b'\n') - 1


def test_write_csv_empty_and_refusals(tmp_path):
    from otto_amd import submission
    submission.write_csv(tmp_path / 'e.csv.gz', [])
    assert gzip.decompress(open(tmp_path / 'e.csv.gz', 'rb').read()) == b''
    with pytest.raises(ValueError):
        submission.write_csv(tmp_path / 'x.csv', [b'a'], chunk_bytes=0)


def test_format_rows_refuses_host_tensors():
    import torch
    from otto_amd import _lib, submission
    with pytest.raises(_lib.OttoError, match='no CPU fallback'):
        submission.format_rows(torch.zeros(3, dtype=torch.int32), [(torch.zeros((3, 2), dtype=torch.int32), torch.zeros(3, dtype=torch.int32))], [0])
