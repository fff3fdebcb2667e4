"""SPEC-SUBMIT and the most-frequent-aid kernels on the device (csrc/otto_submit.hip): device bytes equal the restatement's
exactly, at every digit count, row shape, workgroup and scan tile edge and output alignment; 64 guard bytes on either side
of the output stay untouched in every case."""
import ctypes as C
import gzip

import numpy as np
import pytest

import submit_inputs as si
import submit_restatement as sr

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 64, 0xA5


def _device_case(c, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(c['session_id']), [(t(top), t(n)) for top, n in c['tables']]


class Call:
    """One case on the device through the C-ABI: measure once, format at any first_byte into a guarded buffer."""

    def __init__(self, c, dev, interleave, session_id=None, tables=None):
        from otto_amd import _lib
        self.lib, self.dev, self.c, self.interleave = _lib, dev, c, int(interleave)
        sid, tabs = _device_case(c, dev)
        self.sid = sid if session_id is None else session_id
        self.tabs = tabs if tables is None else tables
        self.S, self.T = len(c['session_id']), len(c['tables'])
        arr = lambda i: (C.c_void_p * self.T)(*[_lib.ptr(tb[i]) if self.S else None for tb in self.tabs])
        self.head = (self.T, arr(0), arr(1), (C.c_int32 * self.T)(*c['types']), self.sid, self.S, c['k'], c['ld'], self.interleave)
        self.work_bytes = int(_lib.lib().otto_submit_workspace(self.S, self.T))
        self.work = _lib.workspace(self.work_bytes, dev)

    def measure(self):
        total = C.c_int64(-1)
        self.lib.call('otto_submit_measure', self.dev, *self.head, C.byref(total), self.work, self.work_bytes)
        return int(total.value)

    def format(self, total, residue, short=0):
        """(before, text, after) as bytes; the buffer ends ``short`` bytes early when asked to"""
        import torch
        first = GUARD + residue
        buf = torch.full((first + total + GUARD,), PATTERN, dtype=torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        out_bytes = first + total - short if short else int(buf.numel())
        try:
            self.lib.call('otto_submit_format', self.dev, *self.head, buf, out_bytes, first, self.work, self.work_bytes)
        finally:
            self.buf = buf.cpu().numpy().tobytes()
        return self.buf[:first], self.buf[first:first + total], self.buf[first + total:]


def _expect(c, interleave):
    return sr.submission_bytes(c['session_id'], c['tables'], c['types'], interleave)


def _check(c, dev, interleave, residues):
    call = Call(c, dev, interleave)
    want = _expect(c, interleave)
    total = call.measure()
    assert total == len(want)
    for r in residues:
        before, text, after = call.format(total, r)
        assert before == bytes([PATTERN]) * (GUARD + r) and after == bytes([PATTERN]) * GUARD, f'guard bytes written at residue {r}'
        assert text == want, f'residue {r}'


# every residue of first_byte where the word edges matter most, two residues (one odd) everywhere else
ALL_RESIDUES = ('digits', 'lone9', 'tile-S33', 'shape-k64-ld67-T3', 'shape-k1-ld1-T1', 'all-skipped')


@pytest.mark.parametrize('interleave', [False, True])
@pytest.mark.parametrize('name', si.CASE_NAMES)
def test_device_bytes_equal_the_restatement(gpu_device, name, interleave):
    residues = range(16) if name in ALL_RESIDUES else (0, 1 + 2 * (si.CASE_NAMES.index(name) % 7))
    _check(si.case(name), gpu_device, interleave, residues)


def test_three_workgroups_meet_in_one_word(gpu_device):
    """The lone-line case at the residues where workgroups 0, 1 and 2 own bytes of one 16-byte word (and workgroup 3 owns
    nothing): checked by the parametrised test above for every residue; here the residues are shown to exist."""
    meet = [r for r in range(16) if max(len(v) for v in si.lone_case_meetings(GUARD + r).values()) >= 3]
    assert meet
    _check(si.case('lone9'), gpu_device, False, meet)


def test_no_sessions(gpu_device):
    call = Call(si.case('no-sessions'), gpu_device, False)
    assert call.measure() == 0
    assert call.format(0, 5)[1] == b''


def _broken(gpu_device, name, interleave, edit):
    """the case with ``edit(session_id, tables)`` applied; (call, expected smallest line)"""
    c = si.case(name)
    sid = c['session_id'].copy()
    tables = [(t.copy(), n.copy()) for t, n in c['tables']]
    edit(sid, tables)
    bad = dict(c, session_id=sid, tables=tables)
    line = sr.first_violation(sid, tables, c['k'], interleave)
    assert line is not None
    return Call(bad, gpu_device, interleave), line


def _n_above_k(sid, tables):
    tables[1][1][40] = 21
    tables[2][1][50] = 64


def _negative_aid(sid, tables):
    s = [i for i in range(len(sid)) if tables[2][1][i] == 20]
    tables[2][0][s[-1], 19] = -1                             # the last aid of a full row, and an earlier row of a later table
    tables[0][0][s[1], 0] = -7


def _negative_session(sid, tables):
    sid[[12, 60]] = [-1, -(1 << 31)]


@pytest.mark.parametrize('interleave', [False, True])
@pytest.mark.parametrize('edit', [_n_above_k, _negative_aid, _negative_session])
def test_violations_name_the_smallest_line(gpu_device, edit, interleave):
    from otto_amd import _lib
    call, line = _broken(gpu_device, 'shape-k20-ld23-T3', interleave, edit)
    with pytest.raises(_lib.OttoError, match=f'otto_submit_measure: line {line}:'):
        call.measure()
    # the workspace now holds length 0 for the violating lines; the format pass finds them again and stays in bounds
    good = si.case('shape-k20-ld23-T3')
    room = len(_expect(good, interleave)) + 64
    with pytest.raises(_lib.OttoError, match=f'otto_submit_format: line {line}:'):
        call.format(room, 3)
    assert call.buf[:GUARD + 3] == bytes([PATTERN]) * (GUARD + 3) and call.buf[-GUARD:] == bytes([PATTERN]) * GUARD


def test_padding_past_n_is_not_an_error(gpu_device):
    c = si.case('shape-k20-ld23-T3')
    assert any((top[s, max(n[s], 0):] == -1).all() and n[s] < 20 for top, n in c['tables'] for s in range(len(n)))
    _check(c, gpu_device, True, (7,))


def test_out_bytes_one_short_is_refused_and_nothing_written(gpu_device):
    from otto_amd import _lib
    c = si.case('tile-S33')
    call = Call(c, gpu_device, False)
    total = call.measure()
    with pytest.raises(_lib.OttoError, match='do not fit out_bytes'):
        call.format(total, 9, short=1)
    assert call.buf == bytes([PATTERN]) * len(call.buf)
    before, text, after = call.format(total, 9)              # the same workspace, enough room
    assert text == _expect(c, False)


def test_a_foreign_workspace_is_refused_in_bounds(gpu_device):
    """Offsets measured for other inputs: -22, and the guards stay."""
    from otto_amd import _lib
    a, b = si.case('tile-S33'), si.case('shape-k20-ld20-T1')
    call = Call(a, gpu_device, False)
    total = call.measure()
    other = Call(dict(b, session_id=b['session_id'][:33], tables=[(t[:33], n[:33]) for t, n in b['tables']]), gpu_device, False)
    other.work, other.work_bytes = call.work, call.work_bytes
    with pytest.raises(_lib.OttoError, match='does not hold the offsets'):
        other.format(total, 4)
    assert other.buf[:GUARD + 4] == bytes([PATTERN]) * (GUARD + 4) and other.buf[-GUARD:] == bytes([PATTERN]) * GUARD


def test_format_rows_header_and_strided_rows(gpu_device):
    from otto_amd import submission
    c = si.case('shape-k20-ld23-T3')
    sid, tabs = _device_case(c, gpu_device)
    got = submission.format_rows(sid, [(top[:, :20], n) for top, n in tabs], c['types'], interleave=True, header=True)
    assert got.cpu().numpy().tobytes() == sr.HEADER + _expect(c, True)


# ---- most frequent aids -------------------------------------------------------------------------------------------------
def _freq_device(case, dev):
    import torch
    aid, typ, n_aids, k, _ = case
    return torch.from_numpy(aid.astype(np.int32)).to(dev), torch.from_numpy(typ).to(dev), n_aids, k


def _assert_lists(got, want):
    for row in sr.ROWS:
        assert got[row][0].tolist() == want[row][0].tolist() and got[row][1].tolist() == want[row][1].tolist(), row
        assert got[row][0].dtype == np.int32 and got[row][1].dtype == np.int64


@pytest.mark.parametrize('name', list(si.freq_cases()))
def test_frequency_lists_equal_the_restatement(gpu_device, name):
    from otto_amd import frequency
    case = si.freq_cases()[name]
    aid, typ, n_aids, k = _freq_device(case, gpu_device)
    counts, lists = frequency.most_frequent(aid, typ, n_aids, k)
    want_counts = sr.frequency_counts(case[0], case[1], n_aids)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    want = sr.frequency_lists(want_counts, k)
    _assert_lists(lists, want)
    if name == 'no-orders':
        assert len(lists['order'][0]) == 0 and len(lists['click'][0]) == k
    if name in ('distinct-few', 'n_aids-1', 'one-aid'):
        assert 0 < len(lists['all'][0]) < k
    if name == 'no-events':
        assert all(len(lists[r][0]) == 0 for r in sr.ROWS)


def test_frequency_accumulates_over_calls(gpu_device):
    from otto_amd import frequency
    case = si.freq_cases()['n_aids-65537']
    aid, typ, n_aids, k = _freq_device(case, gpu_device)
    cut = 1234
    counts, first = frequency.most_frequent(aid[:cut].contiguous(), typ[:cut].contiguous(), n_aids, k)
    counts2, both = frequency.most_frequent(aid[cut:].contiguous(), typ[cut:].contiguous(), n_aids, k, counts=counts)
    assert counts2 is counts
    _assert_lists(both, sr.frequency_lists(sr.frequency_counts(case[0], case[1], n_aids), k))
    _assert_lists(first, sr.frequency_lists(sr.frequency_counts(case[0][:cut], case[1][:cut], n_aids), k))


@pytest.mark.parametrize('what', ['aid', 'type'])
def test_frequency_refuses_out_of_range(gpu_device, what):
    import torch
    from otto_amd import _lib, frequency
    aid, typ, n_aids, k, _ = si.freq_cases()['n_aids-65']
    aid, typ = aid.copy(), typ.copy()
    if what == 'aid':
        aid[[700, 40]] = [n_aids + 5, n_aids]
    else:
        typ[[700, 40]] = [255, 3]
    with pytest.raises(_lib.OttoError, match='event 40:'):
        frequency.count_events(torch.from_numpy(aid.astype(np.int32)).to(gpu_device), torch.from_numpy(typ).to(gpu_device), n_aids)


# ---- chains --------------------------------------------------------------------------------------------------------------
def test_blend_to_submission_file(gpu_device, tmp_path):
    """blend.blend_topk on the small blend inputs -> format_rows -> write_csv (.csv.gz) equals the restatement of the same
    top lists, block by block under one header."""
    import pandas as pd
    import torch
    import blend_inputs as bi
    from otto_amd import submission
    from otto_amd.ranker import blend
    cases = bi.join_cases()
    names = ('M4_click', 'M5_cart', 'ids_to_int32_max')
    put = lambda m: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(gpu_device) for x in m)
    families = [[put(m) for m in cases[n][0]] for n in names]
    weights = [cases[n][1] for n in names]
    left = [cases[n][2] for n in names]
    path = tmp_path / 'blend_submission.csv.gz'
    stats = submission.blend_submission(path, families, weights, k=20, left_of_base_by_type=left, chunk_bytes=4096, threads=4)
    want = sr.HEADER
    for t in range(3):
        sid, top, n = (x.cpu().numpy() for x in blend.blend_topk(families[t], weights[t], left[t], k=20))
        want += sr.submission_bytes(sid, [(top, n)], [t])
    got = gzip.decompress(open(path, 'rb').read())
    assert got == want and stats['bytes'] == len(want)
    assert len(pd.read_csv(path)) == want.count(b'\n') - 1


def test_covisitation_submission_interleaves(gpu_device, tmp_path):
    import torch
    from otto_amd import submission
    c = si.case('shape-k20-ld20-T3')
    sid, tabs = _device_case(c, gpu_device)
    pred, n = torch.stack([t for t, _ in tabs]), torch.stack([n for _, n in tabs])
    submission.covisitation_submission(tmp_path / 'c.csv', sid, pred, n)
    ordered = dict(c, types=[0, 1, 2])
    assert open(tmp_path / 'c.csv', 'rb').read() == sr.HEADER + _expect(ordered, True)


def test_frequency_lists_feed_predictions(gpu_device):
    """frequency.most_frequent -> candidates.predictions equals passing the restated list by hand."""
    import torch
    import cand_inputs as ci
    from otto_amd import frequency
    from otto_amd.covisitation.candidates import candidate_lookup, predictions
    case = ci.case('j-predictions')
    aid, typ, off = case.events()
    t = lambda a: torch.from_numpy(a).to(gpu_device)
    d_aid, d_typ, d_off = t(aid.astype(np.int32)), t(typ), t(off)
    cand, _, n = candidate_lookup(d_aid, d_typ, d_off, case.device_matrices(gpu_device), case.recipe, n_common=case.n_common)
    _, lists = frequency.most_frequent(d_aid, d_typ, case.n_aids, k=20)
    want = sr.frequency_lists(sr.frequency_counts(aid, typ, case.n_aids), 20)
    for row in ('click', 'cart', 'order'):
        assert lists[row][0].tolist() == want[row][0].tolist() and len(want[row][0]) == 20
        got = predictions(d_aid, d_off, cand, n, lists[row][0], n_pred=20)
        by_hand = predictions(d_aid, d_off, cand, n, [int(a) for a in want[row][0]], n_pred=20)
        assert torch.equal(got[0], by_hand[0]) and torch.equal(got[1], by_hand[1])
        assert int((got[1] == 20).sum()) > 0
