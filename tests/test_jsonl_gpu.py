"""The JSONL kernels of csrc/otto_jsonl.hip through ``otto_amd.jsonl`` and ``events.jsonl_to_events_device`` against the
restatement of SPEC-JSONL (``jsonl_restatement``): sizes next to the tile, a tile boundary and the end of the halo on
every byte of a header and an event, a line over several tiles, more tiles than one scan block takes, the limits of every
field, every violation class with its line number, the mutation corpus (``test_jsonl_cpu.py`` runs the same corpora through
the same piece parsers under the sanitizers on the host), chunked reading and the pickle script. Integers only: every
comparison is exact."""
import re

import numpy as np
import pytest

import jsonl_inputs as ji
import jsonl_restatement as jr

pytestmark = pytest.mark.gpu
NAMES = ('session', 'aid', 'ts', 'type', 'sess_off', 'sess_id')


def _dev_bytes(dev, buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev) if len(buf) else torch.empty(0, dtype=torch.uint8, device=dev)


def _parse(dev, buf, line0=0):
    from otto_amd import jsonl
    out = jsonl.parse_bytes(_dev_bytes(dev, buf), line0)
    return {k: t.cpu().numpy() for k, t in zip(NAMES, out)}


def _check(dev, buf, what, line0=0):
    want = jr.parse(buf, line0)
    got = _parse(dev, buf, line0)
    for k in NAMES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(want[k].dtype), want[k]), (what, k)
    return got


def _refused(dev, buf, line, what, line0s=(0, 10 ** 6)):
    from otto_amd import _lib
    for line0 in line0s:
        assert jr.verdict(buf, line0)[0] == line0 + line, what
        with pytest.raises(_lib.OttoError, match=rf'line {line0 + line}:'):
            _parse(dev, buf, line0)


def test_sizes_next_to_the_tile(gpu_device):
    from otto_amd import jsonl
    T = jsonl.TILE_BYTES
    acc = ji.acceptance_corpus()
    for name in ('empty', 'one_line', 'no_last_newline', 'blank_only', 'blank_between'):
        _check(gpu_device, acc[name], name)
    got = _check(gpu_device, b'', 'empty')
    assert got['sess_off'].tolist() == [0] and got['aid'].size == 0
    for n in (T - 1, T, T + 1, 2 * T, 15, 16, 17):
        buf = ji.exact_size(n) if n > 100 else b'\n' * n
        assert len(buf) == n
        _check(gpu_device, buf, n)
        _check(gpu_device, buf[:-1], n - 1)                  # the same without the last newline


def test_unaligned_and_strided_input(gpu_device):
    from otto_amd import jsonl
    buf = ji.buffer(ji.sessions(2, 50))
    want = jr.parse(buf)
    d = _dev_bytes(gpu_device, b'\n\n\n' + buf)
    for view in (d[3:], d[1:], _dev_bytes(gpu_device, bytes(b for c in buf for b in (c, 0)))[::2]):
        got = jsonl.parse_bytes(view)
        for k, t in zip(NAMES, got):
            assert np.array_equal(t.cpu().numpy().view(want[k].dtype), want[k]), k


def test_tile_boundary_on_every_byte_of_header_and_event(gpu_device):
    from otto_amd import jsonl
    T = jsonl.TILE_BYTES
    for k in range(96):
        buf = ji.slide(k, T - 96)
        assert buf[T - 96 + k:T - 96 + k + 1] == b'{'
        _check(gpu_device, buf, ('slide', k))


def test_halo_end_on_every_byte_of_a_longest_piece(gpu_device):
    from otto_amd import jsonl
    T = jsonl.TILE_BYTES
    for j in range(96):
        _check(gpu_device, ji.halo_slide(j, T), ('halo', j))
    for j in (0, 1, 40):                                         # one byte more: refused, where the halo ends too
        buf = ji.halo_slide(j, T, piece=257)
        _refused(gpu_device, buf, buf[:T].count(b'\n') + 1, ('halo 257', j))
    for base in (T, 2 * T):                                      # the slide of a plain line across the end of the halo
        for k in range(0, 96, 3):
            _check(gpu_device, ji.slide(k, base + jsonl.MAX_PIECE - 96), ('halo slide', base, k))


def test_one_line_over_several_tiles(gpu_device):
    from otto_amd import jsonl
    buf = ji.long_line(500)
    assert len(buf) > 5 * jsonl.TILE_BYTES
    got = _check(gpu_device, ji.GOOD + buf + ji.GOOD, 'long line')
    assert got['sess_off'].tolist() == [0, 2, 502, 504]


def test_more_tiles_than_one_scan_block(gpu_device):
    """4,300 tiles: above the 1,024 values one block of ``k_scan_partials`` takes per round and above the 4,096 one block
    of ``device_scan`` takes, so the per-tile counts go through every kernel of the scan. The buffer repeats one block of
    an odd length, so the tiles cut it at ever different bytes; the expectation is the block's, tiled."""
    from otto_amd import jsonl
    block = ji.buffer(ji.sessions(21, 400), orders=ji.KEY_ORDERS) + b' \r\n'
    assert len(block) % 2 == 1
    reps = 4300 * jsonl.TILE_BYTES // len(block) + 1
    one = jr.parse(block)
    S, E = len(one['sess_id']), len(one['aid'])
    got = _parse(gpu_device, block * reps)
    for k in ('session', 'aid', 'ts', 'type', 'sess_id'):
        assert np.array_equal(got[k].view(one[k].dtype), np.tile(one[k], reps)), k
    off = (one['sess_off'][:-1][None, :] + E * np.arange(reps)[:, None]).ravel()
    assert np.array_equal(got['sess_off'], np.r_[off, E * reps]) and len(got['sess_id']) == S * reps


@pytest.mark.parametrize('name', sorted(ji.acceptance_corpus()))
def test_limits_key_orders_ws_variants_and_empty_sessions(gpu_device, name):
    got = _check(gpu_device, ji.acceptance_corpus()[name], name)
    if name == 'limits':
        assert got['sess_id'].view(np.uint32).tolist() == [0, 4294967295]
        assert got['aid'].view(np.uint32).tolist() == [0, 4294967295, 5, 4294967295]
        assert got['ts'].tolist() == [0, 1659304800025, 9223372036854775807, 0] and got['type'].tolist() == [0, 1, 2, 2]
    if name == 'empty_events':
        assert (np.diff(got['sess_off']) == 0).sum() == 3 and np.diff(got['sess_off'])[[0, -1]].tolist() == [0, 0]


@pytest.mark.parametrize('name', sorted(ji.BAD_LINES))
def test_every_violation_class_is_refused_with_its_line(gpu_device, name):
    for where in (1, 101, 201):
        _refused(gpu_device, ji.with_bad_line(ji.BAD_LINES[name], where), where, (name, where))


def test_line_cut_at_every_byte_of_its_last_event(gpu_device):
    for i, buf in enumerate(ji.truncations()):
        _refused(gpu_device, buf, 4, ('cut', i))


def test_smallest_violating_line_wins(gpu_device):
    from otto_amd import jsonl
    lines = [ji.GOOD] * 300                                     # violations in several tiles: the first one is named
    for w in (290, 57, 130):
        lines[w - 1] = ji.BAD_LINES['type_string'] + b'\n'
    buf = b''.join(lines)
    assert len(buf) > 4 * jsonl.TILE_BYTES
    _refused(gpu_device, buf, 57, 'three bad lines')
    buf, line = ji.many_pieces_bad()                            # behind tiles whose piece lists take several rounds
    _refused(gpu_device, buf, line, 'many pieces')
    _refused(gpu_device, b'{' * 5000 + b'\n' + ji.GOOD, 1, 'braces only')


def test_capacities_and_arguments(gpu_device):
    """A capacity below the count is refused and nothing is written past it; an unaligned pointer and a short workspace are
    refused on the host."""
    import ctypes as C
    import torch
    from otto_amd import _lib
    dev = gpu_device
    buf = ji.buffer(ji.sessions(4, 40))
    want = jr.parse(buf)
    S, E = len(want['sess_id']), len(want['aid'])
    d = _dev_bytes(dev, b'\n' + buf)
    lib = _lib.lib()
    wb = int(lib.otto_jsonl_workspace(len(buf) + 1))
    work = _lib.workspace(wb, dev)
    counts = (C.c_int64 * 2)()
    _lib.call('otto_jsonl_count', dev, d, len(buf) + 1, counts, work, wb)
    assert list(counts) == [S, E]

    def run(cap_s, cap_e, data=d, n=len(buf) + 1, wbytes=wb):
        cols = [torch.full((E + 8,), 249 if dt == torch.uint8 else -7, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]
        off = torch.full((S + 9,), -7, dtype=torch.int64, device=dev)
        sid = torch.full((S + 8,), -7, dtype=torch.int32, device=dev)
        try:
            _lib.call('otto_jsonl_parse', dev, data, n, 0, cap_s, cap_e, *cols, off, sid, counts, work, wbytes)
        finally:
            torch.cuda.synchronize(dev)
            assert all(bool((c[cap_e:] == (249 if c.dtype == torch.uint8 else -7)).all()) for c in cols)
            assert bool((off[cap_s + 1:] == -7).all()) and bool((sid[cap_s:] == -7).all())
        return cols, off, sid
    cols, off, sid = run(S, E)
    assert np.array_equal(cols[1][:E].cpu().numpy().view(np.uint32), want['aid']) and np.array_equal(off[:S + 1].cpu().numpy(), want['sess_off'])
    with pytest.raises(_lib.OttoError, match=f'{S} sessions, cap_sessions is {S - 1}'):
        run(S - 1, E)
    with pytest.raises(_lib.OttoError, match=f'{E} events, cap_events is {E - 5}'):
        run(S, E - 5)
    with pytest.raises(_lib.OttoError, match='16-byte aligned'):
        run(S, E, data=d[1:], n=len(buf))
    with pytest.raises(_lib.OttoError, match='workspace too small'):
        run(S, E, wbytes=wb - 1)
    with pytest.raises(_lib.OttoError, match=r'n_bytes must be in \[0, 2\^31\)'):
        run(S, E, n=1 << 31)


def test_mutation_corpus(gpu_device):
    """One substituted, deleted or inserted byte in each of 300 buffers: the verdict and the line number are the
    restatement's, and where the buffer is still valid so are the arrays."""
    from otto_amd import _lib
    n_ok = 0
    for i, buf in enumerate(ji.mutation_corpus()):
        line, want = jr.verdict(buf, 500)
        if line is None:
            _check(gpu_device, buf, ('mutation', i), 500)
            n_ok += 1
        else:
            with pytest.raises(_lib.OttoError, match=rf'line {line}:'):
                _parse(gpu_device, buf, 500)
    assert 20 < n_ok < 150


def _events_equal(a, b):
    import torch
    for k in ('aid', 'ts', 'type', 'sess_off', 'session_ids', 'order'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and bool(torch.equal(x, y)), k
    assert a.n_aids == b.n_aids


def test_chunked_files_equal_the_frame_path_and_the_script(gpu_device, tmp_path, monkeypatch):
    import pandas as pd
    from otto_amd import events
    from otto_amd.utilities import dataset_writer_pickle as dw
    rng = np.random.default_rng(5)
    sess = ji.sessions(31, 400, max_events=20)
    sess = [sess[i] for i in rng.permutation(len(sess))]             # unsorted session ids: the sort has work to do
    train = ji.line(4_000_000, []) + ji.buffer(sess[:300]) + b'\n' + ji.buffer(sess[300:], 'crlf', last_newline=False)
    test = ji.buffer(ji.sessions(32, 80, first=1000), 'dumps', orders=ji.KEY_ORDERS)
    (tmp_path / 'train.jsonl').write_bytes(train)
    (tmp_path / 'test.jsonl').write_bytes(test)
    assert len(train) > 2 * (64 << 10)
    longest = max(len(ln) for ln in train.split(b'\n')) + 1
    want = events.frame_to_events_device(jr.frame(train), gpu_device)
    assert want.n_events == len(jr.parse(train)['aid'])
    for chunk in (longest + 1, 64 << 10, 256 << 20):
        _events_equal(events.jsonl_to_events_device(tmp_path / 'train.jsonl', gpu_device, chunk_bytes=chunk), want)
    with pytest.raises(ValueError, match='a line longer than chunk_bytes'):
        events.jsonl_to_events_device(tmp_path / 'train.jsonl', gpu_device, chunk_bytes=longest - 2)
    both = events.jsonl_to_events_device([tmp_path / 'train.jsonl', tmp_path / 'test.jsonl'], gpu_device, chunk_bytes=64 << 10)
    _events_equal(both, events.frame_to_events_device(jr.frame([train, test]), gpu_device))
    _events_equal(events.jsonl_to_events_device([str(tmp_path / 'test.jsonl')], gpu_device, n_aids=2_000_000, ts_unit='ms'),
                  events.frame_to_events_device(jr.frame(test), gpu_device, n_aids=2_000_000, ts_unit='ms'))
    # a violation in the second chunk of the second file names the line of that file
    from otto_amd import _lib
    bad = test.split(b'\n')
    bad[61] = bad[61].replace(b'"ts"', b'"tz"', 1)
    (tmp_path / 'bad.jsonl').write_bytes(b'\n'.join(bad))
    with pytest.raises(_lib.OttoError, match=r'line 62:'):
        events.jsonl_to_events_device([tmp_path / 'train.jsonl', tmp_path / 'bad.jsonl'], gpu_device, chunk_bytes=4096)
    # the script: pickles with the reference's frame
    monkeypatch.setattr(dw.settings, 'DATA', tmp_path)
    dw.main()
    for name, raw in (('train', train), ('test', test)):
        pd.testing.assert_frame_equal(pd.read_pickle(tmp_path / f'{name}.pkl'), jr.frame(raw))
