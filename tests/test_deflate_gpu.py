"""SPEC-DEFLATE on the device (csrc/otto_deflate.hip): for every input of tests/deflate_inputs.py the device bytes equal the
restatement's exactly, gzip reads them back to the input, 64 guard bytes on either side of the output stay untouched and
a second run gives the same bytes; then the chain format_rows -> write_csv(compressor='device') and the refusals."""
import ctypes as C
import gzip
import io
import zlib

import numpy as np
import pytest

import deflate_inputs as di
import deflate_restatement as dr

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 64, 0xA5


class Call:
    """One input on the device through the C-ABI: plan once, emit into a guarded buffer."""

    def __init__(self, text, block_bytes, dev):
        from otto_amd import _lib
        self.lib, self.dev, self.text, self.bb = _lib, dev, text, block_bytes
        self.n = int(text.numel())
        self.work_bytes = int(_lib.lib().otto_deflate_workspace(self.n, block_bytes))
        self.work = _lib.workspace(self.work_bytes, dev)

    def plan(self, work_bytes=None):
        total = C.c_int64(-1)
        self.lib.call('otto_deflate_plan', self.dev, self.text if self.n else None, self.n, self.bb, C.byref(total), self.work,
                      self.work_bytes if work_bytes is None else work_bytes)
        return int(total.value)

    def emit(self, total, short=0):
        """(before, members, after) as bytes; out_bytes is ``short`` bytes less than the members need when asked to"""
        import torch
        buf = torch.full((GUARD + total + GUARD,), PATTERN, dtype=torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        try:
            self.lib.call('otto_deflate_emit', self.dev, self.text if self.n else None, self.n, self.bb, buf[GUARD:],
                          total - short if short else total + GUARD, self.work, self.work_bytes)
        finally:
            raw = buf.cpu().numpy().tobytes()
        return raw[:GUARD], raw[GUARD:GUARD + total], raw[GUARD + total:]


def _on_device(data, dev, residue=0):
    import torch
    host = np.concatenate([np.zeros(residue, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)])
    t = torch.from_numpy(host).to(dev)
    assert t.data_ptr() % 16 == 0
    return t[residue:]


def _check(data, bb, want, dev, residue=0):
    call = Call(_on_device(data, dev, residue), bb, dev)
    total = call.plan()
    assert total == len(want)
    before, got, after = call.emit(total)
    assert before == bytes([PATTERN]) * GUARD and after == bytes([PATTERN]) * GUARD, 'guard bytes written'
    assert got == want, 'device bytes differ from the restatement'
    assert gzip.decompress(got) == data
    assert call.plan() == total
    assert call.emit(total)[1] == got, 'a second run gives other bytes'


@pytest.mark.parametrize('name', di.CASE_NAMES)
def test_device_bytes_equal_the_restatement(gpu_device, name):
    data, bb = di.case(name)
    _check(data, bb, di.expected(name), gpu_device, residue=di.CASE_NAMES.index(name) % 16)


def test_every_address_residue_of_the_input(gpu_device):
    data = di.text_a()[777:777 + 1500]
    want = dr.gzip_members(data, 512)
    for r in range(16):
        _check(data, 512, want, gpu_device, residue=r)


def test_sizes_on_the_submission_texts(gpu_device):
    """The CPU size conditions, on the device's own bytes."""
    from otto_amd import deflate
    a, b = di.text_a(), di.text_b()
    ours_a = int(deflate.gzip_members(_on_device(a, gpu_device)).numel())
    ours_b = int(deflate.gzip_members(_on_device(b, gpu_device)).numel())
    a_1 = di.zlib_size(a, 1)
    b_h, b_1 = di.zlib_size(b, 6, zlib.Z_HUFFMAN_ONLY), di.zlib_size(b, 1)
    print(f'text A {len(a)}: level1 {a_1} device {ours_a}; text B {len(b)}: huffman {b_h} level1 {b_1} device {ours_b}')
    assert ours_a <= a_1
    assert ours_b <= (b_h + b_1) / 2
    assert ours_a <= deflate.compressed_bound(len(a)) and ours_b <= deflate.compressed_bound(len(b))


def test_gzip_members_wrapper(gpu_device):
    import torch
    from otto_amd import _lib, deflate
    data, bb = di.case('ragged')
    assert deflate.gzip_members(_on_device(data, gpu_device, 3), bb).cpu().numpy().tobytes() == di.expected('ragged')
    empty = deflate.gzip_members(torch.empty(0, dtype=torch.uint8, device=gpu_device))
    assert empty.cpu().numpy().tobytes() == dr.member(b'') == di.expected('n0')
    with pytest.raises(_lib.OttoError):
        deflate.gzip_members(torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        deflate.gzip_members(torch.zeros(4, dtype=torch.int32, device=gpu_device))


@pytest.mark.parametrize('chunk_bytes', [1000, 65536, 100000, 1 << 20])
def test_chain_format_rows_to_device_gzip(gpu_device, tmp_path, chunk_bytes):
    """chunk_bytes smaller than, equal to and not a multiple of the 64 KiB member, and larger than the text"""
    import pandas as pd
    import torch
    from otto_amd import submission
    rng = np.random.default_rng(5)
    S, k = 500, 20
    sid = torch.from_numpy(np.arange(12899779, 12899779 + S, dtype=np.int32)).to(gpu_device)
    tables = [(torch.from_numpy(rng.integers(0, 1855603, (S, k), dtype=np.int32)).to(gpu_device),
               torch.from_numpy(rng.integers(0, k + 1, S, dtype=np.int32)).to(gpu_device)) for _ in range(3)]
    text = submission.format_rows(sid, tables, [0, 1, 2], interleave=True, header=True)
    plain, zipped = str(tmp_path / 'p.csv'), str(tmp_path / 'z.csv.gz')
    submission.write_csv(plain, [text])
    stats = submission.write_csv(zipped, [text, b'tail_clicks,1 2 3\n'], chunk_bytes=chunk_bytes, compressor='device')
    want = open(plain, 'rb').read() + b'tail_clicks,1 2 3\n'
    got = open(zipped, 'rb').read()
    assert gzip.decompress(got) == want
    assert stats['bytes'] == len(want) and stats['file_bytes'] == len(got) and stats['device_s'] > 0.0
    n = int(text.numel())                                    # the members of the device chunks, then zlib's of the host part
    assert got == b''.join(dr.gzip_members(want[lo:min(lo + chunk_bytes, n)]) for lo in range(0, n, chunk_bytes)) + \
        gzip.compress(b'tail_clicks,1 2 3\n', compresslevel=6, mtime=0)
    a = pd.read_csv(zipped)
    b = pd.read_csv(io.BytesIO(want))
    assert a.equals(b) and len(a) == 3 * S + 1


def test_refusals(gpu_device):
    from otto_amd import _lib
    data = di.text_a()[:5000]
    text = _on_device(data, gpu_device)
    for bad in (0, 65537):
        assert _lib.lib().otto_deflate_workspace(len(data), bad) == -1
        call = Call(text, 4096, gpu_device)
        call.bb = bad
        with pytest.raises(_lib.OttoError, match='block_bytes'):
            call.plan()
    call = Call(text, 4096, gpu_device)
    with pytest.raises(_lib.OttoError, match='workspace too small'):
        call.plan(work_bytes=call.work_bytes - 1)
    total = call.plan()
    assert total == len(dr.gzip_members(data, 4096))
    with pytest.raises(_lib.OttoError, match='do not fit'):
        call.emit(total, short=1)
    import torch
    buf = torch.full((total + GUARD,), PATTERN, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.OttoError, match='do not fit'):
        _lib.call('otto_deflate_emit', gpu_device, text, len(data), 4096, buf, total - 1, call.work, call.work_bytes)
    assert buf.cpu().numpy().tobytes() == bytes([PATTERN]) * (total + GUARD), 'a refused call wrote'
    call.work_bytes -= 1
    with pytest.raises(_lib.OttoError, match='workspace too small'):
        call.emit(total)
