"""SPEC-DEFLATE without a GPU: the restatement (tests/deflate_restatement.py) writes valid gzip members that zlib reads
back, the inputs (tests/deflate_inputs.py) reach the paths they are named for, the size conditions hold on the
submission texts, and write_csv keeps its zlib path."""
import gzip
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_inputs as di
import deflate_restatement as dr


@pytest.mark.parametrize('name', di.CASE_NAMES)
def test_restatement_writes_members_zlib_reads(name):
    data, bb = di.case(name)
    z = di.expected(name)
    assert gzip.decompress(z) == data
    blocks = [data[lo:lo + bb] for lo in range(0, len(data), bb)] or [b'']
    pos = 0
    for block in blocks:
        assert z[pos:pos + 10] == dr.GZIP_HEADER
        d = zlib.decompressobj(-15)
        rest = z[pos + 10:]
        assert d.decompress(rest) == block and d.eof      # the stream ends where the trailer begins
        pos += 10 + len(rest) - len(d.unused_data)
        assert z[pos:pos + 4] == zlib.crc32(block).to_bytes(4, 'little')
        assert z[pos + 4:pos + 8] == len(block).to_bytes(4, 'little')
        pos += 8
    assert pos == len(z)
    assert len(z) <= dr.compressed_bound(len(data), bb)


def test_crc_and_symbol_tables():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 1000):
        x = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert dr.crc32(x) == zlib.crc32(x)
    assert dr.length_symbol(3) == (257, 0, 0) and dr.length_symbol(10) == (264, 0, 0) and dr.length_symbol(11) == (265, 1, 0)
    assert dr.length_symbol(257) == (284, 5, 30) and dr.length_symbol(258) == (285, 0, 0)
    assert dr.dist_symbol(1) == (0, 0, 0) and dr.dist_symbol(5) == (4, 1, 0) and dr.dist_symbol(32768) == (29, 13, 8191)


def test_device_helpers_on_the_host_under_sanitizers(tmp_path):
    """csrc/deflate.h (symbol arithmetic, CRC-32 and its join) through tools/deflate_host_main.cpp, a stand-alone program."""
    from conftest import ROOT
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build tools/deflate_host_main.cpp'
    exe = tmp_path / 'deflate_host_main'
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall',
                    '-I', os.path.join(ROOT, 'otto-multi-objective-recommender-system_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'deflate_host_main.cpp'), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'OK', r.stdout


def _tokens(name):
    return [t for p in di.plans(name) for t in p['tokens']]


def _matches(name):
    return [t for t in _tokens(name) if isinstance(t, tuple)]


def _runs(seq):
    out, i = [], 0
    while i < len(seq):
        r = 1
        while i + r < len(seq) and seq[i + r] == seq[i]:
            r += 1
        out.append((seq[i], r))
        i += r
    return out


def test_inputs_reach_the_paths_they_are_named_for():
    M = dr.MIN_MATCH
    one = di.plans('one-byte')[0]
    assert {d for _, d in _matches('one-byte')} == {1} and sum(1 for c in one['dd'] if c) == 1 and one['d_len'][0] == 1
    assert one['ll_len'][one['hlit'] - 1] == one['d_len'][0]             # equal lengths either side of the boundary, coded plainly
    seam = di.plans('seam-repeat')[0]                                    # a repeat token that crosses the boundary
    assert seam['dynamic'] and di.crossing_repeat(seam)
    assert seam['ll_len'][seam['hlit'] - 2:seam['hlit']] == [2, 2] and seam['d_len'][:2] == [2, 2]
    assert not any(di.crossing_repeat(p) for n in di.CASE_NAMES if n != 'seam-repeat' and len(di.case(n)[0]) < 70000 for p in di.plans(n))
    assert _matches('no-match') == [] and di.plans('no-match')[0]['hdist'] == 1 and di.plans('no-match')[0]['d_len'][0] == 0
    assert di.plans('no-match')[0]['hlit'] == 257                        # the last used symbol is end-of-block
    assert _matches('one-match') == [(10, 100)]
    fib = di.plans('fibonacci')[0]
    assert max(dr.huff_lengths(fib['ll'], 99)) > 15 and max(fib['ll_len']) == 15 and fib['hclen'] == 19
    zero_runs = {r for name in ('zero-runs-a', 'zero-runs-b') for p in di.plans(name)
                 for v, r in _runs(p['ll_len'][:p['hlit']] + p['d_len'][:p['hdist']]) if v == 0}
    assert {1, 2, 3, 10, 11, 138, 139} <= zero_runs
    rep = di.plans('repeat-runs')[0]
    assert {3, 6} <= {v + 3 for s, _, v in rep['rl'] if s == 16}
    assert any(v and r == 8 for v, r in _runs(rep['ll_len'][:rep['hlit']]))           # the first, then a repeat run of 7
    assert di.plans('top-285')[0]['hlit'] == 286 and di.plans('top-lowest-length')[0]['hlit'] == 254 + M + 1
    # HCLEN 4 needs a block without a non-zero code length and 5 one whose lengths are all 8 (256 symbols of 8 bits: never
    # smaller than stored), so 6 is the least that is ever emitted
    emitted = [p['hclen'] for n in di.CASE_NAMES if len(di.case(n)[0]) < 70000 for p in di.plans(n) if p['dynamic']]
    assert di.plans('hclen-6')[0]['dynamic'] and di.plans('hclen-6')[0]['hclen'] == 6 == min(emitted) and max(emitted) == 19
    assert di.plans('hclen-5-stored')[0]['hclen'] == 5 and not di.plans('hclen-5-stored')[0]['dynamic']
    assert _matches('len-min-1') == [] and _matches('len-min') == [(M, 1)] and _matches('len-min-far') == [(M, 64)]
    assert _matches('len-258') == [(258, 1)] and _matches('len-259') == [(258, 1)] and _matches('len-258+min') == [(258, 1), (M, 1)]
    assert _matches('match-to-end') == [(17, 70)] and isinstance(_tokens('match-to-end')[-1], tuple)
    assert (20, 32768) in _matches('dist-32768')
    assert all(d == 1 for _, d in _matches('dist-32769'))
    assert _matches('across-cut') == []
    assert {p['bits'] % 8 for p in di.plans('ragged')} == set(range(8))
    assert [len(_tokens(f'tile-{n}')) + 1 for n in (62, 63, 64, 65, 126, 127, 128, 129)] == [63, 64, 65, 66, 127, 128, 129, 130]
    for name, stored in (('stored-65535', 65535 + 5), ('stored-65536', 65536 + 10), ('stored-small', 55)):
        p = di.plans(name)[0]
        assert not p['dynamic'] and p['stored_bytes'] == stored and len(di.expected(name)) == 18 + stored
    eq = di.plans('dynamic-equals-stored')[0]
    assert eq['dynamic_bytes'] == eq['stored_bytes'] and not eq['dynamic']


def test_sizes_on_the_submission_texts():
    """zlib's own ordering first (the premise of the two conditions), then the conditions. Fractions of the input at
    3 x 700 lines: text A Huffman-only 0.470, level 1 0.491, restatement 0.424; text B Huffman-only 0.474, level 1 0.410,
    midpoint 0.442, restatement 0.349."""
    a, b = di.text_a(), di.text_b()
    a_h, a_1 = di.zlib_size(a, 6, zlib.Z_HUFFMAN_ONLY), di.zlib_size(a, 1)
    b_h, b_1, b_6 = di.zlib_size(b, 6, zlib.Z_HUFFMAN_ONLY), di.zlib_size(b, 1), di.zlib_size(b, 6)
    ours_a, ours_b = len(di.expected('text-a')), len(di.expected('text-b'))
    print(f'text A {len(a)}: huffman {a_h} level1 {a_1} ours {ours_a}; text B {len(b)}: huffman {b_h} level1 {b_1} level6 {b_6} ours {ours_b}')
    assert a_h < a_1 and b_6 < b_1 < b_h
    assert ours_a <= a_1
    assert ours_b <= (b_h + b_1) / 2


def test_bound_and_block_bytes_refusals():
    import __graft_entry__ as g
    g.build()
    from otto_amd import deflate
    for n, bb in ((0, 1), (1, 1), (65535, 65535), (65536, 65536), (65537, 65536), (10 ** 9, 4096)):
        assert deflate.compressed_bound(n, bb) == dr.compressed_bound(n, bb)
    for bad in (0, 65537, -1):
        with pytest.raises(ValueError, match='block_bytes'):
            deflate.gzip_members(None, bad)
        with pytest.raises(ValueError, match='block_bytes'):
            deflate.compressed_bound(10, bad)


def test_write_csv_zlib_path_is_unchanged(tmp_path):
    from otto_amd import submission
    text = di.text_a()[:100000]
    parts = [submission.HEADER, text[:40000], np.frombuffer(text[40000:], dtype=np.uint8)]
    want = b''.join(gzip.compress(c, compresslevel=6, mtime=0)
                    for p in parts for c in (bytes(p)[lo:lo + 30000] for lo in range(0, len(bytes(p)), 30000)))
    default, named, mixed = (str(tmp_path / f) for f in ('a.csv.gz', 'b.csv.gz', 'c.csv.gz'))
    s0 = submission.write_csv(default, parts, chunk_bytes=30000)
    s1 = submission.write_csv(named, parts, chunk_bytes=30000, compressor='zlib')
    s2 = submission.write_csv(mixed, parts, chunk_bytes=30000, compressor='device')      # host parts keep the zlib pool
    assert open(default, 'rb').read() == want == open(named, 'rb').read() == open(mixed, 'rb').read()
    assert 'device_s' not in s0 and 'device_s' not in s1 and s2['device_s'] == 0.0
    assert s0['bytes'] == s2['bytes'] == len(submission.HEADER) + len(text) and s0['file_bytes'] == len(want)
    with pytest.raises(ValueError, match='compressor'):
        submission.write_csv(str(tmp_path / 'd.csv.gz'), parts, compressor='gpu')
    with pytest.raises(ValueError, match='compressor'):
        submission.write_csv(str(tmp_path / 'e.csv'), parts, compressor='lz4')
