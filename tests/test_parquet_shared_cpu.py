"""The host pieces every Parquet reader shares (otto_amd/parquet.py): the batch planner on its edge cases, and the one page
walk on hand-built page headers at the four places where a flat leaf and a list leaf are treated differently."""
import pytest


def _planned(sizes, batch_bytes):
    """the planner's runs, after the two properties every plan must have"""
    from otto_amd import parquet
    runs = parquet._plan_batches(sizes, batch_bytes)
    assert [i for r in runs for i in r] == list(range(len(sizes)))           # every group once, in order
    assert all(r for r in runs)
    for r in runs:
        if len(r) > 1:
            assert sum(sizes[i][1] for i in r) <= batch_bytes, (r, sizes, batch_bytes)
    return runs


def test_batch_planner():
    from otto_amd import parquet
    assert _planned([], 100) == []
    assert parquet._largest_batch([], []) == (0, 0)
    sizes = [(16, 40), (32, 60), (16, 1), (48, 99)]
    assert _planned(sizes, 1) == [[0], [1], [2], [3]]                         # every group alone
    assert _planned(sizes, 100) == [[0, 1], [2, 3]]                           # 40 + 60 and 1 + 99 fit exactly
    assert _planned(sizes, 99) == [[0], [1, 2], [3]]                          # one byte less splits both
    assert _planned([(1, 40), (1, 60), (1, 1)], 100) == [[0, 1], [2]]         # one byte more than the budget splits
    assert _planned(sizes, 1 << 40) == [[0, 1, 2, 3]]
    big = [(16, 10), (16, 10), (4096, 500), (16, 10), (16, 10)]               # one group above the budget: alone, its neighbours kept out
    assert _planned(big, 100) == [[0, 1], [2], [3, 4]]
    assert _planned([(4096, 500)], 100) == [[0]]
    assert _planned([(4096, 500), (4096, 500)], 100) == [[0], [1]]
    runs = _planned(big, 100)
    assert parquet._largest_batch(big, runs) == (4096, 500)                   # stored and budget bytes of the largest batch, each on its own
    assert parquet._largest_batch([(100, 1), (1, 100)], [[0], [1]]) == (100, 100)


def _chunk_of(header, num_values=5, body=b'\0' * 8):
    from otto_amd import parquet
    buf = header + body
    return buf, parquet.Chunk('c', 2, 0, num_values, 0, len(buf), 0, None, len(buf), (0, 3))


def _v1(def_enc, rep_enc=3, n=5, body=8):
    from otto_amd.parquet_write import thrift_bytes, T_I32, T_STRUCT
    return thrift_bytes([(1, T_I32, 0), (2, T_I32, body), (3, T_I32, body),
                         (5, T_STRUCT, [(1, T_I32, n), (2, T_I32, 0), (3, T_I32, def_enc), (4, T_I32, rep_enc)])])


def _v2(num_nulls, def_len=2, rep_len=2, n=5, body=8):
    from otto_amd.parquet_write import thrift_bytes, T_I32, T_STRUCT
    return thrift_bytes([(1, T_I32, 3), (2, T_I32, body), (3, T_I32, body),
                         (8, T_STRUCT, [(1, T_I32, n), (2, T_I32, num_nulls), (3, T_I32, n - num_nulls), (4, T_I32, 0), (5, T_I32, def_len),
                                        (6, T_I32, rep_len)])])


def _leaves():
    from otto_amd import parquet
    return (parquet.Leaf('c', 2, parquet.REQUIRED, None, False), parquet.Leaf('c', 2, parquet.OPTIONAL, None, False),
            parquet.ListLeaf('c', ('c', 'list', 'element'), 2, None, True, True))


def _refused(fn):
    from otto_amd import _lib
    with pytest.raises(_lib.OttoError) as e:
        fn()
    return str(e.value)


def test_one_walk_keeps_the_four_differences_between_flat_and_list_leaves():
    from otto_amd import parquet
    required, optional, lst = _leaves()
    # V1, BIT_PACKED definition levels: a REQUIRED column has no levels to read, an OPTIONAL one and a list are refused
    buf, chunk = _chunk_of(_v1(def_enc=4))
    page, = parquet.walk_pages(buf, chunk, required, 'W')
    assert (page.page_type, page.def_len, page.rep_len, page.num_values, page.comp_size) == (parquet.DATA_PAGE, 0, 0, 5, 8)
    assert _refused(lambda: parquet.walk_pages(buf, chunk, optional, 'W')) == 'W, page 0: definition level encoding BIT_PACKED is not supported'
    assert _refused(lambda: parquet.walk_pages(buf, chunk, lst, 'W')) == 'W, page 0: definition level encoding BIT_PACKED is not supported (RLE)'
    # V1, RLE levels: def_len -1 marks the length prefix of an OPTIONAL flat column; a list page is decompressed whole
    buf, chunk = _chunk_of(_v1(def_enc=3))
    assert [parquet.walk_pages(buf, chunk, leaf, 'W')[0].def_len for leaf in (required, optional, lst)] == [0, -1, 0]
    # V1, BIT_PACKED repetition levels: only a list has them
    buf, chunk = _chunk_of(_v1(def_enc=3, rep_enc=4))
    assert parquet.walk_pages(buf, chunk, optional, 'W')[0].def_len == -1
    assert _refused(lambda: parquet.walk_pages(buf, chunk, lst, 'W')) == 'W, page 0: repetition level encoding BIT_PACKED is not supported (RLE)'
    # V2 with a null: refused in a flat column, an ordinary level entry of a list
    buf, chunk = _chunk_of(_v2(num_nulls=1))
    for leaf in (required, optional):
        assert _refused(lambda: parquet.walk_pages(buf, chunk, leaf, 'W')) == 'W, page 0: 1 null(s): nulls are not supported'
    page, = parquet.walk_pages(buf, chunk, lst, 'W')
    assert (page.page_type, page.def_len, page.rep_len, page.num_values) == (parquet.DATA_PAGE_V2, 2, 2, 5)
    # V2 level lengths past the body: a host refusal for a list only
    buf, chunk = _chunk_of(_v2(num_nulls=0, def_len=6, rep_len=3))
    assert _refused(lambda: parquet.walk_pages(buf, chunk, lst, 'W')) == 'W, page 0: level lengths run past the page body'
    assert parquet.walk_pages(buf, chunk, required, 'W')[0].def_len == 6
    # the closing count names what num_values counts
    buf, chunk = _chunk_of(_v1(def_enc=3, n=4))
    assert _refused(lambda: parquet.walk_pages(buf, chunk, required, 'W')) == 'W: the pages hold 4 values, the column chunk declares 5'
    assert _refused(lambda: parquet.walk_pages(buf, chunk, lst, 'W')) == 'W: the pages hold 4 level entries, the column chunk declares 5'
    assert not hasattr(parquet, 'walk_list_pages')
