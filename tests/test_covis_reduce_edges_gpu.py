"""The covisitation reduce kernel at every table and list capacity: each case of tests/reduce_inputs.py (shapes proved by
tests/test_reduce_inputs_cpu.py) is built on the device with all eight kinds -- the type group, the time group and the filter
group in two passes -- and compared bit-exactly with the oracle. Where the library's statistics show the path (work items
per bin, retry rounds), the path is asserted too."""
import numpy as np
import pytest

import covis_oracle as co
import reduce_inputs as ri
from otto_amd.covisitation import spec as cs
from test_covis_gpu import _assert_rows_equal, _build

pytestmark = pytest.mark.gpu

KINDS = cs.ALL_KINDS
_pairs, _rows = {}, {}


def _want(case, k):
    """Oracle rows of a case: the pairs are expanded once per stream, the top-k once per k."""
    if (case.name, k) not in _rows:
        if case.name not in _pairs:
            ev, _ = ri.case_stream(case)
            _pairs[case.name] = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(kinds=KINDS))
        _rows[(case.name, k)] = {kind: co.topk_rows(*_pairs[case.name][kind], k=k) for kind in KINDS}
    return _rows[(case.name, k)]


def _runs():
    for case in ri.CASES:
        for oi, opts in enumerate(case.option_sets):
            for k in case.ks:
                tag = ','.join(f'{n}={v}' for n, v in opts.items()) or 'defaults'
                yield pytest.param(case, oi, k, id=f'{case.name}-{tag}-k{k}')


@pytest.mark.parametrize('case,oi,k', list(_runs()))
def test_reduce_at_its_capacities_matches_oracle(gpu_device, case, oi, k):
    """Rows of all kinds equal the oracle's (ties: smaller aid_y first). Work items per bin equal what the restated
    geometry gives for every aid of the stream. Retry rounds: none, except where a sized partition bucket must overflow --
    case `partitions`, target wide-dominant-key: 12,000 equal records fall into one of four buckets of
    bucket_cap(13000, 2) = 6756, so with part_sized = 1 at least one retry round is certain."""
    ev, where = ri.case_stream(case)
    opts = dict(case.option_sets[oi])
    l_cap = opts.pop('l_cap', None)
    want = _want(case, k)
    b, got = _build(ev, gpu_device, kinds=KINDS, k=k, l_cap=l_cap, options=opts)
    st = b.stats()
    print({name: st[name] for name in ('items_s', 'items_m', 'items_l', 'retries')})
    _assert_rows_equal(got, want, KINDS)
    for t in case.targets:
        x = where[t.name][0]
        for kind, w in t.expect.get('top_w', {}).items():
            gx, gy, gw = got[kind]
            assert int(gw[gx == x][0]) == w, f'{t.name}: best {kind} weight'
    items = ri.expected_items(ev, opts.get('packed_heavy', 2), l_cap or ri.L_CAP)
    assert (st['items_s'], st['items_m']) == (items['items_s'], items['items_m'])
    if case.min_retries.get(oi):
        assert st['retries'] >= case.min_retries[oi] and st['items_l'] >= items['items_l']
    else:
        assert st['retries'] == 0 and st['items_l'] == items['items_l']
