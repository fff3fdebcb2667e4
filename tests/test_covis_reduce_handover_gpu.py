"""The hand-over between two work items of one workgroup of the covisitation reduce kernel: each case of
tests/reduce_handover_inputs.py (shapes proved by tests/test_reduce_handover_inputs_cpu.py) puts at most 8 items into a
multi-wave kernel, so ONE workgroup runs them all in order, and is built with all eight kinds and compared bit-exactly with
the oracle for k = 20 and k = 32."""
import pytest

import covis_oracle as co
import reduce_handover_inputs as hi
import reduce_inputs as ri
from otto_amd.covisitation import spec as cs
from test_covis_gpu import _assert_rows_equal, _build

pytestmark = pytest.mark.gpu

KINDS = cs.ALL_KINDS
_pairs, _rows = {}, {}


def _want(case, k):
    if (case.name, k) not in _rows:
        if case.name not in _pairs:
            ev, _ = ri.case_stream(case)
            _pairs[case.name] = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(kinds=KINDS))
        _rows[(case.name, k)] = {kind: co.topk_rows(*_pairs[case.name][kind], k=k) for kind in KINDS}
    return _rows[(case.name, k)]


def _runs():
    for case in hi.CASES:
        for oi, opts in enumerate(case.option_sets):
            for k in case.ks:
                yield pytest.param(case, oi, k, id=f"{case.name}-{','.join(f'{n}={v}' for n, v in opts.items()) or 'defaults'}-k{k}")


@pytest.mark.parametrize('case,oi,k', list(_runs()))
def test_items_handed_over_inside_one_workgroup_match_oracle(gpu_device, case, oi, k):
    """Rows of all kinds equal the oracle's. Work items per bin equal the restated geometry's; retry rounds: none, except in
    case handover-ovf, whose first item holds more keys than its table has slots."""
    ev, _ = ri.case_stream(case)
    opts = dict(case.option_sets[oi])
    l_cap = opts.pop('l_cap', None)
    b, got = _build(ev, gpu_device, kinds=KINDS, k=k, l_cap=l_cap, options=opts)
    st = b.stats()
    print({name: st[name] for name in ('items_s', 'items_m', 'items_l', 'retries')})
    _assert_rows_equal(got, _want(case, k), KINDS)
    items = ri.expected_items(ev, opts.get('packed_heavy', 2), l_cap or ri.L_CAP)
    assert (st['items_s'], st['items_m']) == (items['items_s'], items['items_m'])
    if case.min_retries.get(oi):
        assert st['retries'] >= case.min_retries[oi] and st['items_l'] >= items['items_l']
    else:
        assert st['retries'] == 0 and st['items_l'] == items['items_l']
