"""The processing order of the partition-pass chunks (options ``part_order`` / ``part_q``): every run of
tests/part_order_inputs.py (chunk counts proved by tests/test_part_order_inputs_cpu.py) is built with the chunks ordered by
record slot and with today's order by aid; both must give the oracle's rows bit for bit. A dropped or doubled chunk changes
a count, so parity is the check."""
import numpy as np
import pytest

import covis_oracle as co
import part_order_inputs as pi
import reduce_inputs as ri
from test_covis_gpu import _assert_rows_equal, _build

pytestmark = pytest.mark.gpu

_want = {}


def _stream(name):
    if name == 'gaps':
        return pi.gap_stream()[0], pi.LCAP, {}
    case = pi.SPOKE_BY_NAME[name]
    return ri.case_stream(case)[0], case.option_sets[0]['l_cap'], case.min_retries


def _oracle(name, kinds, ev):
    if (name, kinds) not in _want:
        sp = co.CovisSpec(max_gap=pi.MAX_GAP, kinds=kinds)
        _want[(name, kinds)] = co.covis_topk_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, sp, k=20)
    return _want[(name, kinds)]


@pytest.mark.parametrize('name,kinds,feeds,opts', pi.RUNS,
                         ids=[f"{s}-{'timed' if k == pi.TIMED else 'type3'}-feeds{f}-{','.join(f'{n}={v}' for n, v in o.items()) or 'defaults'}"
                              for s, k, f, o in pi.RUNS])
def test_rows_equal_oracle_and_unordered_build(gpu_device, name, kinds, feeds, opts):
    ev, l_cap, min_retries = _stream(name)
    want = _oracle(name, kinds, ev)
    rows = {}
    for order in (1, 0):
        b, rows[order] = _build(ev, gpu_device, kinds=kinds, max_gap=pi.MAX_GAP, chunks=feeds, l_cap=l_cap,
                                options={**opts, 'part_order': order})
        st = b.stats()
        names = b.kernel_names()['partition']
        print(order, {n: st[n] for n in ('items_l', 'runs_l', 'retries')}, names)
        assert 'k_partition' in names and ('k_chunk_keys' in names) == bool(order)
        if min_retries and opts.get('part_sized', 1):     # a sized bucket overflows; counted buckets hold every key at once
            assert st['retries'] >= min_retries[0]
        else:
            assert st['retries'] == 0
        _assert_rows_equal(rows[order], want, kinds)
    _assert_rows_equal(rows[1], rows[0], kinds)


def test_gap_stream_hubs_have_private_rows_ahead_of_their_shared_lists(gpu_device):
    """What the CPU proof takes from the pair-expand kernel's layout: a hub's runs are one per component, and the runs of its
    chain and cut sessions are private rows (sp = 63), so hub-a's first chunk has no shared list among its first 64 descriptors."""
    ev, hubs = pi.gap_stream()
    b, _ = _build(ev, gpu_device, kinds=pi.TYPE3, max_gap=pi.MAX_GAP, l_cap=pi.LCAP)
    _, _, run_x, run_desc = b.copy_records()
    run_x, run_desc = np.asarray(run_x), np.asarray(run_desc).astype(np.uint64)
    sp = (run_desc >> np.uint64(48)) & np.uint64(63)        # run descriptor: len | slot << 8 | sp << 48
    for name, h in hubs.items():
        shape = pi.gap_hub_shape(name)
        mine = run_x == h
        assert int(mine.sum()) == shape['runs'], name
        assert int((sp[mine] == 63).sum()) == shape['private_runs'], name
        first = np.flatnonzero(mine)[:pi.GAP_HUBS[name]['chain']]
        assert (sp[first] == 63).all(), name            # the chain sessions come first in the stream
