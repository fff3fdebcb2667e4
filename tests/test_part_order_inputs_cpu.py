"""Every stream of ``tests/part_order_inputs.py`` has the partition-pass chunks it claims (no GPU needed): records and runs of
every aid are recomputed from the oracle's pair expansion, the chunks follow from them by the restated geometry."""
import numpy as np
import pytest

import covis_oracle as co
import part_order_inputs as pi
import reduce_inputs as ri
from test_reduce_inputs_cpu import _profile


@pytest.mark.parametrize('case', pi.SPOKE, ids=lambda c: c.name)
def test_spoke_streams_have_their_chunks(case):
    p = _profile(case)
    ev, where = p['ev'], p['where']
    n, runs = ri.records_runs(ev)
    assert np.array_equal(n, p['n']) and np.array_equal(runs, p['runs'])
    l_cap = case.option_sets[0]['l_cap']
    chunks = pi.chunks_per_aid(n, runs, l_cap)
    for t in case.targets:
        x, _ = where[t.name]
        assert (n[x], runs[x]) == (t.n, t.runs), t.name
        assert ri.kernel_of(t.n, t.runs, 2, l_cap) == t.expect['kernel'][2], t.name
        assert chunks[x] == -(-t.runs // pi.PART_CHUNK_RUNS), t.name
    print(case.name, 'chunks per aid', {int(x): int(chunks[x]) for x in np.flatnonzero(chunks)})
    assert chunks.sum() == pi.SPOKE_CHUNKS[case.name]


def test_the_cases_the_order_can_get_wrong_are_there():
    c = pi.SPOKE_CHUNKS
    two = pi.SPOKE_BY_NAME['two-aids']
    assert len(two.targets) == 2 and all(t.runs > pi.PART_CHUNK_RUNS for t in two.targets)      # two aids of at least 2 chunks
    assert c['one-chunk'] == 1
    assert c['two-aids'] % 4 and pi.GAP_CHUNKS % 4                                               # the dequeue takes 4 at a time
    assert max(c.values()) < pi.DEFAULT_Q                                                        # fewer chunks than bins ...
    assert any(o.get('part_q', pi.DEFAULT_Q) < c[s] for s, _, _, o in pi.RUNS if s in c)      # ... and more
    assert any(feeds == 2 for _, _, feeds, _ in pi.RUNS)
    assert any(kinds == pi.TIMED for _, kinds, _, _ in pi.RUNS) and any(s == 'gaps' and k == pi.TIMED for s, k, _, _ in pi.RUNS)
    dom = pi.SPOKE_BY_NAME['dominant-key']
    assert dom.min_retries == {0: 1} and dom.targets[0].counts[0][0] > ri.bucket_cap(dom.targets[0].n, 2)


def test_gap_stream_hubs_have_their_records_and_chunks():
    ev, hubs = pi.gap_stream()
    st = {}
    pairs = co.covis_pairs_numpy(ev.aid, ev.ts, ev.type, ev.sess_off, co.CovisSpec(max_gap=pi.MAX_GAP, kinds=pi.TYPE3), stats=st)
    x = pairs['click_weighted'][0].astype(np.int64)
    w1, w2, w3 = (pairs[kind][2].astype(np.int64) for kind in pi.TYPE3)
    a = (w2 - w3) // (6 * ri.Q16)                      # c + 6 a + 3 o, c + 9 a + 6 o, c + 3 a + 6 o give back c, a, o
    o = a - (w1 - w3) // (3 * ri.Q16)
    c = w1 // ri.Q16 - 6 * a - 3 * o
    n = np.bincount(x, weights=c + a + o, minlength=ev.n_aids).astype(np.int64)
    assert n.sum() == st['P']
    runs = np.zeros(ev.n_aids, dtype=np.int64)
    for name, h in hubs.items():
        shape = pi.gap_hub_shape(name)
        assert n[h] == shape['n'], name
        # a run is (component, aid): one per chain and plain session, two per cut session
        runs[h] = shape['runs']
        assert shape['private_runs'] > pi.PART_CHUNK_RUNS or name != 'hub-a'     # hub-a: its first chunk is private rows only
        assert pi.GAP_HUBS[name]['chain'] >= pi.ORD_KEY_RUNS                     # no shared list among the first 64 descriptors
    others = np.ones(ev.n_aids, dtype=bool)
    others[list(hubs.values())] = False
    assert n[others].max() <= ri.M_CAP                  # no other aid is partitioned
    chunks = pi.chunks_per_aid(n, runs, pi.LCAP)
    assert [int(chunks[hubs[h]]) for h in ('hub-a', 'hub-b')] == [4, 3] and chunks.sum() == pi.GAP_CHUNKS
