"""Every case of ``tests/cand_inputs.py`` reaches the branch of ``k_cand`` it is named after (no GPU needed).
tests/test_cand_edges_gpu.py compares the kernel with the oracle on these inputs; if an input lost its edge -- one list entry
more or less, aids that no longer collide in a hash partition, counts without a tie at the cut -- those tests would still
pass and prove nothing. The kernel's plan for a session is restated below and evaluated on the oracle's concatenation."""
from collections import Counter

import numpy as np
import pytest

import cand_oracle as cdo
import cand_inputs as ci

# Constants and rules copied from k_cand / cand_lookup in csrc/otto_cand.hip: they must follow the kernel.
VARIANT = {'short': dict(log2t=10, threads=128, digit=8), 'long': dict(log2t=12, threads=512, digit=10)}
CD_STACK = 96
RESERVED = {'short': 2560 * 16, 'long': 512 * 16}          # grid x 2 CD_DQ: sessions the workgroups reserve at launch


def geometry(variant, tot, q, same_src):
    """(table bits, log2 of the first-level partitions, select passes) from TOT, Q and the recipe's most-used source."""
    v = VARIANT[variant]
    cap = (1 << v['log2t']) // 4 * 3
    lt = min(8 if tot <= 192 else (10 if tot <= 768 else v['log2t']), v['log2t'])
    if (1 << lt) < v['threads']:
        lt = v['log2t']
    opt_from = cap if same_src >= 3 else 2 * cap
    lg0 = 0
    while (cap << lg0) < (tot if tot <= opt_from else tot // 2) and lg0 < 6:
        lg0 += 1
    width = (tot | 1).bit_length() + (q | 1).bit_length()
    return lt, lg0, -(-width // v['digit'])


def partitions(aids, lt, lg0, tot, cap):
    """(splits, longest chain of splits, most partitions stacked, partitions selected from) for the distinct aids of a
    concatenation: a partition is split when it holds more than CD_CAP distinct aids and TOT > CD_CAP."""
    h = ci.aid_hash(aids)
    stack = [(p, lg0, 0) for p in range(1 << lg0)]
    splits = depth = done = 0
    stacked = len(stack)
    while stack:
        part, lg, d = stack.pop()
        n = len(h) if lg == 0 else int((((h >> np.uint64(32 - lt - lg)) & np.uint64((1 << lg) - 1)) == np.uint64(part)).sum())
        if tot > cap and n > cap:
            splits, depth = splits + 1, max(depth, d + 1)
            stack += [(part << 1, lg + 1, d + 1), ((part << 1) | 1, lg + 1, d + 1)]
            stacked = max(stacked, len(stack))
        else:
            done += 1
    return splits, depth, stacked, done


_plans = {}


def plan(case, si=0):
    if (case.name, si) in _plans:
        return _plans[case.name, si]
    aids, types = case.sessions[si]
    variant = 'short' if len(aids) <= ci.SHORT_MAXL else 'long'
    src = ci.source_lists(aids, types)
    lens = [case.mats[kind].length(a) if a < case.n_aids else 0 for kind, s in case.recipe for a in src[s]]
    q, tot = len(lens), sum(lens)
    same_src = max(Counter(s for _, s in case.recipe).values())
    lt, lg0, passes = geometry(variant, tot, q, same_src)
    conc, unique = cdo.session_concatenation(aids, types, case.top(), case.recipe)
    assert len(conc) == tot
    counter = Counter(conc)
    cap = (1 << VARIANT[variant]['log2t']) // 4 * 3
    splits, depth, stacked, done = partitions(np.array(list(counter), dtype=np.int64), lt, lg0, tot, cap)
    longest = max(lens, default=0)
    p = dict(variant=variant, q=q, tot=tot, table=1 << lt, lg0=lg0, passes=passes, splits=splits, depth=depth, stacked=stacked,
             selected_from=done, sweeps=(longest + 31) // 32 if longest > 32 else 1, counter=counter, unique=unique, cap=cap,
             order=counter.most_common(), outside=[(a, c) for a, c in counter.most_common() if a not in set(unique)])
    _plans[case.name, si] = p
    return p


def test_plan_restated_on_its_own_edges():
    g = geometry
    assert [g('short', t, 100, 2)[0] for t in (0, 192, 193, 768, 769, 16384)] == [8, 8, 10, 10, 10, 10]
    assert [g('long', t, 100, 2)[0] for t in (1, 192, 193, 768, 769, 262144)] == [12, 12, 10, 10, 12, 12]     # 256 slots < 512 threads
    # first level: 2 terms per source start to halve past 2 CD_CAP, 3 terms per source past CD_CAP
    assert [g('short', t, 100, 2)[1] for t in (768, 769, 1536, 1537, 1538, 16384)] == [0, 1, 1, 0, 1, 4]
    assert [g('short', t, 100, 3)[1] for t in (768, 769, 1536, 1537, 1538, 16384)] == [0, 0, 0, 0, 1, 4]
    assert [g('long', t, 100, 2)[1] for t in (3072, 3073, 6144, 6145, 6146, 262144)] == [0, 1, 1, 0, 1, 6]
    assert [g('long', t, 100, 3)[1] for t in (3072, 3073, 6144, 6145, 6146, 262144)] == [0, 0, 0, 0, 1, 6]
    assert g('long', 1 << 20, 100, 3)[1] == 6
    assert [g('short', t, q, 2)[2] for t, q in ((15, 15), (16, 15), (255, 255), (256, 255), (16384, 256))] == [1, 2, 2, 3, 3]
    assert [g('long', t, q, 2)[2] for t, q in ((31, 31), (32, 31), (1023, 1023), (1024, 1023), (262144, 2047), (262144, 2048))] == [1, 2, 2, 3, 3, 4]
    rng = np.random.default_rng(0)
    assert partitions(rng.permutation(1 << 20)[:1537], 10, 0, 1537, 768)[:2] == (2, 2)
    assert partitions(rng.permutation(1 << 20)[:768], 10, 0, 769, 768)[0] == 0
    assert partitions(rng.permutation(1 << 20)[:769], 10, 0, 768, 768)[0] == 0                    # TOT <= CD_CAP never splits
    s = partitions(rng.permutation(1 << 20)[:16384], 10, 4, 16384, 768)
    assert s[0] >= 16 and s[2] <= CD_STACK
    assert partitions(rng.permutation(1 << 20)[:262144], 12, 6, 262144, 3072)[2] <= CD_STACK
    assert ci.lane_group(16, 128) == (8, 4) and ci.lane_group(17, 128) == (4, 8) and ci.lane_group(32, 128) == (4, 8)
    assert [ci.lane_group(n, 512)[0] for n in (33, 64, 65, 128, 129, 256, 257, 512)] == [8, 8, 4, 4, 2, 2, 1, 1]


# lg0 of the (a) cases, worked out by hand from the rule in k_cand: {variant: {recipe: {TOT: lg0}}}, 0 where not listed
LG0 = {'short': {'r2': {769: 1, 1536: 1, 1538: 1}, 'r3': {1538: 1}}, 'long': {'r2': {3073: 1, 6144: 1, 6146: 1}, 'r3': {6146: 1}}}
TABLE = {'short': lambda t: 256 if t <= 192 else 1024, 'long': lambda t: 1024 if 193 <= t <= 768 else 4096}


@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n.startswith('a-')])
def test_table_and_partition_cases(name):
    case = ci.case(name)
    e, p = case.expect, plan(case)
    assert p['variant'] == e['variant'] and p['tot'] == e['tot'] and p['stacked'] <= CD_STACK
    assert p['table'] == TABLE[p['variant']](p['tot'])
    if name.endswith('-max'):
        assert p['lg0'] == e['lg0'] and p['passes'] == e['passes'] and p['q'] == 8 * len(case.sessions[0][0]) and p['sweeps'] == 2
        assert p['splits'] >= e.get('min_splits', 0)
        if 'min_top_count' in e:
            assert p['order'][0][1] >= e['min_top_count'] and len(p['counter']) > 8000 and p['splits'] == 0
        return
    assert p['lg0'] == LG0[p['variant']][e['rname']].get(p['tot'], 0)
    if e['filling'] == 'distinct':
        assert len(p['counter']) == p['tot'] and ci.POISON not in p['counter']
        if p['tot'] <= p['cap']:
            assert p['splits'] == 0
        else:
            assert p['splits'] >= e['min_splits'] and p['depth'] >= e.get('min_depth', 1)
            assert (1 << p['lg0']) == e.get('first_level', 1 << p['lg0'])
    else:
        assert p['splits'] == 0
        if p['tot'] >= 192:
            counts = [c for _, c in p['order']]
            assert 50 < len(counts) <= 300 and (counts[0] >= 3 or p['tot'] < 768)
            nc = case.n_common
            assert len(counts) <= nc or counts[nc - 1] == counts[nc], 'the cut at n_common falls inside a run of equal counts'
            assert set(p['unique']) & set(p['counter']), 'own aids are counted'


def test_split_and_pass_coverage():
    """2b: in each variant the only partition splits, a first-level partition of several splits, and a child splits again;
    2f: every pass count of the select occurs."""
    for variant, all_passes in (('short', {1, 2, 3}), ('long', {1, 2, 3, 4})):
        ps = [plan(ci.case(n)) for n in ci.CASE_NAMES if n.startswith((f'a-{variant}', f'f-{variant}-passes'))]
        assert any(p['lg0'] == 0 and p['splits'] >= 1 for p in ps)
        assert any(p['lg0'] >= 1 and p['splits'] >= 1 for p in ps)
        assert any(p['depth'] >= 2 for p in ps)
        assert {p['passes'] for p in ps} == all_passes
        assert {p['table'] for p in ps} == ({256, 1024} if variant == 'short' else {1024, 4096})
        assert {1 << p['lg0'] for p in ps} >= ({1, 2, 16} if variant == 'short' else {1, 2, 64})
        assert any(p['selected_from'] >= 3 for p in ps), 'the carried list is merged more than once'
    assert plan(ci.case('a-short-max'))['splits'] >= 16


@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n.startswith('c-')])
def test_list_length_cases(name):
    case = ci.case(name)
    e = case.expect
    ps = [plan(case, si) for si in range(len(case.sessions))]
    assert {p['variant'] for p in ps} == {'short', 'long'}
    if 'k' in e:
        k = e['k']
        assert all(m.width == k for m in case.mats.values())
        seen = {n for m in case.mats.values() for _, n in m.rows.values()}
        assert seen == {-3, 0, 1, k, k + 5}
        for p, (aids, _) in zip(ps, case.sessions):
            assert e['foreign'] >= case.n_aids and e['foreign'] in aids and e['foreign'] in p['counter']
            assert e['foreign'] in [a for a, _ in p['order'][:case.n_common]], 'the foreign aid is inside the cut'
    if 'sweeps' in e:
        assert all(p['sweeps'] == e['sweeps'] for p in ps)
    if name == 'c-mixed-k':
        assert sorted(m.width for m in case.mats.values()) == [20, 33, 45, 64]
        lens = {kind: {m.length(a) for a in m.rows} for kind, m in case.mats.items()}
        assert 33 in lens['k33'] and 45 in lens['k45'] and 64 in lens['k64'] and 20 in lens['k20']
    if 'top_aid' in e:
        for p in ps:
            assert p['order'][0][0] == e['top_aid'] and p['order'][0][1] > p['order'][1][1]
            assert all(m.rows[a][0].tolist().index(e['top_aid']) == 32 for m in [case.mats['k33']] for a in m.rows)


@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n.startswith('d-')])
def test_recipe_cases(name):
    case = ci.case(name)
    srcs = [s for _, s in case.recipe]
    if name == 'd-8-terms-5-sources':
        assert len(case.recipe) == 8 and len(case.mats) == 8 and set(srcs) == {'U', 'CC', 'CO', 'LAST', 'C'}
    else:
        assert len({s for k, s in case.recipe if k == 'm0'}) == 3
    lists = [ci.source_lists(a, t) for a, t in case.sessions]
    assert any(not l['CO'] and l['C'] for l in lists) and any(not l['CC'] and not l['C'] and l['CO'] for l in lists)
    assert sum(len(a) == 1 for a, _ in case.sessions) == 3
    assert {plan(case, si)['variant'] for si in range(len(case.sessions))} == {'short', 'long'}
    assert all(plan(case, si)['tot'] > 0 for si in range(len(case.sessions)))


@pytest.mark.parametrize('variant', ['short', 'long'])
def test_session_length_cases(variant):
    case = ci.case(f'e-lengths-{variant}')
    want = ci.LEN_SHORT if variant == 'short' else ci.LEN_LONG
    assert tuple(len(a) for a, _ in case.sessions) == want
    threads = VARIANT[variant]['threads']
    assert {ci.lane_group(n, threads)[0] for n in want} == ({8, 4} if variant == 'short' else {8, 4, 2, 1})
    for aids, types in case.sessions:
        n = len(aids)
        sub, jlen = ci.lane_group(n, threads)
        if n >= 3:
            assert len(set(aids)) < n and (n < 6 or set(types) == {0, 1, 2})
        pos = {}
        for i, a in enumerate(aids):
            pos.setdefault(a, []).append(i)
        for b in {4, jlen}:                                    # a 4-event read and a lane-group boundary
            if b + 1 < n:
                # one aid on both sides of b whose flags are decided across it
                x, y = aids[b], aids[b + 1]
                assert pos[x] == [b - 1, b] and [types[i] for i in pos[x]] == [ci.T_ORDER, ci.T_CLICK]
                assert pos[y] == [b - 2, b + 1] and [types[i] for i in pos[y]] == [ci.T_CLICK, ci.T_CART]
        src = ci.source_lists(aids, types)
        if n >= 6:
            assert all(src[s] for s in ('U', 'CC', 'CO', 'C'))
    assert all(plan(case, si)['tot'] > 0 for si in range(len(case.sessions)))


@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n.startswith('f-')])
def test_selection_cases(name):
    case = ci.case(name)
    e, nc = case.expect, case.n_common
    ps = [plan(case, si) for si in range(len(case.sessions))]
    for p in ps:
        own_in = [i for i, (a, _) in enumerate(p['order']) if a in set(p['unique'])]
        if 'avail' in e:
            assert {'fewer': nc - 1, 'exact': nc}.get(e['avail'], len(p['outside'])) == len(p['outside'])
            assert (e['avail'] == 'more') == (len(p['outside']) > 2 * nc)
            assert own_in and own_in[0] < max(nc, 4), 'an own aid inside the cut'
        if e.get('tie_at_cut'):
            assert p['order'][nc - 1][1] == p['order'][nc][1] and p['outside'][nc - 1][1] == p['outside'][nc][1]
        if e.get('own_ranks'):
            assert any(i < 64 for i in own_in) and any(64 <= i < 128 for i in own_in)
        if 'count_q' in e:
            assert p['order'][0] == (e['count_q'], p['q']) and p['order'][1][1] < p['q']
        if 'passes' in e:
            assert p['variant'] == e['variant'] and p['passes'] == e['passes'] and len(p['outside']) > nc
    if 'avail' in e or 'own_ranks' in e or 'count_q' in e:
        assert {p['variant'] for p in ps} == {'short', 'long'}
    assert nc in ci.N_COMMON or 'avail' not in e


def test_selection_sizes_covered():
    assert ci.N_COMMON == (1, 63, 64, 65, 127, 128)
    for nc in ci.N_COMMON:
        for avail in ('fewer', 'exact', 'more'):
            assert f'f-nc{nc}-{avail}' in ci.CASE_NAMES
    # 'more' cases: the cut falls inside a run of equal counts for most of them, so first position decides
    tied = [nc for nc in ci.N_COMMON if nc > 1 and all(plan(ci.case(f'f-nc{nc}-more'), si)['order'][nc - 1][1] == plan(ci.case(f'f-nc{nc}-more'), si)['order'][nc][1]
                                                         for si in (0, 1))]
    assert len(tied) >= 3


def test_key_field_case():
    case = ci.case('g-high-aids')
    top, b25, b2425, b24, out_hi, out_b = case.expect['high']
    assert case.n_aids == 1 << 26 and top == (1 << 26) - 1 and all(m.width <= 2 for m in case.mats.values())
    session_aids = {a for aids, _ in case.sessions for a in aids}
    entries = {int(y) for m in case.mats.values() for a, (row, n) in m.rows.items() for y in row[:m.length(a)]}
    sources = {a for m in case.mats.values() for a in m.rows if m.length(a) > 0}
    for a in (top, b25, b2425, b24):
        assert a in session_aids and a in entries and a in sources and a & ((1 << 24) - 1) in (0, (1 << 24) - 1)
    got = set()
    for si in range(len(case.sessions)):
        p = plan(case, si)
        got |= {a for a, _ in p['outside'][:case.n_common]}
        assert set(p['unique']) & set(p['counter'])
    assert {out_hi, out_b, top} <= got, 'high aids among the candidates, 2^26 - 1 included'
    assert {plan(case, si)['variant'] for si in range(len(case.sessions))} == {'short', 'long'}


@pytest.mark.parametrize('name', [n for n in ci.CASE_NAMES if n.startswith('h-')])
def test_work_list_cases(name):
    case = ci.case(name)
    lens = np.array([len(a) for a, _ in case.sessions])
    n_short, n_long = int((lens <= 32).sum()), int((lens > 32).sum())
    assert (n_short, n_long) == (case.expect['n_short'], case.expect['n_long']) and lens.min() >= 1 and lens.max() <= 512
    assert all(m.width <= 2 for m in case.mats.values())
    if name == 'h-past-the-reserved-work':
        assert n_short == RESERVED['short'] + 1 and n_long == RESERVED['long'] + 1
        # both kinds up to the end of the call: the last work items are not all of one kind
        assert (lens[-64:] <= 32).any() and (lens[-64:] > 32).any()
    else:
        assert n_short in (1, 8, 9, 16, 17)
    assert len(set(case.template.tolist())) >= min(len(case.sessions), 6)
    assert any(len(plan(case, si)['outside']) > 0 for si in range(min(len(case.sessions), 12)))


def test_refusal_case():
    case = ci.case('i-513-events')
    lens = [len(a) for a, _ in case.sessions]
    assert lens[case.expect['too_long']] == 513 and 512 in lens and min(lens) <= 32 and lens[0] <= 512 and lens[-1] <= 512
    assert 0 < case.expect['too_long'] < len(lens) - 1


def test_every_case_is_named_and_the_oracle_is_not_degenerate():
    assert len(set(ci.CASE_NAMES)) == len(ci.CASE_NAMES)
    for name in ci.CASE_NAMES:
        case = ci.case(name)
        assert case.branch and case.modes == (False, True)
        if name.startswith('h-past') or name in ('a-short-tot0-distinct-r2', 'a-short-tot0-distinct-r3', 'a-short-tot0-overlap-r2',
                                                 'a-short-tot0-overlap-r3', 'f-nc1-fewer'):
            continue
        aids, types = case.sessions[0]
        a, c = cdo.session_candidates(aids, types, case.top(), case.recipe, case.n_common)
        a2, c2, own = cdo.session_candidates_self(aids, types, case.top(), case.recipe, case.n_common)
        assert len(a2) >= max(len(a), 1) and c == sorted(c, reverse=True) and len(own) == len(aids), name
        assert len(a) >= 1 or case.n_common == 1, name
        assert set(a) <= set(a2) or len(a2) == case.n_common


def test_self_oracle_definition():
    top = {'m': {1: [1, 7, 8], 2: [7, 1, 9]}}
    a, c, own = cdo.session_candidates_self([1, 2, 1], [0, 1, 2], top, (('m', 'U'),), n_common=2)
    assert (a, c, own) == ([7, 8], [2, 1], [2, 0, 2])
    assert cdo.session_candidates([1, 2, 1], [0, 1, 2], top, (('m', 'U'),), n_common=2) == ([7], [2])
    assert cdo.session_candidates([1, 2, 1], [0, 1, 2], top, (('m', 'C'),), n_common=5) == ([7, 8], [1, 1])


def test_prediction_case():
    case = ci.case('j-predictions')
    assert case.n_common == 64
    uniq = [len(set(a)) for a, _ in case.sessions]
    assert tuple(uniq[::2]) == ci.PRED_UNIQUE and tuple(uniq[1::2]) == ci.PRED_UNIQUE
    n_out = [len(plan(case, si)['outside']) for si in range(len(case.sessions))]
    assert all(1 <= n < 20 for n in n_out[::2]) and all(n > 64 for n in n_out[3::2])        # (one unique aid reads three lists)
