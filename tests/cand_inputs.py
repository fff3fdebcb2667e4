"""Hand-built inputs of the candidate lookup (``k_cand`` in csrc/otto_cand.hip): matrices and sessions that do NOT come from
the covisitation builder, one named case per branch of the kernel. tests/test_cand_inputs_cpu.py proves without a GPU that
every case reaches the branch it is named after; tests/test_cand_edges_gpu.py compares the kernel with oracle/cand_oracle.py
on them, exactly (everything is an integer).

A matrix is a sparse set of rows ``aid -> (width entries, mat_n)``: only the rows the sessions read are set, every other row
has ``mat_n = 0``. A row always carries ``width`` plausible entries, so a kernel that reads past ``mat_n`` counts aids the
oracle does not (``POISON`` behind the exact-TOT lists)."""
import numpy as np

# The aid hash of k_cand (slot and partition bits). Copied from csrc/otto_cand.hip; it must follow it.
HASH = 0x9E3779B1
SHORT_MAXL, LONG_MAXL = 32, 512
POISON = 5                       # behind mat_n in the exact-TOT rows; never a list entry, never a session aid
T_CLICK, T_CART, T_ORDER = 0, 1, 2


def aid_hash(a):
    return (np.asarray(a, dtype=np.uint64) * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)


def source_lists(aids, types):
    """The five source lists of include/otto_cand.h for one session."""
    aids = [int(a) for a in aids]
    a, t = np.array(aids, dtype=np.int64), np.array(types, dtype=np.int64)
    return {'U': list(dict.fromkeys(aids[::-1])), 'CC': np.unique(a[t <= 1]).tolist(), 'CO': np.unique(a[t >= 1]).tolist(),
            'LAST': aids[-1:], 'C': np.unique(a[t == 0]).tolist()}


class Mat:
    def __init__(self, n_aids, width):
        self.n_aids, self.width, self.rows = int(n_aids), int(width), {}

    def set(self, aid, entries, mat_n):
        entries = np.asarray(entries, dtype=np.int32)
        assert entries.shape == (self.width,) and 0 <= aid < self.n_aids and aid not in self.rows
        self.rows[int(aid)] = (entries, int(mat_n))

    def length(self, aid):
        return min(max(self.rows[aid][1], 0), self.width) if aid in self.rows else 0

    def top(self):
        """What covisitation_df_to_dict would hold: aids with at least one entry."""
        return {a: y[:self.length(a)].tolist() for a, (y, n) in self.rows.items() if self.length(a) > 0}

    def device(self, dev):
        import torch
        y = torch.zeros((self.n_aids, self.width), dtype=torch.int32, device=dev)
        n = torch.zeros(self.n_aids, dtype=torch.int32, device=dev)
        if self.rows:
            idx = torch.tensor(list(self.rows), dtype=torch.int64, device=dev)
            y[idx] = torch.from_numpy(np.stack([r[0] for r in self.rows.values()])).to(dev)
            n[idx] = torch.tensor([r[1] for r in self.rows.values()], dtype=torch.int32, device=dev)
        return (y, None, n)


class Case:
    def __init__(self, name, branch, n_aids, mats, recipe, sessions, n_common=100, modes=(False, True), **expect):
        self.name, self.branch, self.n_aids, self.mats, self.recipe = name, branch, n_aids, mats, tuple(recipe)
        self.sessions = [(list(map(int, a)), list(map(int, t))) for a, t in sessions]
        self.n_common, self.modes, self.expect = n_common, modes, expect
        assert all(len(a) == len(t) for a, t in self.sessions)

    def events(self):
        aid = np.array([x for a, _ in self.sessions for x in a], dtype=np.uint32)
        typ = np.array([x for _, t in self.sessions for x in t], dtype=np.uint8)
        off = np.r_[0, np.cumsum([len(a) for a, _ in self.sessions])].astype(np.int64)
        return aid, typ, off

    def top(self):
        return {kind: m.top() for kind, m in self.mats.items()}

    def device_matrices(self, dev):
        return {kind: m.device(dev) for kind, m in self.mats.items()}


# ---- builders -----------------------------------------------------------------------------------------------------------
def _slots(recipe, sessions, n_aids):
    """(kind, source aid) of every list a session reads, in concatenation order, per session."""
    out = []
    for aids, types in sessions:
        src = source_lists(aids, types)
        out.append([(kind, a) for kind, s in recipe for a in src[s] if a < n_aids])
    return out


def _weighted_rows(rng, n_rows, pool, width, skew):
    """n_rows lists of ``width`` DISTINCT aids of ``pool``, the front of the pool more often (weights (rank + 1)^-skew):
    Gumbel top-k = sampling without replacement."""
    pool = np.asarray(pool, dtype=np.int64)
    assert width <= len(pool)
    key = rng.gumbel(size=(n_rows, len(pool))) - skew * np.log(np.arange(1, len(pool) + 1))
    if width < len(pool):
        part = np.argpartition(-key, width - 1, axis=1)[:, :width]
    else:
        part = np.tile(np.arange(len(pool)), (n_rows, 1))
    order = np.argsort(-np.take_along_axis(key, part, axis=1), axis=1)
    return pool[np.take_along_axis(part, order, axis=1)].astype(np.int32)


def _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.7, mat_n=None):
    """Every row the sessions read: ``width`` distinct aids of the pool; mat_n(kind, aid, width) or a random length."""
    for sl in _slots(recipe, sessions, n_aids):
        for kind, a in sl:
            m = mats[kind]
            if a in m.rows:
                continue
            n = int(rng.integers(0, m.width + 1)) if mat_n is None else mat_n(kind, a, m.width)
            m.set(a, _weighted_rows(rng, 1, pool, m.width, skew)[0], n)


def _fill_exact(rng, mats, recipe, session, n_aids, tot, filling, pool, skew=0.7):
    """One session whose concatenation has exactly ``tot`` entries: the lengths are dealt evenly over its lists (every matrix
    is read by one term, so a list is a row). 'distinct': the entries are ``pool[:tot]`` in order; 'overlap': weighted draws."""
    slots = _slots(recipe, [session], n_aids)[0]
    assert len(set(slots)) == len(slots), 'a row read twice cannot take two lengths'
    base, rem = divmod(tot, len(slots))
    at = 0
    for i, (kind, a) in enumerate(slots):
        m, n = mats[kind], base + (1 if i < rem else 0)
        assert n <= m.width, f'{tot} entries do not fit {len(slots)} lists of {m.width}'
        row = np.full(m.width, POISON, dtype=np.int32)
        row[:n] = pool[at:at + n] if filling == 'distinct' else _weighted_rows(rng, 1, pool, m.width, skew)[0][:n]
        at += n
        m.set(a, row, n)
    assert filling != 'distinct' or at == tot <= len(pool)


def _session(rng, n, vocab, types=(0, 1, 2)):
    """n events over the aids of ``vocab`` (every one of them at least once when n allows), random types."""
    vocab = np.asarray(vocab, dtype=np.int64)
    a = np.r_[vocab[:n], rng.choice(vocab, max(n - len(vocab), 0))]
    return rng.permutation(a).tolist(), rng.choice(np.asarray(types), n).tolist()


def _aids_with(rng, n_aids, count, exclude, keep=None):
    """``count`` distinct aids in [64, n_aids) outside ``exclude``, in random order; ``keep(hash)`` filters by hash bits."""
    a = rng.permutation(np.arange(64, n_aids, dtype=np.int64))
    a = a[~np.isin(a, np.fromiter(exclude, dtype=np.int64))]
    if keep is not None:
        a = a[keep(aid_hash(a))]
    assert len(a) >= count
    return a[:count]


# ---- a. table sizes and first-level partitions, b. splits -------------------------------------------------------------------
# most-used source read by 2 terms / by 3 terms: opt_from = 2 CD_CAP / CD_CAP
RECIPE_2 = (('m0', 'U'), ('m1', 'U'), ('m2', 'CC'), ('m3', 'CC'))
RECIPE_3 = (('m0', 'U'), ('m1', 'CC'), ('m2', 'CC'), ('m3', 'CC'))
RECIPE_MAX = (('m0', 'U'), ('m1', 'U'), ('m2', 'U'), ('m3', 'CC'), ('m4', 'CC'), ('m5', 'CC'), ('m6', 'CO'), ('m7', 'CO'))
TOT_SHORT = (0, 1, 192, 193, 768, 769, 1536, 1537, 1538)
TOT_LONG = (192, 193, 768, 769, 3072, 3073, 6144, 6145, 6146)


def _bit(lt, level, value):
    """hash filter: partition bit ``level`` (1 = the first bit below the lt slot bits) equals ``value``."""
    return lambda h: ((h >> np.uint64(32 - lt - level)) & np.uint64(1)) == np.uint64(value)


def _case_tot(variant, tot, filling, rname):
    seed = (0 if variant == 'short' else 1) * 100003 + tot * 7 + (filling == 'overlap') * 3 + (rname == 'r3')
    rng = np.random.default_rng(seed)
    n_aids = 1 << 15
    recipe = RECIPE_2 if rname == 'r2' else RECIPE_3
    own = rng.permutation(np.arange(64, n_aids))[:32 if variant == 'short' else 150]
    sess = _session(rng, 32, own, types=(0, 0, 1, 1, 1, 2)) if variant == 'short' else _session(rng, 190, own, types=(0, 0, 1, 1, 1, 2))
    mats = {f'm{i}': Mat(n_aids, 32) for i in range(4)}
    cap, lt = (768, 10) if variant == 'short' else (3072, 12)
    keep, expect, uneven = None, {}, False
    if filling == 'distinct' and tot > cap:
        # b. which partition splits is decided by the hash bits of the entries
        opt_from = 2 * cap if rname == 'r2' else cap
        lg0 = 1 if (tot if tot <= opt_from else tot // 2) > cap else 0
        uneven = lg0 == 1 and tot in (2 * cap, 2 * cap + 2)
        if tot == cap + 1 and lg0 == 0:
            keep, expect = _bit(lt, 1, 0), dict(min_splits=2, min_depth=2)          # the only partition splits, its child 0 again
        elif tot == cap + 1:
            keep, expect = _bit(lt, 1, 0), dict(min_splits=1, first_level=2)        # first level of two: every entry in partition 0
        else:
            expect = dict(min_splits=1)
    if filling == 'distinct':
        pool = _aids_with(rng, n_aids, tot, set(own.tolist()), keep)
        if uneven:
            # first level of two: partition 0 takes cap + 32 of the entries and splits, partition 1 does not
            p0 = _aids_with(rng, n_aids, cap + 32, set(own.tolist()), _bit(lt, 1, 0))
            p1 = _aids_with(rng, n_aids, tot - cap - 32, set(own.tolist()), _bit(lt, 1, 1))
            pool = rng.permutation(np.r_[p0, p1])
    else:
        pool = np.r_[own[:12], _aids_with(rng, n_aids, 288, set(own.tolist()))]
        pool = rng.permutation(pool)
    _fill_exact(rng, mats, recipe, sess, n_aids, tot, filling, pool)
    return Case(f'a-{variant}-tot{tot}-{filling}-{rname}', f'{variant} variant, TOT = {tot}, {filling} entries, recipe {rname}',
                n_aids, mats, recipe, [sess], n_common=100, variant=variant, tot=tot, filling=filling, rname=rname, **expect)


def _case_max(variant):
    rng = np.random.default_rng(77 if variant == 'short' else 78)
    if variant == 'short':
        n_aids, n_ev, tot, filling = 1 << 15, 32, 16384, 'distinct'
    else:
        n_aids, n_ev, tot, filling = 8192, 512, 262144, 'overlap'
    own = rng.permutation(np.arange(64, n_aids))[:n_ev]
    sess = (own.tolist(), [T_CART] * n_ev)                     # carts: U, CC and CO hold every aid
    mats = {f'm{i}': Mat(n_aids, 64) for i in range(8)}
    if filling == 'distinct':
        _fill_exact(rng, mats, RECIPE_MAX, sess, n_aids, tot, 'distinct', _aids_with(rng, n_aids, tot, set(own.tolist())))
        expect = dict(min_splits=16, lg0=4, passes=3)
    else:
        pool = rng.permutation(np.arange(n_aids))                # every aid of the matrices, the session's own among them
        for i in range(8):
            rows = _weighted_rows(rng, n_ev, pool, 64, 1.0)
            for a, r in zip(own.tolist(), rows):
                mats[f'm{i}'].set(a, r, 64)
        expect = dict(lg0=6, passes=4, min_top_count=1000)
    return Case(f'a-{variant}-max', f'{variant} variant, the largest concatenation ({tot} entries)', n_aids, mats, RECIPE_MAX, [sess],
                n_common=100, variant=variant, tot=tot, filling=filling, **expect)


# ---- c. list lengths -----------------------------------------------------------------------------------------------------------
def _mat_n_edges():
    """mat_n of the rows in turn: -3 (read as 0), 0, 1, k, k + 5 (clamped to k)."""
    state = {'i': 0}

    def f(kind, aid, width):
        state['i'] += 1
        return (-3, 0, 1, width, width + 5)[state['i'] % 5]
    return f


def _case_k(k):
    rng = np.random.default_rng(300 + k)
    n_aids = 1000
    own_s, own_l = np.arange(100, 120), np.arange(200, 260)
    # aid 1500 >= n_aids: no list of its own, but the lists hold it and it leaves the candidates
    sessions = [_session(rng, 24, np.r_[own_s, 1500]), _session(rng, 90, np.r_[own_l, 1500])]
    pool = np.r_[1500, own_s[:3], own_l[:3], np.arange(600, 600 + max(2 * k, 6))]
    mats = {kind: Mat(n_aids, k) for kind in ('a', 'b', 'c')}
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'), ('a', 'LAST'))
    _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.3, mat_n=_mat_n_edges())
    return Case(f'c-k{k}', f'lists of {k} entries, mat_n in (-3, 0, 1, k, k + 5), a session aid >= n_aids', n_aids, mats, recipe,
                sessions, n_common=100, k=k, foreign=1500)


def _case_mixed_k():
    rng = np.random.default_rng(345)
    n_aids = 2000
    sessions = [_session(rng, 30, np.arange(100, 118)), _session(rng, 70, np.arange(200, 240))]
    widths = {'k20': 20, 'k33': 33, 'k45': 45, 'k64': 64}
    mats = {kind: Mat(n_aids, w) for kind, w in widths.items()}
    recipe = (('k20', 'U'), ('k33', 'CC'), ('k45', 'LAST'), ('k64', 'CO'), ('k33', 'C'))
    pool = np.r_[np.arange(100, 106), np.arange(200, 206), np.arange(900, 1100)]
    full = lambda kind, aid, width: width if aid % 3 else width - 2          # most lists full: 33 = a second sweep of ONE entry
    _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.8, mat_n=full)
    return Case('c-mixed-k', 'a k = 20 matrix with mat_k = 33, 45 and 64 matrices: 2 sweeps of the gather', n_aids, mats, recipe,
                sessions, n_common=100, sweeps=2)


def _case_k33_only():
    """Only the 33rd entries of the lists hold the aid that wins: it is lost if the second sweep is."""
    rng = np.random.default_rng(346)
    n_aids = 2000
    sessions = [_session(rng, 20, np.arange(100, 112), types=(0,)), _session(rng, 50, np.arange(200, 230), types=(0,))]
    mats = {'k20': Mat(n_aids, 20), 'k33': Mat(n_aids, 33)}
    recipe = (('k20', 'U'), ('k33', 'CC'))
    pool = np.arange(900, 1100)
    _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.2, mat_n=lambda kind, aid, width: width)
    for a, (row, n) in mats['k33'].rows.items():
        row[32] = 1999
    return Case('c-k33-last-entry', 'mat_k = 33: the second sweep carries one entry per list, the most common aid', n_aids, mats, recipe,
                sessions, n_common=20, sweeps=2, top_aid=1999)


# ---- d. recipes ------------------------------------------------------------------------------------------------------------------
def _case_recipes():
    rng = np.random.default_rng(400)
    n_aids = 3000
    sessions = [_session(rng, 28, np.arange(100, 115)), _session(rng, 120, np.arange(200, 250)),
                _session(rng, 20, np.arange(300, 310), types=(0,)), _session(rng, 60, np.arange(320, 350), types=(0,)),
                _session(rng, 20, np.arange(400, 410), types=(2,)), _session(rng, 60, np.arange(420, 450), types=(2,)),
                ([500], [0]), ([501], [1]), ([502], [2])]
    out = []
    r8 = tuple((f'm{i}', s) for i, s in enumerate(('U', 'CC', 'CO', 'LAST', 'C', 'CC', 'U', 'C')))
    r3 = (('m0', 'U'), ('m0', 'CO'), ('m0', 'C'), ('m1', 'LAST'))
    for name, recipe, branch in (('d-8-terms-5-sources', r8, '8 terms over 8 matrices, all five sources'),
                                 ('d-one-matrix-3-sources', r3, 'one matrix read through three sources')):
        mats = {kind: Mat(n_aids, 12) for kind in dict.fromkeys(k for k, _ in recipe)}
        pool = np.r_[np.arange(100, 104), np.arange(200, 204), 300, 320, 400, 420, 500, 501, 502, np.arange(1000, 1150)]
        _fill_random(np.random.default_rng(401), mats, recipe, sessions, n_aids, pool, skew=0.8)
        out.append(Case(name, branch + '; clicks-only, orders-only and one-event sessions', n_aids, mats, recipe, sessions, n_common=100))
    return out


# ---- e. session lengths at the lane-group thresholds of phase A -----------------------------------------------------------------
LEN_SHORT = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32)
LEN_LONG = (33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)


def lane_group(n, threads):
    """(lanes per event, events per lane) of phase A. Copied from k_cand; it must follow it."""
    lg = 0
    while lg < 3 and (n << (lg + 1)) <= threads:
        lg += 1
    return 1 << lg, (((n + (1 << lg) - 1) >> lg) + 3) & ~3


def plant(aids, types, b, x, y):
    """Two aids around boundary b: x at b-1 (order) and b (click) -- last occurrence b, first click/cart b, first cart/order b-1,
    first click b; y at b-2 (click) and b+1 (cart) -- last occurrence b+1, first click/cart b-2, first cart/order b+1."""
    n = len(aids)
    if b - 1 >= 0 and b < n:
        aids[b - 1], types[b - 1], aids[b], types[b] = x, T_ORDER, x, T_CLICK
    if b - 2 >= 0 and b + 1 < n:
        aids[b - 2], types[b - 2], aids[b + 1], types[b + 1] = y, T_CLICK, y, T_CART


def _case_lengths(variant):
    rng = np.random.default_rng(500 + (variant == 'long'))
    n_aids = 4000
    sessions, base = [], 100
    for n in (LEN_SHORT if variant == 'short' else LEN_LONG):
        vocab = np.arange(base, base + max(n // 3, 1))
        aids, types = _session(rng, n, vocab)
        sub, jlen = lane_group(n, 128 if variant == 'short' else 512)
        for j, b in enumerate(sorted({4, jlen, 2 * jlen})):
            plant(aids, types, b, base + 300 + 2 * j, base + 301 + 2 * j)
        sessions.append((aids, types))
        base += 10
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'), ('d', 'C'), ('e', 'LAST'))
    mats = {kind: Mat(n_aids, 6) for kind in 'abcde'}
    _fill_random(rng, mats, recipe, sessions, n_aids, np.arange(2000, 2400), skew=0.0, mat_n=lambda kind, aid, width: 1 + aid % width)
    return Case(f'e-lengths-{variant}', f'{variant} variant: sessions of {LEN_SHORT if variant == "short" else LEN_LONG} events, repeated aids '
                'decided across the 4-event reads and the lane groups', n_aids, mats, recipe, sessions, n_common=100, variant=variant)


# ---- f. selection ------------------------------------------------------------------------------------------------------------------
N_COMMON = (1, 63, 64, 65, 127, 128)


def _case_select(nc, avail):
    """Candidates outside the session: nc - 1 ('fewer'), nc ('exact') or 4 nc + 40 ('more'); three own aids lead the pool and
    three trail it, so own aids sit inside the cut and far behind it."""
    rng = np.random.default_rng(600 + 10 * nc + len(avail))
    n_aids = 5000
    own_s, own_l = np.arange(100, 112), np.arange(200, 240)
    sessions = [_session(rng, 24, own_s), _session(rng, 80, own_l)]
    n_out = {'fewer': nc - 1, 'exact': nc, 'more': 4 * nc + 40}[avail]
    out = rng.permutation(np.arange(1000, 4000))[:n_out]
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'))
    width = min(16, n_out + 4)
    mats = {kind: Mat(n_aids, width) for kind in 'abc'}
    for own, sess in zip((own_s, own_l), sessions):
        pool = np.r_[own[:2], out[:40], own[2:4], out[40:]]
        if avail == 'more':
            _fill_random(rng, mats, recipe, [sess], n_aids, pool, skew=0.35, mat_n=lambda kind, aid, w: w)
            continue
        # a cyclic walk over the pool: every aid of it is in the concatenation, so the number outside the session is exact
        pool, at = rng.permutation(pool), 0
        for kind, a in _slots(recipe, [sess], n_aids)[0]:
            mats[kind].set(a, pool[(at + np.arange(width)) % len(pool)], width)
            at += width
    return Case(f'f-nc{nc}-{avail}', f'n_common = {nc} with {avail} candidates outside the session', n_aids, mats, recipe, sessions,
                n_common=nc, avail=avail, n_outside=n_out)


def _case_ranks(nc):
    """Flat counts over ~200 outside aids and 20 own aids spread over the whole order: own aids inside the top 64 and among
    ranks 65 to 128; the cut at n_common falls inside a run of equal counts."""
    rng = np.random.default_rng(650 + nc + (1000 if nc == 64 else 0))      # seeds at which both sessions tie at the cut
    n_aids = 5000
    own_s, own_l = np.arange(100, 124), np.arange(200, 260)
    sessions = [_session(rng, 32, own_s), _session(rng, 140, own_l)]
    out = rng.permutation(np.arange(1000, 4000))[:200]
    pool = rng.permutation(np.r_[own_s, own_l[:24], out])
    mats = {kind: Mat(n_aids, 20) for kind in 'abc'}
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'))
    _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.25, mat_n=lambda kind, aid, w: w)
    return Case(f'f-ranks-nc{nc}', f'n_common = {nc}: ties at the cut, own aids in the top 64 and in ranks 65 to 128', n_aids, mats, recipe,
                sessions, n_common=nc, tie_at_cut=True, own_ranks=True)


def _case_count_q():
    """Aid 4999 opens every list: its count is Q, the largest a count can be."""
    rng = np.random.default_rng(660)
    n_aids = 5000
    sessions = [_session(rng, 30, np.arange(100, 120)), _session(rng, 200, np.arange(200, 330))]
    mats = {kind: Mat(n_aids, 8) for kind in 'abcd'}
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'), ('d', 'C'), ('a', 'LAST'))
    _fill_random(rng, mats, recipe, sessions, n_aids, np.arange(1000, 1400), skew=0.3, mat_n=lambda kind, aid, w: 1 + aid % w)
    for m in mats.values():
        for row, n in m.rows.values():
            row[0] = 4999
    return Case('f-count-equals-q', 'one aid in every list: count = Q', n_aids, mats, recipe, sessions, n_common=50, count_q=4999)


def _case_passes(variant, passes):
    """The select's width bits(TOT) + bits(Q) at ``passes`` digits (8 bits short, 10 bits long)."""
    rng = np.random.default_rng(680 + 10 * (variant == 'long') + passes)
    n_aids = 1 << 15
    # (events, distinct aids, terms, k): Q = terms * distinct, TOT = Q * k
    shape = {('short', 1): (6, 3, 2, 2), ('short', 2): (20, 12, 3, 6), ('short', 3): (32, 32, 4, 16),
             ('long', 1): (40, 3, 2, 5), ('long', 2): (60, 30, 3, 10), ('long', 3): (300, 200, 4, 32)}[(variant, passes)]
    n_ev, n_own, n_terms, k = shape
    own = np.arange(100, 100 + n_own)
    sessions = [_session(rng, n_ev, own, types=(1,))]
    recipe = (('a', 'U'), ('b', 'CC'), ('c', 'CO'), ('d', 'U'))[:n_terms]
    mats = {kind: Mat(n_aids, k) for kind, _ in recipe}
    pool = np.r_[own[:2], np.arange(1000, 1000 + max(3 * k, 40))]
    _fill_random(rng, mats, recipe, sessions, n_aids, pool, skew=0.5, mat_n=lambda kind, aid, w: w)
    return Case(f'f-{variant}-passes{passes}', f'{variant} variant: radix select of {passes} pass(es)', n_aids, mats, recipe, sessions,
                n_common=3 if passes == 1 else 10, variant=variant, passes=passes)


# ---- g. key fields --------------------------------------------------------------------------------------------------------------
def _case_high_aids():
    n_aids = 1 << 26
    top, b25, b2425, b24 = n_aids - 1, 1 << 25, 3 << 24, 1 << 24
    out_hi, out_b = n_aids - 2, b25 + 1                          # candidates outside the sessions with the high bits set
    mats = {'w2': Mat(n_aids, 2), 'w1': Mat(n_aids, 1)}
    rows2 = {top: (b25, out_hi), 7: (top, out_b), b25: (out_hi, top), b2425: (out_b, out_hi), 9: (b24, b2425), b24: (out_hi, b2425)}
    rows1 = {top: (out_b,), 7: (out_hi,), b25: (b2425,), b2425: (top,), 9: (out_hi,), b24: (12,)}
    for a, r in rows2.items():
        mats['w2'].set(a, r, 2)
    for a, r in rows1.items():
        mats['w1'].set(a, r, 1)
    short = ([top, 7, b25, 7, top], [0, 1, 2, 0, 1])
    long_ = ([top, 9, b2425, b24, 7] * 8, [0, 1, 2, 1, 0] * 8)
    last = ([b2425, b24], [1, 1])
    recipe = (('w2', 'U'), ('w1', 'CC'), ('w2', 'CO'), ('w1', 'LAST'), ('w2', 'C'))
    return Case('g-high-aids', 'n_aids = 2^26: aid 2^26 - 1 and aids of high bits only as source, list entry and session aid', n_aids, mats,
                recipe, [short, long_, last], n_common=16, high=(top, b25, b2425, b24, out_hi, out_b))


# ---- h. work lists ------------------------------------------------------------------------------------------------------------------
def _templates(rng):
    short = [_session(rng, int(n), rng.permutation(np.arange(100, 140))[:max(int(n) // 2, 1)]) for n in rng.integers(1, 4, 24)]
    long_ = [_session(rng, 33 + int(n), rng.permutation(np.arange(100, 140))[:12]) for n in rng.integers(0, 3, 6)]
    return short, long_


def _case_worklist(n_short, n_long, name=None):
    """``n_short`` short and ``n_long`` long sessions interleaved, drawn from 30 templates (``template`` = index per session:
    the oracle runs once per template); lists of 2 entries."""
    rng = np.random.default_rng(800 + n_short)
    n_aids = 200
    short, long_ = _templates(rng)
    pick = np.r_[rng.integers(0, len(short), n_short), len(short) + rng.integers(0, len(long_), n_long)]
    pick = rng.permutation(pick)
    templates = short + long_
    mats = {'a': Mat(n_aids, 2), 'b': Mat(n_aids, 1)}
    recipe = (('a', 'U'), ('b', 'CC'), ('a', 'CO'))
    _fill_random(rng, mats, recipe, templates, n_aids, np.arange(100, 160), skew=0.2, mat_n=lambda kind, aid, w: w - (aid % 3 == 0))
    c = Case(name or f'h-{n_short}-sessions', f'work lists: {n_short} short and {n_long} long sessions in one call', n_aids, mats, recipe,
             [templates[i] for i in pick], n_common=8, n_short=n_short, n_long=n_long)
    c.template = pick
    return c


# ---- i. refusals -------------------------------------------------------------------------------------------------------------------
def _case_refusal():
    rng = np.random.default_rng(900)
    n_aids = 1000
    sessions = [_session(rng, 10, np.arange(100, 106)), _session(rng, 512, np.arange(200, 400)), _session(rng, 513, np.arange(200, 400)),
                _session(rng, 40, np.arange(100, 120))]
    mats = {'a': Mat(n_aids, 4)}
    recipe = (('a', 'U'), ('a', 'CC'))
    _fill_random(rng, mats, recipe, sessions, n_aids, np.r_[np.arange(100, 104), np.arange(600, 700)], skew=0.5)
    return Case('i-513-events', 'a 513-event session between valid ones is refused; 512 events are accepted', n_aids, mats, recipe,
                sessions, n_common=30, too_long=2)


# ---- j. final predictions ------------------------------------------------------------------------------------------------------
PRED_UNIQUE = (1, 19, 20, 21, 63, 64, 65)


def _case_predictions():
    """Sessions with fewer, exactly and more unique aids than n_pred = 1, 20 and 64; the first of each pair has few candidates
    (the most frequent aids fill its row), the second many."""
    rng = np.random.default_rng(950)
    n_aids = 3000
    sessions, base = [], 100
    for u in PRED_UNIQUE:
        for _ in range(2):
            sessions.append(_session(rng, u + int(rng.integers(0, 6)), np.arange(base, base + u)))
            base += u
    mats = {'a': Mat(n_aids, 10), 'b': Mat(n_aids, 10)}
    recipe = (('a', 'U'), ('b', 'CC'), ('a', 'LAST'))
    for i, sess in enumerate(sessions):
        pool = np.r_[sess[0][:2], np.arange(2000, 2012 if i % 2 == 0 else 2300)]
        _fill_random(rng, mats, recipe, [sess], n_aids, pool, skew=0.4)
    return Case('j-predictions', 'final predictions: sessions around n_pred unique aids, rows filled by the frequent aids', n_aids, mats,
                recipe, sessions, n_common=64)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _specs():
    s = {}
    for variant, tots in (('short', TOT_SHORT), ('long', TOT_LONG)):
        for tot in tots:
            for filling in ('distinct', 'overlap'):
                for rname in ('r2', 'r3'):
                    s[f'a-{variant}-tot{tot}-{filling}-{rname}'] = (_case_tot, (variant, tot, filling, rname))
        s[f'a-{variant}-max'] = (_case_max, (variant,))
    for k in (1, 8, 9, 32):
        s[f'c-k{k}'] = (_case_k, (k,))
    s['c-mixed-k'] = (_case_mixed_k, ())
    s['c-k33-last-entry'] = (_case_k33_only, ())
    for i, name in enumerate(('d-8-terms-5-sources', 'd-one-matrix-3-sources')):
        s[name] = (lambda i=i: _case_recipes()[i], ())
    for variant in ('short', 'long'):
        s[f'e-lengths-{variant}'] = (_case_lengths, (variant,))
    for nc in N_COMMON:
        for avail in ('fewer', 'exact', 'more'):
            s[f'f-nc{nc}-{avail}'] = (_case_select, (nc, avail))
    for nc in (64, 65, 128):
        s[f'f-ranks-nc{nc}'] = (_case_ranks, (nc,))
    s['f-count-equals-q'] = (_case_count_q, ())
    for variant, passes in (('short', 1), ('short', 2), ('short', 3), ('long', 1), ('long', 2), ('long', 3)):
        s[f'f-{variant}-passes{passes}'] = (_case_passes, (variant, passes))
    s['g-high-aids'] = (_case_high_aids, ())
    for n in (1, 8, 9, 16, 17):
        s[f'h-{n}-sessions'] = (_case_worklist, (n, n))
    s['h-past-the-reserved-work'] = (_case_worklist, (40961, 8193, 'h-past-the-reserved-work'))
    s['i-513-events'] = (_case_refusal, ())
    s['j-predictions'] = (_case_predictions, ())
    return s


SPECS = _specs()
CASE_NAMES = tuple(SPECS)
_built = {}


def case(name):
    if name not in _built:
        f, args = SPECS[name]
        _built[name] = f(*args)
        assert _built[name].name == name
    return _built[name]
