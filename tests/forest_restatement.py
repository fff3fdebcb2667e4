"""Plain NumPy float64 restatement of SPEC-FOREST (include/otto_forest.h) for the tests.

It works on the unpacked arrays of a ``Forest`` and on the float64 thresholds of the model file: it never sees the
float32 thresholds of the packed image. Everything the device computes is exact, so the tests compare bit for bit.
"""
import numpy as np

ZERO_THRESHOLD = np.float32(1e-35)


def validate(forest, max_leaves=None, max_features=None):
    """The structural rules of ``otto_forest_pack``; raises ValueError naming the tree."""
    F = forest.n_features
    if max_features is not None and not 1 <= F <= max_features:
        raise ValueError(f'F = {F}')
    for t in range(forest.n_trees):
        n0, l0 = int(forest.node_off[t]), int(forest.leaf_off[t])
        L = int(forest.leaf_off[t + 1]) - l0
        nint = int(forest.node_off[t + 1]) - n0
        if L < 1 or nint != L - 1 or (max_leaves is not None and L > max_leaves):
            raise ValueError(f'tree {t}: {L} leaves, {nint} nodes')
        if not np.isfinite(forest.leaf_value[l0:l0 + L]).all():
            raise ValueError(f'tree {t}: non-finite leaf')
        dt = forest.decision_type[n0:n0 + nint].astype(np.int64) & 0xFF
        if (dt & 1).any() or (((dt >> 2) & 3) == 3).any() or (dt >> 4).any():
            raise ValueError(f'tree {t}: decision_type')
        sf = forest.split_feature[n0:n0 + nint]
        if ((sf < 0) | (sf >= F)).any():
            raise ValueError(f'tree {t}: split_feature')
        if np.isnan(forest.threshold[n0:n0 + nint]).any():
            raise ValueError(f'tree {t}: NaN threshold')
        seen_node, seen_leaf = np.zeros(nint, dtype=np.int64), np.zeros(L, dtype=np.int64)
        if nint == 0:
            seen_leaf[0] = 1
            continue
        seen_node[0] = 1
        for side in (forest.left_child, forest.right_child):
            c = side[n0:n0 + nint].astype(np.int64)
            if (c >= nint).any() or (~c[c < 0] >= L).any():
                raise ValueError(f'tree {t}: child outside the tree')
            np.add.at(seen_node, c[c >= 0], 1)
            np.add.at(seen_leaf, ~c[c < 0], 1)
        # every node and leaf is the child of exactly one node (the root of none): with L - 1 nodes and L leaves this
        # leaves no room for a cycle only if all of them hang off the root, which the walk below confirms
        if (seen_node != 1).any() or (seen_leaf != 1).any():
            raise ValueError(f'tree {t}: a node or a leaf is not reached exactly once')
        reached, stack = 0, [0]
        while stack:
            i = stack.pop()
            reached += 1
            for side in (forest.left_child, forest.right_child):
                c = int(side[n0 + i])
                if c >= 0:
                    stack.append(c)
        if reached != nint:
            raise ValueError(f'tree {t}: a cycle beside the root')


def leaves(forest, X):
    """The reached leaf of every (row, tree), int32 [n_rows, T]; X float32 [n_rows, >= F]."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and X.ndim == 2
    n = X.shape[0]
    out = np.zeros((n, forest.n_trees), dtype=np.int32)
    rows = np.arange(n)
    for t in range(forest.n_trees):
        n0 = int(forest.node_off[t])
        nint = int(forest.node_off[t + 1]) - n0
        if nint == 0:
            continue
        sf = forest.split_feature[n0:n0 + nint].astype(np.int64)
        thr = forest.threshold[n0:n0 + nint]
        dt = forest.decision_type[n0:n0 + nint].astype(np.int64) & 0xFF
        lc = forest.left_child[n0:n0 + nint].astype(np.int64)
        rc = forest.right_child[n0:n0 + nint].astype(np.int64)
        cur = np.zeros(n, dtype=np.int64)
        for _ in range(nint):
            act = rows[cur >= 0]
            if act.size == 0:
                break
            c = cur[act]
            x = X[act, sf[c]].copy()
            missing, default_left = (dt[c] >> 2) & 3, (dt[c] & 2) != 0
            nan = np.isnan(x)
            x[nan & (missing != 2)] = 0
            use_default = ((missing == 1) & (np.abs(x) <= ZERO_THRESHOLD)) | ((missing == 2) & nan)
            with np.errstate(invalid='ignore'):
                left = np.where(use_default, default_left, x.astype(np.float64) <= thr[c])
            cur[act] = np.where(left, lc[c], rc[c])
        assert (cur < 0).all(), f'tree {t}: a walk did not end within L - 1 steps'
        out[:, t] = ~cur
    return out


def raw_scores(forest, X, leaf=None):
    """The float64 sum of the reached leaf values, trees added in order."""
    leaf = leaves(forest, X) if leaf is None else leaf
    acc = np.zeros(leaf.shape[0], dtype=np.float64)
    for t in range(forest.n_trees):
        acc = acc + forest.leaf_value[int(forest.leaf_off[t]) + leaf[:, t].astype(np.int64)]
    return acc


def ensemble(forests, X):
    """acc = 0.0; for each forest: acc += float64(float32(raw)) / n_forests."""
    acc = np.zeros(np.asarray(X).shape[0], dtype=np.float64)
    with np.errstate(over='ignore'):
        for f in forests:
            acc = acc + raw_scores(f, X).astype(np.float32).astype(np.float64) / np.float64(len(forests))
    return acc


def session_topk(score, aid, row_off, k):
    """(top_aid int32 [S, k] padded -1, top_score float64 [S, k] padded -inf, n int32 [S], n_invalid_sessions).
    Stable sort by descending score: ties (and -0.0 / +0.0) keep the row order, NaN goes last."""
    score, aid, row_off = np.asarray(score, dtype=np.float64), np.asarray(aid, dtype=np.int32), np.asarray(row_off, dtype=np.int64)
    S = row_off.size - 1
    top_aid = np.full((S, k), -1, dtype=np.int32)
    top_score = np.full((S, k), -np.inf, dtype=np.float64)
    n = np.zeros(S, dtype=np.int32)
    invalid = 0
    for s in range(S):
        lo, hi = int(row_off[s]), int(row_off[s + 1])
        if not 0 <= lo <= hi <= score.size:
            invalid += 1
            continue
        sc = score[lo:hi]
        order = np.argsort(-sc, kind='stable')[:k]       # numpy sorts NaN behind every number; stable among equals
        m = order.size
        top_aid[s, :m], top_score[s, :m], n[s] = aid[lo:hi][order], sc[order], m
    return top_aid, top_score, n, invalid


def floor_f32(t):
    """The largest float32 <= the float64 t (-inf if there is none; +inf stays +inf)."""
    t = np.float64(t)
    with np.errstate(over='ignore'):
        f = np.float32(t)
    if np.float64(f) > t:
        f = np.nextafter(f, np.float32(-np.inf), dtype=np.float32)
    return f


# ---- seeded synthetic forests for the device tests

def random_forest(rng, T, L, F, X=None, shape='random', dtypes=(2, 8, 10, 4, 6, 0)):
    """T trees of L leaves over F features. ``shape``: 'random' grows each tree by splitting a random leaf, 'left_chain'
    always splits the leftmost leaf (depth L - 1). Thresholds are drawn from the values of X's column when X is given
    (so x == threshold happens), nudged up by one float64 ulp half of the time as LightGBM's dumps do."""
    from otto_amd.ranker.forest import Forest
    sf, thr, dt, lc, rc, lv, node_off, leaf_off = [], [], [], [], [], [], [0], [0]
    for _ in range(T):
        nint = L - 1
        left, right = np.zeros(nint, dtype=np.int32), np.zeros(nint, dtype=np.int32)
        # grow: leaf slots are (parent, side); splitting a slot turns it into the next internal node
        slots = [(-1, 0)]
        for i in range(nint):
            j = 0 if shape == 'left_chain' else int(rng.integers(len(slots)))
            p, side = slots.pop(j)
            if p >= 0:
                (left if side == 0 else right)[p] = i
            slots[j:j] = [(i, 0), (i, 1)]
        order = rng.permutation(L) if shape == 'random' else np.arange(L)
        for leaf, (p, side) in zip(order, slots):
            if p >= 0:
                (left if side == 0 else right)[p] = ~int(leaf)
        f = rng.integers(0, F, nint).astype(np.int32)
        if X is not None and X.shape[0]:
            v = X[rng.integers(0, X.shape[0], nint), f]
            v = np.where(np.isfinite(v), v, np.float32(0.5)).astype(np.float64)
        else:
            v = rng.standard_normal(nint)
        bump = rng.random(nint) < 0.5
        v = np.where(bump, np.nextafter(v, np.inf), v)
        sf.append(f); thr.append(v); dt.append(rng.choice(np.array(dtypes, dtype=np.int8), nint)); lc.append(left); rc.append(right)
        lv.append(rng.standard_normal(L) * 0.1)
        node_off.append(node_off[-1] + nint); leaf_off.append(leaf_off[-1] + L)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)
    return Forest(node_off, leaf_off, cat(sf, np.int32), cat(thr, np.float64), cat(dt, np.int8), cat(lc, np.int32),
                  cat(rc, np.int32), cat(lv, np.float64), F)


def concat_forests(forests):
    """One forest holding the trees of several (same F), in order."""
    from otto_amd.ranker.forest import Forest
    cat = lambda name: np.concatenate([getattr(f, name) for f in forests])
    node_off, leaf_off = [np.zeros(1, dtype=np.int64)], [np.zeros(1, dtype=np.int64)]
    for f in forests:
        node_off.append(f.node_off[1:] + node_off[-1][-1])
        leaf_off.append(f.leaf_off[1:] + leaf_off[-1][-1])
    return Forest(np.concatenate(node_off), np.concatenate(leaf_off), cat('split_feature'), cat('threshold'), cat('decision_type'),
                  cat('left_child'), cat('right_child'), cat('leaf_value'), forests[0].n_features)


def random_rows(rng, n, F, lo=-3.0, hi=3.0):
    """float32 [n, F]: uniform values with NaN, +-0, +-1e-35f and +-inf sprinkled in."""
    X = rng.uniform(lo, hi, (n, F)).astype(np.float32)
    specials = np.array([0.0, -0.0, 1e-35, -1e-35, np.inf, -np.inf], dtype=np.float32)
    m = rng.random((n, F))
    X[m < 0.10] = np.nan
    pick = (m >= 0.10) & (m < 0.14)
    X[pick] = specials[rng.integers(0, specials.size, int(pick.sum()))]
    return X
