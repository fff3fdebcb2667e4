"""LightGBM forest scoring and per-session top-k on the device (SPEC-FOREST): a model-file parser
and thin Python over ``include/otto_forest.h``.

What this replaces in the reference: ``lgb.Booster.predict`` over every (session, candidate) row and the fold average
(``src/ranker/lgb_trainer.py:181, 248-266``), then "sort by (session, score desc), head(20)"
(``lgb_trainer.py:183-189``, ``src/ranker/inference.py:175-176, 245-246, 314-315``). Numerical splits only; raw scores
(no output transform). The caller supplies the float32 feature matrix and chunks its rows by whole sessions.
"""

import numpy as np

from .. import _lib

MAX_LEAVES = 2048        # OTTO_FOREST_MAX_LEAVES
MAX_FEATURES = 128       # OTTO_FOREST_MAX_FEATURES
MAX_K = 64               # OTTO_FOREST_MAX_K
GROUP_BYTES = 24576      # OTTO_FOREST_GROUP_BYTES

_NODE_ARRAYS = (('split_feature', np.int32), ('threshold', np.float64), ('decision_type', np.int8),
                ('left_child', np.int32), ('right_child', np.int32))


class Forest:
    """The unpacked trees of one model: ``node_off`` / ``leaf_off`` int64 [T+1] (tree t owns nodes
    ``[node_off[t], node_off[t+1])`` and leaves ``[leaf_off[t], leaf_off[t+1])``), ``split_feature`` int32, ``threshold``
    float64, ``decision_type`` int8, ``left_child`` / ``right_child`` int32 (c >= 0: internal node c of the tree, c < 0:
    leaf ``~c``), ``leaf_value`` float64; ``feature_names``, ``n_features``, ``objective`` (kept as a string; the
    scores are raw)."""

    def __init__(self, node_off, leaf_off, split_feature, threshold, decision_type, left_child, right_child, leaf_value,
                 n_features, feature_names=None, objective=''):
        self.node_off = np.ascontiguousarray(node_off, dtype=np.int64)
        self.leaf_off = np.ascontiguousarray(leaf_off, dtype=np.int64)
        self.split_feature = np.ascontiguousarray(split_feature, dtype=np.int32)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        self.decision_type = np.ascontiguousarray(decision_type, dtype=np.int8)
        self.left_child = np.ascontiguousarray(left_child, dtype=np.int32)
        self.right_child = np.ascontiguousarray(right_child, dtype=np.int32)
        self.leaf_value = np.ascontiguousarray(leaf_value, dtype=np.float64)
        self.n_features = int(n_features)
        self.feature_names = list(feature_names) if feature_names is not None else [f'Column_{i}' for i in range(self.n_features)]
        self.objective = objective
        if self.node_off.ndim != 1 or self.node_off.shape != self.leaf_off.shape or self.node_off.size < 2:
            raise ValueError('node_off and leaf_off: expected int64 [T+1] with T >= 1')
        n_nodes, n_leaves = int(self.node_off[-1]), int(self.leaf_off[-1])
        for name, _ in _NODE_ARRAYS:
            if getattr(self, name).shape != (n_nodes,):
                raise ValueError(f'{name}: expected {n_nodes} entries (node_off[-1])')
        if self.leaf_value.shape != (n_leaves,):
            raise ValueError(f'leaf_value: expected {n_leaves} entries (leaf_off[-1])')
        self._packed = {}

    @property
    def n_trees(self):
        return self.node_off.size - 1

    @property
    def num_leaves(self):
        return np.diff(self.leaf_off)

    def pack(self):
        """The packed image (``include/otto_forest.h``) as a uint8 array; raises ``OttoError`` with the validation
        message of ``otto_forest_pack`` for a forest it refuses."""
        lib = _lib.lib()
        n = int(lib.otto_forest_packed_bytes(self.n_trees, int(self.node_off[-1]), int(self.leaf_off[-1])))
        if n <= 0:
            raise _lib.OttoError('otto_forest_packed_bytes refused the forest (tree, node and leaf counts disagree)')
        out = np.zeros(n, dtype=np.uint8)
        _lib.call('otto_forest_pack', None, self.n_trees, self.n_features, self.node_off, self.leaf_off, self.split_feature,
                  self.threshold, self.decision_type, self.left_child, self.right_child, self.leaf_value, out, n, stream=False)
        return out

    def to(self, device):
        """Pack (once) and upload (once per device); returns ``self``."""
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.OttoError('Forest.to needs a ROCm device (no CPU fallback)')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._packed:
            self._packed[device] = torch.from_numpy(self.pack()).to(device)
        return self


class ModelFormatError(ValueError):
    pass


def _fail(lineno, msg):
    raise ModelFormatError(f'line {lineno}: {msg}')


def parse_lightgbm_model(text):
    """A :class:`Forest` from a LightGBM v3 text dump: the header keys ``version``, ``num_class``,
    ``num_tree_per_iteration``, ``max_feature_idx``, ``objective``, ``feature_names``, ``tree_sizes``, then the
    ``Tree=i`` blocks up to ``end of trees`` (everything behind that line is ignored). Refused, with the line number:
    ``num_class != 1``, ``num_tree_per_iteration != 1``, ``num_cat > 0``, ``is_linear=1``, ``average_output``, a tree
    count that disagrees with ``tree_sizes``, an array whose length disagrees with ``num_leaves``."""
    header, trees, cur = {}, [], None
    ended = False
    for lineno, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if line == 'end of trees':
            ended = True
            break
        if not line or (lineno == 1 and line == 'tree'):
            continue
        if line == 'average_output':
            _fail(lineno, 'average_output (a random-forest model) is not supported')
        if '=' not in line:
            _fail(lineno, f'expected key=value, got {line[:40]!r}')
        key, val = line.split('=', 1)
        if key == 'Tree':
            if val != str(len(trees)):
                _fail(lineno, f'expected Tree={len(trees)}, got Tree={val}')
            cur = {'Tree': (lineno, val)}
            trees.append(cur)
        elif cur is None:
            header[key] = (lineno, val)
        else:
            cur[key] = (lineno, val)
    if not ended:
        raise ModelFormatError('no "end of trees" line')

    def h_int(key, want=None):
        if key not in header:
            raise ModelFormatError(f'header key {key} is missing')
        lineno, val = header[key]
        try:
            v = int(val)
        except ValueError:
            _fail(lineno, f'{key}={val!r} is not an integer')
        if want is not None and v != want:
            _fail(lineno, f'{key}={v} is not supported (only {key}={want})')
        return v

    if 'version' not in header or header['version'][1] != 'v3':
        _fail(header.get('version', (1, ''))[0], f'version={header.get("version", (1, "?"))[1]} is not supported (only version=v3)')
    h_int('num_class', 1)
    h_int('num_tree_per_iteration', 1)
    n_features = h_int('max_feature_idx') + 1
    names = header['feature_names'][1].split() if 'feature_names' in header else None
    if names is not None and len(names) != n_features:
        _fail(header['feature_names'][0], f'{len(names)} feature_names for max_feature_idx={n_features - 1}')
    if 'tree_sizes' in header:
        lineno, val = header['tree_sizes']
        if len(val.split()) != len(trees):
            _fail(lineno, f'tree_sizes lists {len(val.split())} trees, the file holds {len(trees)}')
    if not trees:
        raise ModelFormatError('the model holds no tree')

    cols = {name: [] for name, _ in _NODE_ARRAYS}
    leaf_value, node_off, leaf_off = [], [0], [0]
    for t, tr in enumerate(trees):
        def t_int(key, default=None):
            if key not in tr:
                if default is not None:
                    return tr['Tree'][0], default
                _fail(tr['Tree'][0], f'Tree={t} has no {key}')
            try:
                return tr[key][0], int(tr[key][1])
            except ValueError:
                _fail(tr[key][0], f'{key}={tr[key][1]!r} is not an integer')

        def t_array(key, dtype, want):
            if key not in tr:
                if want == 0:
                    return np.zeros(0, dtype=dtype)
                _fail(tr['Tree'][0], f'Tree={t} has no {key}')
            lineno, val = tr[key]
            try:
                a = np.array([float(x) for x in val.split()], dtype=np.float64) if dtype == np.float64 else \
                    np.array([int(x) for x in val.split()], dtype=np.int64)
            except ValueError:
                _fail(lineno, f'{key} of Tree={t} holds a value that is not a number')
            if a.size != want:
                _fail(lineno, f'{key} of Tree={t} has {a.size} entries, num_leaves={want + (key != "leaf_value")} needs {want}')
            if dtype != np.float64 and a.size and (a.min() < np.iinfo(dtype).min or a.max() > np.iinfo(dtype).max):
                _fail(lineno, f'{key} of Tree={t} holds a value outside {np.dtype(dtype).name}')
            return a.astype(dtype)

        lineno, L = t_int('num_leaves')
        if L < 1:
            _fail(lineno, f'num_leaves={L}')
        lineno, num_cat = t_int('num_cat', 0)
        if num_cat > 0:
            _fail(lineno, f'num_cat={num_cat}: categorical splits are not supported')
        lineno, is_linear = t_int('is_linear', 0)
        if is_linear != 0:
            _fail(lineno, 'is_linear=1: linear trees are not supported')
        for name, dtype in _NODE_ARRAYS:
            cols[name].append(t_array(name, dtype, L - 1))
        leaf_value.append(t_array('leaf_value', np.float64, L))
        node_off.append(node_off[-1] + L - 1)
        leaf_off.append(leaf_off[-1] + L)
    return Forest(node_off, leaf_off, *(np.concatenate(cols[name]) for name, _ in _NODE_ARRAYS), np.concatenate(leaf_value),
                  n_features, feature_names=names, objective=header['objective'][1] if 'objective' in header else '')


def load_lightgbm_model(path):
    with open(path) as f:
        return parse_lightgbm_model(f.read())


def _check_X(forest, X):
    import torch
    if not isinstance(forest, Forest):
        raise ValueError('forest: expected a Forest (parse_lightgbm_model / load_lightgbm_model)')
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError('X: expected a float32 tensor [n_rows, >= n_features]')
    if X.device.type != 'cuda':
        raise _lib.OttoError('forest scoring needs a ROCm device (no CPU fallback)')
    if X.shape[1] < forest.n_features:
        raise ValueError(f'X has {X.shape[1]} columns, the forest reads {forest.n_features}')
    if X.shape[0] and (X.stride(1) != 1 or X.stride(0) < forest.n_features):
        raise ValueError('X: expected row-major rows (stride(1) == 1); a column slice X[:, :F] of a wider matrix is fine')
    return int(X.shape[0]), int(X.stride(0)) if X.shape[0] else max(int(X.shape[1]), 1)


def _predict_into(forest, X, raw, acc, divisor):
    n, ld = _check_X(forest, X)
    img = forest.to(X.device)._packed[X.device]
    # X goes in as rows with the leading dimension ld (_check_X): it may be a column slice of a wider matrix
    _lib.call('otto_forest_predict', X.device, img, img.numel(), _lib.ptr(X), ld, n, forest.n_features, raw, acc, float(divisor))


def forest_predict(forest, X):
    """Raw scores float64 [n_rows] of ``X`` float32 [n_rows, >= n_features] on the device: the leaf values of the T trees
    added in tree order in float64."""
    import torch
    _check_X(forest, X)
    raw = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
    _predict_into(forest, X, raw, None, 1.0)
    return raw


def forest_leaves(forest, X):
    """The reached leaf of every (row, tree), int32 [n_rows, T] (``Booster.predict(pred_leaf=True)``)."""
    import torch
    n, ld = _check_X(forest, X)
    img = forest.to(X.device)._packed[X.device]
    leaf = torch.empty((n, forest.n_trees), dtype=torch.int32, device=X.device)
    _lib.call('otto_forest_leaves', X.device, img, img.numel(), _lib.ptr(X), ld, n, forest.n_features, forest.n_trees, leaf)
    return leaf


def ensemble_predict(forests, X):
    """The fold average of ``lgb_trainer.py:248-261``: ``acc = 0.0; acc += float64(float32(raw_i)) / n_forests`` per
    forest, in the order given. float64 [n_rows]."""
    import torch
    forests = list(forests)
    if not forests:
        raise ValueError('forests: expected at least one Forest')
    for f in forests:
        _check_X(f, X)
    acc = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
    for f in forests:
        _predict_into(f, X, None, acc, float(len(forests)))
    return acc


def session_topk(score, aid, row_off, k=20):
    """Per session (rows ``[row_off[s], row_off[s+1])``) the first ``k`` rows by (score descending, row position
    ascending); NaN after every number, -0.0 and +0.0 tie. ``score`` float64 [n_rows], ``aid`` int32 [n_rows],
    ``row_off`` int64 [S+1], all on the device. Returns (top_aid int32 [S, k] (-1 padded), top_score float64 [S, k]
    (-inf padded), n int32 [S])."""
    import torch
    _lib.need(score, 'score', torch.float64, 1)
    dev = score.device
    _lib.need(aid, 'aid', torch.int32, 1, device=dev)
    _lib.need(row_off, 'row_off', torch.int64, 1, device=dev)
    if aid.numel() != score.numel():
        raise ValueError(f'aid has {aid.numel()} rows, score has {score.numel()}')
    if row_off.numel() < 1:
        raise ValueError('row_off: expected int64 [S+1]')
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    S = row_off.numel() - 1
    top_aid = torch.empty((S, k), dtype=torch.int32, device=dev)
    top_score = torch.empty((S, k), dtype=torch.float64, device=dev)
    n = torch.empty(S, dtype=torch.int32, device=dev)
    _lib.call('otto_forest_session_topk', dev, score, aid, row_off, S, score.numel(), k, top_aid, top_score, n)
    return top_aid, top_score, n


def rank_candidates(forests, X, aid, row_off, k=20):
    """:func:`ensemble_predict` over the candidate rows, then :func:`session_topk`: (top_aid, top_score, n)."""
    return session_topk(ensemble_predict(forests, X), aid, row_off, k=k)
