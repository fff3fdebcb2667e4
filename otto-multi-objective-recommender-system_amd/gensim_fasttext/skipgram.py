"""Skip-gram negative-sampling aid embeddings on the device (SPEC-SGNS): thin Python over
``include/otto_sgns.h``.

What this replaces in the reference: ``fasttext.train_unsupervised`` with ``models/fasttext/config.yaml`` (skipgram, loss
ns, ``minn = maxn = 0``: no sub-words) and gensim's ``Word2Vec(sg=1, negative>0)`` of ``src/gensim_fasttext/trainer.py``.
The vocabulary tables are computed here on the host in float64 and integers; subsampling, windows, negative draws and the
SGD step run in HIP kernels. There is no CPU fallback.

gensim's ``hs: 1`` next to ``negative > 0`` (SPEC-SGNS-HS) adds the Huffman path of every pair's context in front of its
negative-sampling targets: :func:`huffman_tables` builds the tree and the path tables in the library (host C++), the
engine takes them as ``hs=`` and trains a third table ``Syn1``.

CBOW (fastText ``model: cbow``, gensim ``sg: 0``) and Doc2Vec (PV-DM, PV-DBOW; SPEC-CBOW and SPEC-DOC2VEC) run on the same
plan, sampler and tables through :meth:`SkipGramEngine.step_cbow`, :func:`train_cbow` and :func:`train_doc2vec`; the two
Doc2Vec archs train ``Doc``, one row per session.

A session that took no part in training gets its vector from :func:`infer_doc2vec` (SPEC-DOC2VEC-INFER, gensim's
``infer_vector``): one launch over all passes against a frozen :class:`Doc2VecModel`, which :func:`train_doc2vec` returns
with ``return_model=True`` and :func:`doc2vec_model` builds from arrays.
"""
import ctypes as C

import numpy as np

from .. import _lib

HOGWILD, BATCH = 0, 1               # OTTO_SGNS_HOGWILD, OTTO_SGNS_BATCH
ARCH_CBOW, ARCH_PVDM, ARCH_DBOW = 0, 1, 2               # OTTO_SGNS_ARCH_*
CBOW_SUM, CBOW_MEAN, CBOW_FASTTEXT = 0, 1, 2            # OTTO_SGNS_CBOW_*
MAX_DIM, MAX_NEG, MAX_WS = 128, 64, 32
MAX_INFER_PASSES = 64               # OTTO_SGNS_MAX_INFER_PASSES
NS_EXPONENTS = (0.0, 0.5, 0.75, 1.0)
_U32_MAX = (1 << 32) - 1
_MAX_BUCKETS = 1 << 21


def _host_counts(aid, n_aids):
    if hasattr(aid, 'device') and hasattr(aid, 'cpu'):            # a torch tensor: count where it lives
        import torch
        if aid.numel() and (int(aid.min()) < 0 or int(aid.max()) >= n_aids):
            raise ValueError(f'aid outside [0, {n_aids})')
        return torch.bincount(aid.to(torch.int64), minlength=n_aids).cpu().numpy().astype(np.int64)
    aid = np.asarray(aid)
    if aid.size and (aid.min() < 0 or aid.max() >= n_aids):
        raise ValueError(f'aid outside [0, {n_aids})')
    return np.bincount(aid.astype(np.int64), minlength=n_aids).astype(np.int64)


def vocab_tables(aid, n_aids, min_count=1, t=1e-4, ns_exponent=0.5):
    """``(count int64, keep_q uint32, weight uint32)`` NumPy arrays [n_aids] of SPEC-SGNS. ``aid``: the events (a NumPy
    array, or a tensor on any device: the counts are taken where it lives). ``keep_q = min(2^32 - 1, floor(p * 2^32))``
    with ``p = sqrt(t/f) + t/f``, ``f = count/E`` (``t = 0``: always kept); ``weight = min(2^32 - 1, floor(count^e *
    2^16))`` with ``e`` in {0, 0.5, 0.75, 1}; an aid with ``count < min_count`` (or no event) has both 0."""
    n_aids, min_count, t, e = int(n_aids), int(min_count), float(t), float(ns_exponent)
    if n_aids < 1:
        raise ValueError('n_aids must be positive')
    if t < 0:
        raise ValueError('t must be >= 0')
    if e not in NS_EXPONENTS:
        raise ValueError(f'ns_exponent must be one of {NS_EXPONENTS} (got {ns_exponent})')
    return _tables_of_counts(_host_counts(aid, n_aids), min_count, t, e)


def _tables_of_counts(count, min_count, t, e):
    """:func:`vocab_tables` from the counts on: what training and inference both derive from ``count``."""
    n_aids = len(count)
    E = int(count.sum())
    in_vocab = count >= max(min_count, 1)
    c = count.astype(np.float64)
    keep_q = np.zeros(n_aids, dtype=np.uint32)
    if t == 0.0:
        keep_q[in_vocab] = _U32_MAX
    else:
        f = c[in_vocab] / float(E)
        p = np.sqrt(t / f) + t / f
        keep_q[in_vocab] = np.minimum(np.floor(p * 4294967296.0), float(_U32_MAX)).astype(np.uint64).astype(np.uint32)
    if e == 0.0:
        w = np.ones_like(c)
    elif e == 0.5:
        w = np.sqrt(c)
    elif e == 0.75:
        r = np.sqrt(np.sqrt(c))          # exact on fourth powers, and so is r^3
        w = r * r * r
    else:
        w = c
    weight = np.zeros(n_aids, dtype=np.uint32)
    weight[in_vocab] = np.minimum(np.floor(w[in_vocab] * 65536.0), float(_U32_MAX)).astype(np.uint64).astype(np.uint32)
    return count, keep_q, weight


class HuffmanTables:
    """The path tables of SPEC-SGNS-HS (NumPy, host): ``V`` in-vocabulary aids, ``n_inner = max(V - 1, 1)`` rows of
    ``Syn1``, ``path_off`` int64 [n_aids+1], ``path_node`` int32 [sum L], ``code`` uint64 [n_aids], ``max_len``."""

    def __init__(self, V, path_off, path_node, code, max_len):
        self.V, self.n_inner, self.max_len = int(V), max(int(V) - 1, 1), int(max_len)
        self.path_off, self.path_node, self.code = path_off, path_node, code

    @property
    def n_aids(self):
        return len(self.path_off) - 1

    def lengths(self):
        """int64 [n_aids]: the path length of every aid (0 outside the vocabulary)"""
        return np.diff(self.path_off)


def huffman_tables(count, min_count=1):
    """:class:`HuffmanTables` over ``count`` int64 [n_aids] (:func:`vocab_tables`'s first result): the word2vec.c tree
    over the aids with ``count >= max(min_count, 1)``, leaves by count descending then aid ascending. Built by
    ``otto_sgns_hs_tree`` on the host; raises ``OttoError`` when a path is longer than the 64 bits of a code word."""
    count = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
    if count.ndim != 1 or count.size < 1:
        raise ValueError('count: expected int64 [n_aids], n_aids >= 1')
    n = int(count.size)
    sizes = np.zeros(3, dtype=np.int64)
    _lib.call('otto_sgns_hs_tree_sizes', None, count, n, int(min_count), sizes.ctypes.data_as(C.POINTER(C.c_int64)), stream=False)
    V, total, max_len = (int(x) for x in sizes)
    path_off = np.zeros(n + 1, dtype=np.int64)
    path_node = np.zeros(total, dtype=np.int32)
    code = np.zeros(n, dtype=np.uint64)
    _lib.call('otto_sgns_hs_tree', None, count, n, int(min_count), path_off, path_node, total, code, stream=False)
    return HuffmanTables(V, path_off, path_node, code, max_len)


def init_tables(n_aids, d, seed=0):
    """``(In, Out)`` float32 NumPy [n_aids, d]: ``In`` uniform(-1/d, 1/d), ``Out`` zeros, as fastText initialises."""
    rng = np.random.default_rng(int(seed))
    In = rng.uniform(-1.0 / d, 1.0 / d, size=(int(n_aids), int(d))).astype(np.float32)
    return In, np.zeros((int(n_aids), int(d)), dtype=np.float32)


def learning_rate(lr, events_consumed, total_events):
    """The rate of a launch: ``lr * max(1e-4, 1 - events_consumed / total_events)``; ``events_consumed`` counts events
    before subsampling, as fastText's ``tokenCount`` does; ``total_events = epochs * E``."""
    return float(lr) * max(1e-4, 1.0 - float(events_consumed) / float(max(int(total_events), 1)))


class Plan:
    """One epoch's plan on the device: ``tok_aid`` int32 [T], ``tok_src`` int64 [T], ``tok_off`` int64 [S+1], ``radius``
    uint8 [T], ``tok_left`` uint8 [T], ``pair_off`` int64 [T+1]; ``T`` tokens, ``P`` pairs, ``epoch``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _as_u32_tensor(a, dev):
    import torch
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    return torch.from_numpy(a.view(np.int32)).to(dev)


def _check_hyper(d, neg, ws, seed, name='d', hs=True):
    """``(d, neg, ws, seed)`` as ints, ``ValueError`` (naming the argument as given, ``d`` as ``name``) unless they are in
    SPEC-SGNS's ranges; ``hs=False``: ``neg = 0`` leaves a frozen model without targets."""
    di, negi, wsi, seedi = int(d), int(neg), int(ws), int(seed)
    if di % 4 or not 4 <= di <= MAX_DIM or (di // 4) & (di // 4 - 1):
        raise ValueError(f'{name} must be a multiple of 4 in [4, {MAX_DIM}] with {name}/4 a power of two (got {d})')
    if not 0 <= negi <= MAX_NEG:
        raise ValueError(f'neg must be in [0, {MAX_NEG}] (got {neg})')
    if negi == 0 and not hs:
        raise ValueError('neg = 0 without hierarchical softmax leaves nothing to infer against')
    if not 1 <= wsi <= MAX_WS:
        raise ValueError(f'ws must be in [1, {MAX_WS}] (got {ws})')
    if not 0 <= seedi < 1 << 64:
        raise ValueError('seed: expected a uint64')
    return di, negi, wsi, seedi


class SkipGramEngine:
    """Plan / step with persistent workspaces. ``keep_q`` / ``weight``: the uint32 tables of :func:`vocab_tables`.
    ``hs``: the :class:`HuffmanTables` of :func:`huffman_tables` (or any object with its fields); they are uploaded, and
    :meth:`step` then trains the path half of SPEC-SGNS-HS on a ``Syn1`` float32 [hs.n_inner, d] table."""

    def __init__(self, n_aids, d, ws, neg, keep_q, weight, seed=0, device='cuda:0', n_buckets=None, hs=None):
        import torch
        self.dev = _lib.rocm_device(device, 'SkipGramEngine')
        self.n_aids = int(n_aids)
        self.d, self.neg, self.ws, self.seed = _check_hyper(d, neg, ws, seed)
        if len(keep_q) != self.n_aids or len(weight) != self.n_aids:
            raise ValueError('keep_q and weight must have n_aids entries')
        self.lib = _lib.lib()
        if n_buckets is None:
            n_buckets = 1
            while n_buckets < self.n_aids and n_buckets < _MAX_BUCKETS:
                n_buckets *= 2
        self.n_buckets = int(n_buckets)
        with torch.cuda.device(self.dev):
            self.keep_q = _as_u32_tensor(keep_q, self.dev)
            self.weight = _as_u32_tensor(weight, self.dev)
            self.cum = torch.empty(self.n_aids, dtype=torch.int64, device=self.dev)
            self.bucket = torch.empty(self.n_buckets + 1, dtype=torch.int32, device=self.dev)
            self.table = _lib.SgnsTable()
            nb = self.lib.otto_sgns_neg_table_workspace(self.n_aids)
            if nb <= 0:
                raise _lib.OttoError('otto_sgns_neg_table_workspace refused its arguments')
            work = _lib.workspace(nb, self.dev)
            self._call('otto_sgns_neg_table', self.weight, self.n_aids, self.n_buckets, self.cum, self.bucket, C.byref(self.table),
                       work, work.numel())
        self._work = None
        self._bufs = None
        self._grads = None
        self._gsyn1 = None
        self._gdoc = None
        self.hs = None
        self.Syn1 = None                 # the table of the last HS step (train(hs=True) leaves its own here)
        if hs is not None:
            self._upload_hs(hs)
        self._loss = torch.zeros(1, dtype=torch.float64, device=self.dev)

    def _call(self, name, *args):
        _lib.call(name, self.dev, *args)

    def _need_table(self, name, M, rows):
        """``ValueError`` unless ``M`` is a table a step can train: contiguous float32 [rows, d] on the engine's device"""
        import torch
        if M is None or M.dtype != torch.float32 or tuple(M.shape) != (rows, self.d) or not M.is_contiguous() or M.device != self.dev:
            raise ValueError(f'{name}: expected contiguous float32 [{rows}, {self.d}] on {self.dev}')

    def _workspaces(self, mode, doc_rows=None):
        """``(gin, gout, gsyn1, gdoc)`` of a launch: None in HOGWILD; in BATCH the float64 workspaces, made zero at their
        first use (a launch leaves them zero), ``gsyn1`` with Huffman tables only and ``gdoc`` [doc_rows, d] for the Doc2Vec
        archs only."""
        import torch
        if mode != BATCH:
            return None, None, None, None
        z = lambda rows: torch.zeros(rows, self.d, dtype=torch.float64, device=self.dev)
        if self._grads is None:
            self._grads = (z(self.n_aids), z(self.n_aids))
        if self.hs is not None and self._gsyn1 is None:
            self._gsyn1 = z(self.n_inner)
        if doc_rows is not None and (self._gdoc is None or self._gdoc.shape[0] != doc_rows):
            self._gdoc = z(doc_rows)
        return (*self._grads, self._gsyn1 if self.hs is not None else None, self._gdoc if doc_rows is not None else None)

    def _upload_hs(self, hs):
        import torch
        path_off = np.ascontiguousarray(np.asarray(hs.path_off, dtype=np.int64))
        path_node = np.ascontiguousarray(np.asarray(hs.path_node, dtype=np.int32))
        code = np.ascontiguousarray(np.asarray(hs.code, dtype=np.uint64))
        n_inner = int(hs.n_inner)
        if path_off.shape != (self.n_aids + 1,) or code.shape != (self.n_aids,):
            raise ValueError(f'hs: path_off needs n_aids + 1 = {self.n_aids + 1} entries and code n_aids')
        lens = np.diff(path_off)
        if path_off[0] != 0 or (lens < 0).any() or (lens > 64).any() or path_off[-1] != path_node.size:
            raise ValueError('hs: path_off must ascend from 0 to len(path_node) in rows of at most 64 ids')
        if not 1 <= n_inner < 1 << 31 or (path_node.size and (path_node.min() < 0 or path_node.max() >= n_inner)):
            raise ValueError('hs: n_inner must be positive and every path id below it')
        self.hs = hs
        self.n_inner = n_inner
        self._path_off = torch.from_numpy(path_off).to(self.dev)
        self._path_node = torch.from_numpy(path_node if path_node.size else np.zeros(1, dtype=np.int32)).to(self.dev)
        self._code = torch.from_numpy(code.view(np.int64)).to(self.dev)
        self._path_len = torch.from_numpy(lens.astype(np.int64)).to(self.dev)
        self._gsyn1 = None

    def path_targets(self, plan, t0=0, t1=None):
        """The sum of the path lengths of the contexts of all pairs of the centres ``[t0, t1)`` of ``plan`` (an int),
        computed on the device: the contexts of centre c are the tokens c - left .. c - 1 and c + 1 .. c + right, two
        ranges of a prefix sum over the tokens' path lengths."""
        import torch
        t1 = plan.T if t1 is None else int(t1)
        if self.hs is None or t1 <= t0:
            return 0
        cs = torch.zeros(plan.T + 1, dtype=torch.int64, device=self.dev)
        cs[1:] = torch.cumsum(self._path_len[plan.tok_aid.to(torch.int64)], 0)
        c = torch.arange(int(t0), t1, dtype=torch.int64, device=self.dev)
        left = plan.tok_left[t0:t1].to(torch.int64)
        right = plan.pair_off[t0 + 1:t1 + 1] - plan.pair_off[t0:t1] - left
        return int((cs[c] - cs[c - left] + cs[c + 1 + right] - cs[c + 1]).sum().item())

    @property
    def total(self):
        return int(self.table.total)

    def draw(self, keys):
        """``upper_bound(cum, mulhi64(key, total))`` for every key: int64-viewed uint64 tensor [m] -> int32 [m]."""
        import torch
        out = torch.empty(keys.numel(), dtype=torch.int32, device=self.dev)
        self._call('otto_sgns_draw', C.byref(self.table), keys, keys.numel(), out)
        return out

    def plan(self, aid, sess_off, epoch, event0=0, out=None):
        """The :class:`Plan` of ``epoch`` over ``aid`` int32 [E] / ``sess_off`` int64 [S+1] on the device. ``out``: a
        dict of pre-allocated output tensors (tests); by default the engine's persistent buffers are reused, so a plan is
        valid until the next call. Raises ``OttoError`` for an aid outside ``[0, n_aids)`` or bad offsets."""
        import torch
        _lib.need(aid, 'aid', torch.int32, device=self.dev)
        _lib.need(sess_off, 'sess_off', torch.int64, device=self.dev)
        E, S = int(aid.numel()), int(sess_off.numel()) - 1
        if S < 0:
            raise ValueError('sess_off: expected int64 [S+1]')
        with torch.cuda.device(self.dev):
            nb = self.lib.otto_sgns_plan_workspace(E)
            if nb <= 0:
                raise _lib.OttoError('otto_sgns_plan_workspace refused its arguments')
            if self._work is None or self._work.numel() < nb:
                self._work = _lib.workspace(nb, self.dev)
            if out is None:
                if self._bufs is None or self._bufs['tok_aid'].numel() < E or self._bufs['tok_off'].numel() < S + 1:
                    self._bufs = dict(tok_aid=torch.empty(E, dtype=torch.int32, device=self.dev),
                                      tok_src=torch.empty(E, dtype=torch.int64, device=self.dev),
                                      tok_off=torch.empty(S + 1, dtype=torch.int64, device=self.dev),
                                      radius=torch.empty(E, dtype=torch.uint8, device=self.dev),
                                      tok_left=torch.empty(E, dtype=torch.uint8, device=self.dev),
                                      pair_off=torch.empty(E + 1, dtype=torch.int64, device=self.dev))
                out = self._bufs
            cap = min(out['tok_aid'].numel(), out['tok_src'].numel(), out['radius'].numel(), out['tok_left'].numel(),
                      out['pair_off'].numel() - 1)
            if out['tok_off'].numel() < S + 1:
                raise ValueError('tok_off: room for S + 1 entries needed')
            counts = (C.c_int64 * 2)()
            self._call('otto_sgns_plan', aid, E, sess_off, S, self.keep_q, self.n_aids, self.seed, int(epoch), int(event0), self.ws,
                       cap, out['tok_aid'], out['tok_src'], out['tok_off'], out['radius'], out['tok_left'], out['pair_off'], counts,
                       self._work, self._work.numel())
        T, P = int(counts[0]), int(counts[1])
        return Plan(tok_aid=out['tok_aid'][:T], tok_src=out['tok_src'][:T], tok_off=out['tok_off'][:S + 1],
                    radius=out['radius'][:T], tok_left=out['tok_left'][:T], pair_off=out['pair_off'][:T + 1], T=T, P=P,
                    epoch=int(epoch))

    def step(self, plan, t0, t1, In, Out, lr, mode=HOGWILD, ctx_out=None, neg_out=None, loss=None, Syn1=None):
        """One launch over the centres ``[t0, t1)`` of ``plan``; updates ``In`` / ``Out`` (float32 [n_aids, d] on the
        device) in place and returns the device float64 [1] loss sum. ``ctx_out`` int32 [pairs], ``neg_out`` int32
        [pairs, neg]: the sampler's choices for the launch's pairs (tests). An engine built with ``hs=`` takes the
        SPEC-SGNS-HS entry point and needs ``Syn1`` float32 [hs.n_inner, d], updated in place as well; without tables
        ``Syn1`` must stay None."""
        import torch
        self._need_table('In', In, self.n_aids)
        self._need_table('Out', Out, self.n_aids)
        if self.hs is None and Syn1 is not None:
            raise ValueError('Syn1 given to an engine without hierarchical-softmax tables')
        if Syn1 is not None:
            self._need_table('Syn1', Syn1, self.n_inner)
        if mode not in (HOGWILD, BATCH):
            raise ValueError(f'unknown mode {mode}')
        out_pairs = 0
        if ctx_out is not None:
            out_pairs = ctx_out.numel()
        if neg_out is not None:
            out_pairs = neg_out.numel() // max(self.neg, 1) if ctx_out is None else min(out_pairs, neg_out.numel() // max(self.neg, 1))
        loss = self._loss if loss is None else loss
        with torch.cuda.device(self.dev):
            gin, gout, gsyn1, _ = self._workspaces(mode)
            if self.hs is not None:
                self._call('otto_sgns_step_hs', plan.tok_aid, plan.tok_src, plan.tok_left, plan.pair_off, plan.T, int(t0), int(t1),
                           In, Out, self.d, self.neg, float(lr), int(mode), self.seed, plan.epoch, C.byref(self.table), loss,
                           ctx_out, neg_out, out_pairs, gin, gout, self._path_off, self._path_node, self._code, Syn1,
                           self.n_inner, gsyn1)
                self.Syn1 = Syn1
                return loss
            self._call('otto_sgns_step', plan.tok_aid, plan.tok_src, plan.tok_left, plan.pair_off, plan.T, int(t0), int(t1), In, Out,
                       self.d, self.neg, float(lr), int(mode), self.seed, plan.epoch, C.byref(self.table), loss, ctx_out, neg_out,
                       out_pairs, gin, gout)
        return loss

    # ---- SPEC-CBOW, SPEC-DOC2VEC
    def cbow_targets(self, plan, arch, t0=0, t1=None):
        """The number of targets the centres ``[t0, t1)`` train under ``arch`` (an int, computed on the device): ``1 + neg``
        plus the path length of the centre's aid, for every centre that is not skipped (CBOW skips a centre without
        context)."""
        import torch
        t1 = plan.T if t1 is None else int(t1)
        if t1 <= t0:
            return 0
        aid = plan.tok_aid[t0:t1].to(torch.int64)
        per = torch.full_like(aid, 1 + self.neg)
        if self.hs is not None:
            per = per + self._path_len[aid]
        if arch == ARCH_CBOW:
            per = per * (plan.pair_off[t0 + 1:t1 + 1] > plan.pair_off[t0:t1])
        return int(per.sum().item())

    def _cbow_job(self, plan, t0, t1, In, Out, lr, arch, variant, mode, Syn1, Doc, neg_out, loss, grads):
        """The ``otto_sgns_cbow_job`` of one launch on the current stream; ``grads`` = (gin, gout, gsyn1, gdoc)."""
        p = lambda t, what: _lib.ptr(t, self.dev, what)
        hs = self.hs is not None
        S = int(plan.tok_off.numel()) - 1
        gin, gout, gsyn1, gdoc = grads
        return _lib.SgnsCbowJob(
            p(plan.tok_aid, 'tok_aid'), p(plan.tok_src, 'tok_src'), p(plan.tok_left, 'tok_left'), p(plan.pair_off, 'pair_off'),
            p(plan.tok_off, 'tok_off'), int(plan.T), S, int(t0), int(t1), p(In, 'In'), p(Out, 'Out'), p(Syn1, 'Syn1'), p(Doc, 'Doc'),
            self.n_aids, self.n_inner if hs else 0, self.d, self.neg, float(lr), int(arch), int(variant), int(mode), self.seed,
            int(plan.epoch), self.table, p(self._path_off, 'path_off') if hs else None, p(self._path_node, 'path_node') if hs else None,
            p(self._code, 'code') if hs else None, p(loss, 'loss'), p(neg_out, 'neg_out'), p(gin, 'gin'), p(gout, 'gout'),
            p(gsyn1, 'gsyn1'), p(gdoc, 'gdoc'), _lib.stream(self.dev))

    def step_cbow(self, plan, t0, t1, In, Out, lr, arch, variant=CBOW_MEAN, mode=HOGWILD, Syn1=None, Doc=None, neg_out=None,
                  loss=None):
        """One launch of SPEC-CBOW / SPEC-DOC2VEC over the centres ``[t0, t1)`` of ``plan``; returns the device float64 [1]
        loss sum. ``arch``: ``ARCH_CBOW`` (updates ``In`` and ``Out``), ``ARCH_PVDM`` (``In``, ``Out`` and ``Doc`` float32
        [S, d], one row per session of the plan) or ``ARCH_DBOW`` (``Out`` and ``Doc``; ``In`` may be None and is never
        touched). ``variant``: ``CBOW_SUM``, ``CBOW_MEAN`` or ``CBOW_FASTTEXT`` (ignored by DBOW). An engine built with
        ``hs=`` walks the centre's own Huffman path on ``Syn1`` first. ``neg_out`` int32 [t1 - t0, neg]: the sampler's
        choices per centre (tests)."""
        import torch
        if arch not in (ARCH_CBOW, ARCH_PVDM, ARCH_DBOW):
            raise ValueError(f'unknown arch {arch}')
        if arch != ARCH_DBOW and variant not in (CBOW_SUM, CBOW_MEAN, CBOW_FASTTEXT):
            raise ValueError(f'unknown variant {variant}')
        if mode not in (HOGWILD, BATCH):
            raise ValueError(f'unknown mode {mode}')
        S = int(plan.tok_off.numel()) - 1
        shapes = [('Out', Out, self.n_aids, True), ('In', In, self.n_aids, arch != ARCH_DBOW), ('Doc', Doc, S, arch != ARCH_CBOW),
                  ('Syn1', Syn1, self.n_inner if self.hs is not None else 0, self.hs is not None)]
        for name, M, rows, wanted in shapes:
            if M is None and not wanted:
                continue
            if name == 'Syn1' and self.hs is None:
                raise ValueError('Syn1 given to an engine without hierarchical-softmax tables')
            self._need_table(name, M, rows)
        if neg_out is not None:
            _lib.need(neg_out, 'neg_out', torch.int32, device=self.dev)
            if neg_out.numel() < (int(t1) - int(t0)) * self.neg:
                raise ValueError('neg_out: room for [t1 - t0, neg] entries needed')
        loss = self._loss if loss is None else loss
        with torch.cuda.device(self.dev):
            grads = self._workspaces(mode, S if arch != ARCH_CBOW else None)
            job = self._cbow_job(plan, t0, t1, In if arch != ARCH_DBOW else None, Out, lr, arch, variant, mode, Syn1,
                                 Doc if arch != ARCH_CBOW else None, neg_out, loss, grads)
            _lib.call('otto_sgns_cbow_step', self.dev, C.byref(job), stream=False)
        if self.hs is not None:
            self.Syn1 = Syn1
        return loss


def init_doc(n_sessions, d, seed=0):
    """``Doc`` float32 NumPy [n_sessions, d], uniform(-1/d, 1/d) from ``default_rng([seed, 1])``: a stream of its own, so
    that ``In`` is the same table with and without it."""
    rng = np.random.default_rng([int(seed), 1])
    return rng.uniform(-1.0 / d, 1.0 / d, size=(int(n_sessions), int(d))).astype(np.float32)


def _train_loop(step, targets, doc, aid, sess_off, n_aids, dim, ws, neg, epochs, lr, t, min_count, ns_exponent, seed,
                tokens_per_launch, device, hs):
    """The tables, the engine, the initial rows and the epoch / launch loop of :func:`train`, :func:`train_cbow` and
    :func:`train_doc2vec`. What differs comes in as two callables: ``step(eng, plan, t0, t1, In, Out, rate, Syn1, Doc)`` is one
    launch and returns its device loss sum, ``targets(eng, plan)`` is the denominator of the epoch's mean loss. ``doc``: a
    ``Doc`` table is trained. Returns ``(Doc or None, In, Out, losses, Syn1 or None)``."""
    import torch
    dev = aid.device if device is None else torch.device(device)
    tokens_per_launch = int(tokens_per_launch)
    if tokens_per_launch < 1:
        raise ValueError('tokens_per_launch must be positive')
    count, keep_q, weight = vocab_tables(aid, n_aids, min_count, t, ns_exponent)
    tables = huffman_tables(count, min_count) if hs else None
    eng = SkipGramEngine(n_aids, dim, ws, neg, keep_q, weight, seed=seed, device=dev, hs=tables)
    In_h, Out_h = init_tables(n_aids, dim, seed)
    In, Out = torch.from_numpy(In_h).to(eng.dev), torch.from_numpy(Out_h).to(eng.dev)
    Syn1 = torch.zeros(tables.n_inner, int(dim), dtype=torch.float32, device=eng.dev) if hs else None
    Doc = torch.from_numpy(init_doc(int(sess_off.numel()) - 1, dim, seed)).to(eng.dev) if doc else None
    E = int(aid.numel())
    losses = []
    for ep in range(int(epochs)):
        plan = eng.plan(aid, sess_off, ep)
        starts = list(range(0, plan.T, tokens_per_launch))
        first_src = plan.tok_src[torch.tensor(starts, dtype=torch.int64, device=eng.dev)].cpu().tolist() if starts else []
        total = torch.zeros(1, dtype=torch.float64, device=eng.dev)
        for t0, src in zip(starts, first_src):
            rate = learning_rate(lr, ep * E + int(src), int(epochs) * E)
            total += step(eng, plan, t0, min(t0 + tokens_per_launch, plan.T), In, Out, rate, Syn1, Doc)
        losses.append(float(total.item()) / max(targets(eng, plan), 1))
    return Doc, In, Out, losses, Syn1


def _train_arch(arch, variant, mode, neg, hs, *args):
    """:func:`_train_loop` over ``step_cbow``; ``args``: its arguments from ``aid`` on."""
    if int(neg) == 0 and not hs:
        raise ValueError('neg = 0 without hierarchical softmax leaves nothing to train against')
    return _train_loop(lambda eng, plan, t0, t1, In, Out, rate, Syn1, Doc:
                       eng.step_cbow(plan, t0, t1, In, Out, rate, arch, variant, mode, Syn1=Syn1, Doc=Doc),
                       lambda eng, plan: eng.cbow_targets(plan, arch), arch != ARCH_CBOW, *args)


def train_cbow(aid, sess_off, n_aids, dim=32, ws=10, neg=40, epochs=5, lr=0.05, t=1e-4, min_count=1, ns_exponent=0.5, seed=0,
               mode=HOGWILD, tokens_per_launch=1 << 24, device=None, hs=False, variant=CBOW_MEAN):
    """Train CBOW aid embeddings (SPEC-CBOW): the arguments, the loop, the launch cut and the rate of :func:`train`.
    ``variant``: ``CBOW_SUM`` (gensim ``cbow_mean: 0``), ``CBOW_MEAN`` (``cbow_mean: 1``) or ``CBOW_FASTTEXT`` (fastText
    ``model: cbow``). Returns ``(In, Out, losses)``, or ``(In, Out, losses, Syn1)`` with ``hs=True``; the mean loss divides
    by the number of targets actually trained (a centre without context trains none). ``neg = 0`` needs ``hs=True``."""
    _, In, Out, losses, Syn1 = _train_arch(ARCH_CBOW, variant, mode, neg, hs, aid, sess_off, n_aids, dim, ws, neg, epochs, lr, t,
                                           min_count, ns_exponent, seed, tokens_per_launch, device, hs)
    return (In, Out, losses, Syn1) if hs else (In, Out, losses)


def train_doc2vec(aid, sess_off, n_aids, dim=32, ws=10, neg=40, epochs=5, lr=0.05, t=1e-4, min_count=1, ns_exponent=0.5, seed=0,
                  mode=HOGWILD, tokens_per_launch=1 << 24, device=None, hs=False, dm=1, dm_mean=1, return_model=False):
    """Train session vectors (SPEC-DOC2VEC): ``dm=1`` is PV-DM (the mean of the context rows and the session's row with
    ``dm_mean=1``, their sum with ``dm_mean=0``), ``dm=0`` is PV-DBOW (``In`` is returned as initialised). ``Doc`` float32
    [S, dim] starts uniform(-1/dim, 1/dim) from ``default_rng([seed, 1])``. Returns ``(Doc, In, Out, losses)``, or
    ``(Doc, In, Out, losses, Syn1)`` with ``hs=True``. ``return_model=True`` appends the :class:`Doc2VecModel` of the run
    (the trained tables as they are on the device, the counts and the hyper-parameters): what :func:`infer_doc2vec`
    needs to embed a session that was not trained on."""
    arch = ARCH_PVDM if int(dm) else ARCH_DBOW
    variant = CBOW_MEAN if int(dm_mean) else CBOW_SUM
    Doc, In, Out, losses, Syn1 = _train_arch(arch, variant, mode, neg, hs, aid, sess_off, n_aids, dim, ws, neg, epochs, lr, t,
                                             min_count, ns_exponent, seed, tokens_per_launch, device, hs)
    out = (Doc, In, Out, losses, Syn1) if hs else (Doc, In, Out, losses)
    if return_model:
        out += (Doc2VecModel(In if int(dm) else None, Out, Syn1, _host_counts(aid, int(n_aids)), dim=dim, ws=ws, neg=neg, t=t,
                             min_count=min_count, ns_exponent=ns_exponent, seed=seed, dm=dm, dm_mean=dm_mean, hs=hs, lr=lr,
                             epochs=epochs),)
    return out


# ---- SPEC-DOC2VEC-INFER
class Doc2VecModel:
    """What training knew, frozen: ``In`` (PV-DM; None for PV-DBOW), ``Out`` float32 [n_aids, dim], ``Syn1`` float32
    [n_inner, dim] (with ``hs``, else None), ``count`` int64 [n_aids] of the training corpus, and the hyper-parameters
    ``dim, ws, neg, t, min_count, ns_exponent, seed, dm, dm_mean, hs, lr, epochs``. The tables are NumPy arrays or tensors on
    any device. ``ValueError`` for shapes and values no training run could have produced; nothing here touches a device."""
    HYPER = ('dim', 'ws', 'neg', 't', 'min_count', 'ns_exponent', 'seed', 'dm', 'dm_mean', 'hs', 'lr', 'epochs')

    def __init__(self, In, Out, Syn1, count, dim, ws, neg, t, min_count, ns_exponent, seed, dm, dm_mean, hs, lr, epochs):
        self.min_count, self.t, self.ns_exponent, self.lr, self.epochs = int(min_count), float(t), float(ns_exponent), float(lr), int(epochs)
        self.dm, self.dm_mean, self.hs = int(bool(int(dm))), int(bool(int(dm_mean))), bool(hs)
        self.dim, self.neg, self.ws, self.seed = _check_hyper(dim, neg, ws, seed, 'dim', self.hs)
        if self.t < 0 or self.ns_exponent not in NS_EXPONENTS:
            raise ValueError(f't must be >= 0 and ns_exponent one of {NS_EXPONENTS}')
        self.count = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
        if self.count.ndim != 1 or self.count.size < 1 or (self.count < 0).any():
            raise ValueError('count: expected non-negative int64 [n_aids], n_aids >= 1')
        self.n_aids = int(self.count.size)
        self.huffman = None                  # the HuffmanTables, built at the first inference
        for name, M, wanted in (('Out', Out, True), ('In', In, bool(self.dm)), ('Syn1', Syn1, self.hs)):
            if M is None:
                if wanted:
                    raise ValueError(f'{name}: this model (dm = {self.dm}, hs = {self.hs}) needs it')
                continue
            rows = None if name == 'Syn1' else self.n_aids
            if len(M.shape) != 2 or M.shape[1] != self.dim or (rows is not None and M.shape[0] != rows) or 'float32' not in str(M.dtype):
                raise ValueError(f'{name}: expected float32 [{"n_inner" if rows is None else rows}, {self.dim}]')
        self.In, self.Out, self.Syn1 = (In if self.dm else None), Out, (Syn1 if self.hs else None)
        self._engines = {}                   # device -> (engine, device tables)

    @property
    def variant(self):
        return CBOW_MEAN if self.dm_mean else CBOW_SUM

    def hyper(self):
        """the hyper-parameters as a plain dict (what ``model.json`` holds)"""
        return {k: getattr(self, k) for k in self.HYPER}

    def host(self, name):
        """table ``name`` as a NumPy array (None when the model has none)"""
        M = getattr(self, name)
        return None if M is None else (M.detach().cpu().numpy() if hasattr(M, 'detach') else np.asarray(M))

    def engine(self, dev):
        """``(SkipGramEngine, {name: device tensor})`` of this model on ``dev``, built once per device: the 0 / 2^32 - 1 keep
        table, the training corpus's negative table and Huffman tables, and the model tables as contiguous device tensors."""
        import torch
        if dev not in self._engines:
            _, keep_q, weight = _tables_of_counts(self.count, self.min_count, self.t, self.ns_exponent)
            keep = np.where(keep_q != 0, _U32_MAX, 0).astype(np.uint32)
            if self.hs and self.huffman is None:
                self.huffman = huffman_tables(self.count, self.min_count)
            if self.hs and tuple(self.Syn1.shape) != (self.huffman.n_inner, self.dim):
                raise ValueError(f'Syn1: expected float32 [{self.huffman.n_inner}, {self.dim}] for these counts')
            eng = SkipGramEngine(self.n_aids, self.dim, self.ws, self.neg, keep, weight, seed=self.seed, device=dev,
                                 hs=self.huffman if self.hs else None)
            tabs = {}
            for name in ('In', 'Out', 'Syn1'):
                M = getattr(self, name)
                if M is not None:
                    M = M if hasattr(M, 'detach') else torch.from_numpy(np.ascontiguousarray(M))
                    tabs[name] = M.detach().to(eng.dev).contiguous()
            self._engines[dev] = (eng, tabs)
        return self._engines[dev]


def doc2vec_model(In, Out, Syn1, count, **hyper):
    """The :class:`Doc2VecModel` of arrays saved earlier: ``hyper`` holds every name of ``Doc2VecModel.HYPER``."""
    missing = [k for k in Doc2VecModel.HYPER if k not in hyper]
    if missing or len(hyper) != len(Doc2VecModel.HYPER):
        raise ValueError(f'hyper-parameters: expected exactly {Doc2VecModel.HYPER}, missing {missing}')
    return Doc2VecModel(In, Out, Syn1, count, **hyper)


def infer_rates(alpha, min_alpha, passes):
    """float32 [passes]: ``alpha - (alpha - min_alpha) * p / max(passes - 1, 1)`` in float64, then rounded: the linear decay
    of gensim's ``infer_vector`` from ``alpha`` in pass 0 to ``min_alpha`` in the last pass (one pass runs at ``alpha``)."""
    passes, alpha, min_alpha = int(passes), float(alpha), float(min_alpha)
    if not 1 <= passes <= MAX_INFER_PASSES:
        raise ValueError(f'passes must be in [1, {MAX_INFER_PASSES}] (got {passes})')
    if not (np.isfinite(alpha) and np.isfinite(min_alpha)) or alpha <= 0 or min_alpha < 0 or min_alpha > alpha:
        raise ValueError(f'expected 0 <= min_alpha <= alpha, alpha > 0 (got alpha {alpha}, min_alpha {min_alpha})')
    return np.array([alpha - (alpha - min_alpha) * p / max(passes - 1, 1) for p in range(passes)], dtype=np.float64).astype(np.float32)


def infer_job(model, dev, tok_aid, tok_off, rates, Doc, loss=None, sess_key=None, order=None, neg_out=None, radius_out=None,
              variant=None):
    """The ``otto_sgns_infer_job`` of one launch on ``dev``'s current stream: ``tok_aid`` int32 [T] / ``tok_off`` int64 [S+1] as
    the plan left them, ``rates`` float32 [passes], ``Doc`` float32 [S, dim] out; every tensor contiguous on ``dev``."""
    eng, tabs = model.engine(dev)
    p = lambda t, what: _lib.ptr(t, dev, what)
    hs = eng.hs is not None
    return _lib.SgnsInferJob(
        p(tok_aid, 'tok_aid'), p(tok_off, 'tok_off'), int(tok_aid.numel()), int(tok_off.numel()) - 1, p(sess_key, 'sess_key'),
        p(order, 'order'), p(tabs.get('In'), 'In'), p(tabs['Out'], 'Out'), p(tabs.get('Syn1'), 'Syn1'), model.n_aids,
        eng.n_inner if hs else 0, model.dim, model.neg, model.ws, ARCH_PVDM if model.dm else ARCH_DBOW,
        model.variant if variant is None else int(variant), len(rates), (C.c_float * MAX_INFER_PASSES)(*[float(r) for r in rates]),
        model.seed, eng.table, p(eng._path_off, 'path_off') if hs else None, p(eng._path_node, 'path_node') if hs else None,
        p(eng._code, 'code') if hs else None, p(Doc, 'Doc'), p(loss, 'loss'), p(neg_out, 'neg_out'), p(radius_out, 'radius_out'),
        _lib.stream(dev))


def infer_doc2vec(aid, sess_off, model, passes=None, alpha=None, min_alpha=1e-4, sess_key=None, length_order=True, neg_out=None,
                  radius_out=None, variant=None):
    """Session vectors for sessions the model was not trained on (SPEC-DOC2VEC-INFER): ``aid`` int32 [E] sorted by
    (session, ts) and ``sess_off`` int64 [S+1], device tensors as :func:`train_doc2vec` takes them; ``model`` a
    :class:`Doc2VecModel`, which stays as it is. ``passes`` defaults to the model's ``epochs``, ``alpha`` to its ``lr``;
    the rates are :func:`infer_rates`. ``sess_key``: int64 / uint64 [S], the session ids that key the initial row and every
    draw (default: the row index); with it a session's vector is the same bytes in whatever batch it arrives. Events whose
    aid the model does not know are dropped; nothing is sub-sampled. Returns ``(Doc', loss)``: float32 [S, dim] and
    float64 [S, 2] (the session's loss sum in the first and in the last pass) on the device; the call does not synchronise.

    ``length_order``: sessions are handed to the lane groups longest first (sorted on the device); the result does not
    depend on it. ``variant``: ``CBOW_SUM`` / ``CBOW_MEAN`` / ``CBOW_FASTTEXT`` for PV-DM in place of the model's ``dm_mean``.
    ``neg_out`` int32 [passes, T, neg] / ``radius_out`` uint8 [passes, T]: the sampler's choices (tests).
    ``ValueError`` for bad arguments, raised before the device is touched."""
    import torch
    if not isinstance(model, Doc2VecModel):
        raise ValueError('model: expected a Doc2VecModel (train_doc2vec(..., return_model=True) or doc2vec_model(...))')
    rates = infer_rates(model.lr if alpha is None else alpha, min_alpha, model.epochs if passes is None else passes)
    P = len(rates)
    if variant is not None and variant not in (CBOW_SUM, CBOW_MEAN, CBOW_FASTTEXT):
        raise ValueError(f'unknown variant {variant}')
    for name, t in (('aid', aid), ('sess_off', sess_off)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f'{name}: expected a 1-d tensor')
    S = int(sess_off.numel()) - 1
    if S < 0:
        raise ValueError('sess_off: expected int64 [S+1]')
    if sess_key is not None:
        if not isinstance(sess_key, torch.Tensor):
            k = np.asarray(sess_key)
            if k.dtype.kind not in 'iu':
                raise ValueError('sess_key: expected integers')
            sess_key = torch.from_numpy(np.ascontiguousarray(k.astype(np.uint64)).view(np.int64))
        if sess_key.dtype != torch.int64 or tuple(sess_key.shape) != (S,):
            raise ValueError(f'sess_key: expected int64 (or uint64 viewed as int64) [{S}]')
    dev = _lib.rocm_device(aid.device, 'infer_doc2vec')
    eng, tabs = model.engine(dev)
    plan = eng.plan(aid, sess_off, 0)                      # the keep table holds 0 and 2^32 - 1: in-vocabulary events, in order
    T = plan.T
    for name, w, n in (('neg_out', neg_out, P * T * model.neg), ('radius_out', radius_out, P * T)):
        if w is not None and (w.dtype != (torch.int32 if name == 'neg_out' else torch.uint8) or w.numel() < n):
            raise ValueError(f'{name}: room for {n} entries of its type needed')
    with torch.cuda.device(dev):
        Doc = torch.empty(S, model.dim, dtype=torch.float32, device=dev)
        loss = torch.empty(S, 2, dtype=torch.float64, device=dev)
        order = None
        if length_order and S > 1:
            order = torch.argsort(plan.tok_off[1:] - plan.tok_off[:-1], descending=True, stable=True)
        if sess_key is not None:
            sess_key = sess_key.to(dev).contiguous()
        job = infer_job(model, dev, plan.tok_aid, plan.tok_off, rates, Doc, loss, sess_key, order, neg_out, radius_out, variant)
        _lib.call('otto_sgns_infer', dev, C.byref(job), stream=False)
    return Doc, loss


def train(aid, sess_off, n_aids, dim=32, ws=10, neg=40, epochs=5, lr=0.05, t=1e-4, min_count=1, ns_exponent=0.5, seed=0,
          mode=HOGWILD, tokens_per_launch=1 << 24, device=None, hs=False):
    """Train SGNS aid embeddings. ``aid`` int32 [E] sorted by (session, ts) and ``sess_off`` int64 [S+1], device tensors.
    Returns ``(In, Out, losses)``: the float32 [n_aids, dim] tables on the device and the per-epoch mean loss per pair
    target (loss sum / (pairs * (1 + neg))). The rate of a launch is :func:`learning_rate` at the source event of the
    launch's first token.

    ``hs=True`` (SPEC-SGNS-HS): every pair also walks the Huffman path of its context on a third table ``Syn1``
    float32 [max(V - 1, 1), dim], zero-initialised. The mean loss then divides by ``pairs * (1 + neg)`` plus the sum of
    the path lengths of the pairs' contexts (computed on the device from the plan), so it stays a mean per target.
    The return value becomes ``(In, Out, losses, Syn1)``: the fourth entry exists only with ``hs=True``."""
    _, In, Out, losses, Syn1 = _train_loop(
        lambda eng, plan, t0, t1, In, Out, rate, Syn1, Doc: eng.step(plan, t0, t1, In, Out, rate, mode, Syn1=Syn1),
        lambda eng, plan: plan.P * (1 + int(neg)) + eng.path_targets(plan), False,
        aid, sess_off, n_aids, dim, ws, neg, epochs, lr, t, min_count, ns_exponent, seed, tokens_per_launch, device, hs)
    return (In, Out, losses, Syn1) if hs else (In, Out, losses)


def save_vec(path, In, count, fmt='%.9g'):
    """word2vec text format of the input vectors: header ``<n_vocab> <dim>``, then one line per aid with ``count > 0`` (the caller
    zeroes the counts below ``min_count``), ordered by count descending, then aid ascending: the aid and ``dim`` values.
    Returns the aid order."""
    In = np.asarray(In, dtype=np.float32)
    count = np.asarray(count)
    order = np.lexsort((np.arange(len(count)), -count.astype(np.int64)))
    order = order[count[order] > 0]
    with open(path, 'w') as fh:
        fh.write(f'{len(order)} {In.shape[1]}\n')
        for a in order:
            fh.write(str(int(a)) + ' ' + ' '.join(fmt % float(v) for v in In[a]) + '\n')
    return order


def load_vec(path):
    """``(aids int64 [n], vectors float32 [n, d])`` of a word2vec text file."""
    with open(path) as fh:
        n, d = (int(x) for x in fh.readline().split())
        aids = np.empty(n, dtype=np.int64)
        vec = np.empty((n, d), dtype=np.float32)
        for i in range(n):
            parts = fh.readline().split()
            aids[i] = int(parts[0])
            vec[i] = np.array(parts[1:], dtype=np.float64)
    return aids, vec
