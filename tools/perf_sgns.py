"""Time the skip-gram negative-sampling trainer (csrc/otto_sgns.hip) at OTTO shape and print one JSON line.

Sessions from ``synth.generate_sessions`` (n_aids = 1,855,603), d = 32, ws = 10, neg = 40, t = 1e-4, the reference's
``models/fasttext/config.yaml``. hipEvents around each call, 1 warm-up, 5 repeats, median with min and max:

  plan     one epoch's plan over all events
  hogwild  one launch of up to 2^24 kept tokens: tokens/s, target-row updates/s and the algorithmic bytes per second
           against the 8 TB/s HBM peak. Per target 2 * 4d bytes of Out (read and written), per centre 2 * 4d bytes of In,
           per kept token 4 bytes of token id and 1 byte of radius; the ids of the drawn negatives are not counted.

``--hs`` times the same launch through ``otto_sgns_step_hs`` (SPEC-SGNS-HS: the Huffman path of every pair's context on
``Syn1`` in front of its 1 + neg targets; the reference's ``models/word2vec/config.yaml`` has ``window: 12``, so pass
``--ws 12``). It adds the mean path length per pair and, to the algorithmic bytes, 2 * 4d bytes of ``Syn1`` plus 4 bytes of
node id per path node per pair. Compare it with a run without ``--hs`` by alternating the two in one job, several processes
each; ``--skip-host`` leaves the host baseline out of such runs.

``--arch cbow | pvdm | dbow`` times one launch of ``otto_sgns_cbow_step`` (SPEC-CBOW, SPEC-DOC2VEC) on the same plan instead,
with ``--variant sum | mean | fasttext``. Its targets are 1 + neg (plus the centre's own path with ``--hs``) per trained
centre, not per pair; to the algorithmic bytes each input row (a context row of In, PV-DM's doc row) adds 2 * 4d bytes, read
and written once, and each context 4 bytes of token id. DBOW reads and writes one Doc row per session of the launch.
``--append`` adds the JSON line to ``--out`` instead of replacing the file, so that alternating runs collect in one .jsonl.

Host baseline, same run: vectorised NumPy batch steps of 4,096 centres over 2^16 tokens (the restatement's sequential loop is far too
slow to time). No fastText or gensim figure exists: neither library is installed where this project is built.
Needs a GPU; there is no fallback.

    python tools/perf_sgns.py [--sessions 2000000] [--tokens 16777216] [--hs] [--arch skipgram] [--variant mean] [--skip-host]
                              [--out profiles/sgns/perf_sgns.json] [--append]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
HBM_PEAK = 8.0e12     # bytes / s, MI355X data sheet


def _time(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def _host_batch_step(tok_aid, left, pair_off, In, Out, neg, lr, rng, lo, hi):
    """vectorised NumPy batch step over the centres [lo, hi); negatives uniform (the draw is not what is timed)"""
    npair = (pair_off[lo + 1:hi + 1] - pair_off[lo:hi]).astype(np.int64)
    centre = np.repeat(np.arange(lo, hi), npair)
    k = np.arange(len(centre)) - np.repeat(pair_off[lo:hi] - pair_off[lo], npair)
    lf = left[centre].astype(np.int64)
    ct = np.where(k < lf, centre - lf + k, centre + 1 + (k - lf))
    tgt = np.concatenate((tok_aid[ct][:, None], rng.integers(0, In.shape[0], (len(centre), neg))), axis=1)
    h = In[tok_aid[centre]]
    x = np.einsum('pd,ptd->pt', h, Out[tgt])
    label = np.zeros_like(x)
    label[:, 0] = 1.0
    g = lr * (label - 1.0 / (1.0 + np.exp(-x)))
    gin = np.einsum('pt,ptd->pd', g, Out[tgt])
    np.add.at(In, tok_aid[centre], gin)
    np.add.at(Out, tgt.reshape(-1), (g[:, :, None] * h[:, None, :]).reshape(-1, In.shape[1]))
    return len(centre)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=2_000_000)
    ap.add_argument('--tokens', type=int, default=1 << 24)
    ap.add_argument('--dim', type=int, default=32)
    ap.add_argument('--ws', type=int, default=10)
    ap.add_argument('--neg', type=int, default=40)
    ap.add_argument('--t', type=float, default=1e-4)
    ap.add_argument('--host-tokens', type=int, default=1 << 16)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--hs', action='store_true', help='time otto_sgns_step_hs: the Huffman path half next to the negatives')
    ap.add_argument('--arch', choices=('skipgram', 'cbow', 'pvdm', 'dbow'), default='skipgram',
                    help='cbow, pvdm, dbow: time otto_sgns_cbow_step on the same plan')
    ap.add_argument('--variant', choices=('sum', 'mean', 'fasttext'), default='mean')
    ap.add_argument('--skip-host', action='store_true', help='leave the NumPy host baseline out')
    ap.add_argument('--append', action='store_true', help='append the line to --out')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_sgns: no ROCm device visible (this tool does not fall back)')
    from otto_amd.gensim_fasttext import skipgram as sg
    from otto_amd.synth import generate_sessions
    dev = torch.device('cuda:0')
    ev = generate_sessions(args.sessions)
    aid = torch.from_numpy(ev.aid.astype(np.int32)).to(dev)
    sess_off = torch.from_numpy(ev.sess_off).to(dev)
    n_aids, d, E = ev.n_aids, args.dim, int(aid.numel())
    count, keep_q, weight = sg.vocab_tables(aid, n_aids, 1, args.t, 0.5)
    tables = None
    if args.hs:
        t0 = time.perf_counter()
        tables = sg.huffman_tables(count, 1)
        tree_s = time.perf_counter() - t0
    eng = sg.SkipGramEngine(n_aids, d, args.ws, args.neg, keep_q, weight, seed=1, device=dev, hs=tables)
    In_h, Out_h = sg.init_tables(n_aids, d, 1)
    In, Out = torch.from_numpy(In_h).to(dev), torch.from_numpy(Out_h).to(dev)
    # hs: Syn1 starts at zero in training; a launch over zeros would time rows that never change, so it starts as In does
    step_kw = {}
    if args.hs:
        step_kw['Syn1'] = torch.from_numpy(sg.init_tables(tables.n_inner, d, 2)[0]).to(dev)
    out = {'tool': 'perf_sgns', 'device': torch.cuda.get_device_name(0), 'sessions': args.sessions, 'events': E, 'n_aids': n_aids,
           'd': d, 'ws': args.ws, 'neg': args.neg, 't': args.t, 'warmup': args.warmup, 'repeats': args.repeats,
           'table_bytes_each': n_aids * d * 4, 'hs': bool(args.hs), 'arch': args.arch}
    if args.hs:
        out['huffman'] = {'V': tables.V, 'n_inner': tables.n_inner, 'max_len': tables.max_len, 'path_nodes': int(tables.path_node.size),
                          'host_tree_seconds': round(tree_s, 3)}
    out['plan'] = _time(lambda: eng.plan(aid, sess_off, 0), args.warmup, args.repeats)
    plan = eng.plan(aid, sess_off, 0)
    n_tok = min(args.tokens, plan.T)
    pairs = int(plan.pair_off[n_tok] - plan.pair_off[0])
    out.update(kept_tokens=plan.T, pairs=plan.P, launch_tokens=n_tok, launch_pairs=pairs)
    if args.arch != 'skipgram':
        out['variant'] = args.variant
        out['hogwild'] = _time_cbow(args, sg, eng, plan, n_tok, pairs, In, Out, step_kw, d)
        _emit(out, args.out, args.append)
        return
    hw = _time(lambda: eng.step(plan, 0, n_tok, In, Out, 0.05, sg.HOGWILD, **step_kw), args.warmup, args.repeats)
    sec = hw['median_ms'] * 1e-3
    path_rows = eng.path_targets(plan, 0, n_tok)
    targets = pairs * (1 + args.neg) + path_rows
    n_bytes = targets * 2 * 4 * d + n_tok * 2 * 4 * d + n_tok * 5 + path_rows * 4
    if args.hs:
        hw.update(path_rows=path_rows, mean_path_length_per_pair=round(path_rows / max(pairs, 1), 3))
    hw.update(tokens_per_s=round(n_tok / sec), target_rows_per_s=round(targets / sec), algorithmic_bytes=n_bytes,
              bytes_per_s=round(n_bytes / sec), share_of_hbm_peak=round(n_bytes / sec / HBM_PEAK, 4))
    out['hogwild'] = hw
    if args.skip_host:
        _emit(out, args.out, args.append)
        return
    m = min(args.host_tokens, plan.T)
    tok_aid, left = plan.tok_aid[:m + 64].cpu().numpy().astype(np.int64), plan.tok_left[:m + 64].cpu().numpy()
    pair_off = plan.pair_off[:m + 65].cpu().numpy()
    valid = m
    while valid and (pair_off[valid] - pair_off[valid - 1]) - left[valid - 1] + valid - 1 >= len(tok_aid):
        valid -= 1                                           # keep every context inside the copied head
    rng = np.random.default_rng(0)
    In_c, Out_c = In_h.copy(), Out_h.copy()
    t0 = time.perf_counter()
    host_pairs = 0
    for lo in range(0, valid, 4096):                         # 4,096 centres per batch step bound the gathered rows' memory
        host_pairs += _host_batch_step(tok_aid, left, pair_off, In_c, Out_c, args.neg, 0.05, rng, lo, min(lo + 4096, valid))
    hs = time.perf_counter() - t0
    out['host_numpy_batch_step'] = {'tokens': valid, 'pairs': host_pairs, 'seconds': round(hs, 3), 'tokens_per_s': round(valid / hs),
                                    'what': 'one run, one process, vectorised NumPy batch step on the host of the GPU machine; '
                                            'no fastText or gensim figure exists (neither is installed)'}
    _emit(out, args.out, args.append)


def _time_cbow(args, sg, eng, plan, n_tok, pairs, In, Out, step_kw, d):
    """one hogwild launch of otto_sgns_cbow_step over the first n_tok centres: the timing and the byte model of the docstring"""
    import torch
    arch = {'cbow': sg.ARCH_CBOW, 'pvdm': sg.ARCH_PVDM, 'dbow': sg.ARCH_DBOW}[args.arch]
    variant = {'sum': sg.CBOW_SUM, 'mean': sg.CBOW_MEAN, 'fasttext': sg.CBOW_FASTTEXT}[args.variant]
    S = int(plan.tok_off.numel()) - 1
    kw = dict(step_kw)
    if arch != sg.ARCH_CBOW:
        kw['Doc'] = torch.from_numpy(sg.init_doc(S, d, 1)).to(In.device)
    hw = _time(lambda: eng.step_cbow(plan, 0, n_tok, In, Out, 0.05, arch, variant, sg.HOGWILD, **kw), args.warmup, args.repeats)
    sec = hw['median_ms'] * 1e-3
    targets = eng.cbow_targets(plan, arch, 0, n_tok)
    sessions = int(((plan.tok_off[:-1] < n_tok) & (plan.tok_off[1:] > plan.tok_off[:-1])).sum().item())      # with a token in the launch
    if arch == sg.ARCH_DBOW:
        input_rows, id_bytes = sessions, n_tok * 4
    else:
        input_rows = pairs + (n_tok if arch == sg.ARCH_PVDM else 0)
        id_bytes = n_tok * 5 + pairs * 4
    n_bytes = targets * 2 * 4 * d + input_rows * 2 * 4 * d + id_bytes
    hw.update(targets=targets, input_rows=input_rows, sessions_in_launch=sessions, tokens_per_s=round(n_tok / sec),
              target_rows_per_s=round(targets / sec), algorithmic_bytes=n_bytes, bytes_per_s=round(n_bytes / sec),
              share_of_hbm_peak=round(n_bytes / sec / HBM_PEAK, 4))
    return hw


def _emit(out, path, append=False):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'a' if append else 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
