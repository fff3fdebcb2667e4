"""Time Doc2Vec inference (otto_sgns_infer, SPEC-DOC2VEC-INFER; csrc/otto_sgns.hip) at OTTO shape and print one JSON line.

The 2 M sessions of ``tools/perf_sgns.py`` (``synth.generate_sessions``, n_aids = 1,855,603), d = 32, ws = 10, neg = 40, the
model's 5 passes. All sessions are inferred in ONE launch: every event is a token (nothing is sub-sampled at inference), so the
launch does ``passes * events`` token steps. hipEvents around the entry point alone (the token plan and the length order are
made once, outside the timed region), 1 warm-up, ``--repeats`` repeats, the median with min and max:

  infer_length_order   sessions handed to the lane groups longest first (what ``infer_doc2vec`` does)
  infer_identity       the same launch without the order array
  train_hogwild        one hogwild training launch of the same arch over the first 2^24 kept tokens of the training plan
                       (``tools/perf_sgns.py --arch``), alternated with the two above in the same process

``ms_per_pass_per_2p24_tokens`` scales each inference time to one pass over 2^24 tokens, the unit of the training figure. The
model tables are initialised as training initialises ``In`` (a launch over the zeros of a fresh ``Out`` would time rows that
all hold the same value). Run it three times per arch with ``--append``. Needs a GPU; there is no fallback.

    python tools/perf_sgns_infer.py --arch pvdm|dbow [--sessions 2000000] [--passes 5] [--repeats 3]
                                    [--out profiles/sgns/perf_sgns_infer.jsonl] [--append]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def _time(fns, warmup, repeats):
    """{name: timing} of the launches in `fns`, alternated: one round runs each of them once"""
    import torch
    ms = {k: [] for k in fns}
    for r in range(warmup + repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[k].append(a.elapsed_time(b))
    return {k: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', choices=('pvdm', 'dbow'), required=True)
    ap.add_argument('--sessions', type=int, default=2_000_000)
    ap.add_argument('--train-tokens', type=int, default=1 << 24)
    ap.add_argument('--dim', type=int, default=32)
    ap.add_argument('--ws', type=int, default=10)
    ap.add_argument('--neg', type=int, default=40)
    ap.add_argument('--t', type=float, default=1e-4)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--append', action='store_true', help='append the line to --out')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('perf_sgns_infer: no ROCm device visible (this tool does not fall back)')
    from otto_amd import _lib
    from otto_amd.gensim_fasttext import skipgram as sg
    from otto_amd.synth import generate_sessions
    dev = torch.device('cuda:0')
    ev = generate_sessions(args.sessions)
    aid = torch.from_numpy(ev.aid.astype(np.int32)).to(dev)
    sess_off = torch.from_numpy(ev.sess_off).to(dev)
    n_aids, d, E, S = ev.n_aids, args.dim, int(aid.numel()), int(sess_off.numel()) - 1
    dm = args.arch == 'pvdm'
    In = torch.from_numpy(sg.init_tables(n_aids, d, 1)[0]).to(dev)
    Out = torch.from_numpy(sg.init_tables(n_aids, d, 2)[0]).to(dev)
    count = sg.vocab_tables(aid, n_aids, 1, args.t, 0.5)[0]
    model = sg.doc2vec_model(In if dm else None, Out, None, count, dim=d, ws=args.ws, neg=args.neg, t=args.t, min_count=1,
                             ns_exponent=0.5, seed=1, dm=int(dm), dm_mean=1, hs=False, lr=0.05, epochs=args.passes)
    # inference: the plan once, the order once, then the entry point alone
    ieng, _ = model.engine(dev)
    plan = ieng.plan(aid, sess_off, 0)
    tok_aid, tok_off, T = plan.tok_aid.clone(), plan.tok_off.clone(), plan.T
    lens = tok_off[1:] - tok_off[:-1]
    order = torch.argsort(lens, descending=True, stable=True)
    rates = sg.infer_rates(0.05, 1e-4, args.passes)
    Doc = torch.empty(S, d, dtype=torch.float32, device=dev)
    loss = torch.empty(S, 2, dtype=torch.float64, device=dev)

    def infer(use_order):
        job = sg.infer_job(model, dev, tok_aid, tok_off, rates, Doc, loss, None, order if use_order else None)
        _lib.call('otto_sgns_infer', dev, C.byref(job), stream=False)

    # training: the launch of tools/perf_sgns.py --arch on its own plan (sub-sampled with t), tables of its own
    _, keep_q, weight = sg.vocab_tables(aid, n_aids, 1, args.t, 0.5)
    teng = sg.SkipGramEngine(n_aids, d, args.ws, args.neg, keep_q, weight, seed=1, device=dev)
    tplan = teng.plan(aid, sess_off, 0)
    n_tok = min(args.train_tokens, tplan.T)
    tIn, tOut = In.clone(), torch.zeros_like(Out)
    tDoc = torch.from_numpy(sg.init_doc(S, d, 1)).to(dev)
    arch = sg.ARCH_PVDM if dm else sg.ARCH_DBOW
    res = _time({'infer_length_order': lambda: infer(True), 'infer_identity': lambda: infer(False),
                 'train_hogwild': lambda: teng.step_cbow(tplan, 0, n_tok, tIn, tOut, 0.05, arch, sg.CBOW_MEAN, sg.HOGWILD, Doc=tDoc)},
                args.warmup, args.repeats)
    steps = T * args.passes
    for k in ('infer_length_order', 'infer_identity'):
        res[k]['ms_per_pass_per_2p24_tokens'] = round(res[k]['median_ms'] * (1 << 24) / steps, 3)
        res[k]['token_steps_per_s'] = round(steps / (res[k]['median_ms'] * 1e-3))
    res['train_hogwild']['launch_tokens'] = n_tok
    res['train_hogwild']['ms_per_2p24_tokens'] = round(res['train_hogwild']['median_ms'] * (1 << 24) / n_tok, 3)
    out = {'tool': 'perf_sgns_infer', 'device': torch.cuda.get_device_name(0), 'arch': args.arch, 'sessions': S, 'events': E, 'tokens': T,
           'n_aids': n_aids, 'd': d, 'ws': args.ws, 'neg': args.neg, 'passes': args.passes, 'warmup': args.warmup, 'repeats': args.repeats,
           'longest_session': int(lens.max().item()), 'mean_loss_first_pass': round(float(loss[:, 0].sum().item()) / max(T * (1 + args.neg), 1), 6),
           'mean_loss_last_pass': round(float(loss[:, 1].sum().item()) / max(T * (1 + args.neg), 1), 6), **res}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
