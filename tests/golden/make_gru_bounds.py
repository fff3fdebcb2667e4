"""Writes tests/golden/gru_bounds.json: the bounds of the GRU4Rec tests, every one 4 x a distance measured between two
references on the CPU (the project's convention; the device is not involved).

  torch      float64 restatement (tests/gru_restatement.py) against torch.nn.GRU(bias=False, batch_first=True) + nn.Linear +
             autograd in float64, over the edge shapes: the largest relative distance of o and of the five gradients.
  adam       the restatement's dense Adam against torch.optim.Adam over three steps, float64.
  cases      per GPU-test input and quantity: the distance between the float32 and the float64 restatement. 4 x that is the
             band the device's float32 result must keep to the float64 restatement.
  train      the same for the parameters after three training steps.

    python tests/golden/make_gru_bounds.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gru_inputs as I                       # noqa: E402
import gru_restatement as R                  # noqa: E402

PATH = os.path.join(HERE, 'gru_bounds.json')
FACTOR = 4.0


def distance(a, b):
    """largest absolute difference relative to the largest reference value (0 where the reference is all zero and a too)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return 0.0
    d, m = float(np.abs(a - b).max()), float(np.abs(b).max())
    return d / m if m > 0 else d


def torch_grad(c):
    """o, the five gradients (item gradient dense) and the loss sum of a case by torch autograd in float64"""
    import torch
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c['P'].items()}
    De, H, B = c['De'], c['H'], len(c['seq_lo'])
    gru = torch.nn.GRU(De, H, bias=False, batch_first=True).double()
    lin = torch.nn.Linear(H, De).double()
    gru.weight_ih_l0, gru.weight_hh_l0 = torch.nn.Parameter(P[R.KEYS[1]]), torch.nn.Parameter(P[R.KEYS[2]])
    lin.weight, lin.bias = torch.nn.Parameter(P[R.KEYS[3]]), torch.nn.Parameter(P[R.KEYS[4]])
    E = P[R.KEYS[0]]
    outs = []
    for lo, n in zip(c['seq_lo'], c['seq_len']):
        rows = torch.tensor(c['aid'][lo:lo + n].astype(np.int64) + 1)
        h = gru(E[rows][None])[1][0, 0] if n else torch.zeros(H, dtype=torch.float64)
        outs.append(lin(h))
    o = torch.stack(outs) if B else torch.zeros((0, De), dtype=torch.float64)
    pos, neg = (torch.tensor(c[k].astype(np.int64) + 1) for k in ('target', 'neg'))
    x = (o * E[pos]).sum(-1) - (o * E[neg]).sum(-1)
    loss = -torch.log(R.GAMMA + torch.sigmoid(x))
    loss.mean().backward()
    grads = {R.KEYS[0]: E.grad, R.KEYS[1]: gru.weight_ih_l0.grad, R.KEYS[2]: gru.weight_hh_l0.grad, R.KEYS[3]: lin.weight.grad,
             R.KEYS[4]: lin.bias.grad}
    return o.detach().numpy(), {k: (np.zeros(c['P'][k].shape) if g is None else g.numpy()) for k, g in grads.items()}, float(loss.sum().detach())


def against_torch(c):
    """{quantity: distance} of the float64 restatement from torch on one case"""
    G, _, o = R.grad(c['P'], c['aid'], c['seq_lo'], c['seq_len'], c['target'], c['neg'])
    to, tg, _ = torch_grad(c)
    out = {'o': distance(o, to), 'encode': distance(R.encode(c['P'], c['aid'], c['seq_lo'], c['seq_len']), to)}
    out.update({k: distance(G[k], tg[k]) for k in R.KEYS})
    return out


def adam_against_torch(steps=3):
    """largest distance of the restatement's dense Adam from torch.optim.Adam over ``steps`` steps, float64"""
    import torch
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal((7, 5))
    grads = [rng.standard_normal((7, 5)) * 10.0 ** -q for q in range(steps)]
    tp = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([tp], lr=I.ADAM['lr'], betas=I.ADAM['betas'], eps=I.ADAM['eps'])
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    worst = 0.0
    for t, g in enumerate(grads, 1):
        tp.grad = torch.tensor(g)
        opt.step()
        R.adam_dense(p, m, v, g, t=t, dtype=np.float64, **I.ADAM)
        worst = max(worst, distance(p, tp.detach().numpy()))
    return worst


def precision_distances(c):
    """{quantity: distance} between the float32 and the float64 restatement on one case"""
    a = (c['P'], c['aid'], c['seq_lo'], c['seq_len'], c['target'], c['neg'])
    G64, l64, o64 = R.grad(*a, dtype=np.float64)
    G32, l32, o32 = R.grad(*a, dtype=np.float32)
    out = {'o': distance(o32, o64)}
    out.update({k: distance(G32[k], G64[k]) for k in R.KEYS})
    return out


def train_distances(steps=3):
    c = I.training_corpus()
    a = (c['P'], c['aid'], c['sess_off'], c['n_aids'], c['batch'], I.ADAM['lr'], I.ADAM['betas'], I.ADAM['eps'], I.SEED, I.EPOCH, c['L'])
    s64, _ = R.train(*a, steps=steps, dtype=np.float64)
    s32, _ = R.train(*a, steps=steps, dtype=np.float32)
    return {k: distance(s32['p'][k], s64['p'][k]) for k in R.KEYS}


def _entry(d):
    return {'distance': d, 'band': FACTOR * d}


def measure():
    cases = I.cases()
    torch_d = max(max(against_torch(c).values()) for c in cases.values())
    adam_d = adam_against_torch()
    return {'factor': FACTOR,
            'torch': {'measured': torch_d, 'bound': FACTOR * torch_d},
            'adam': {'measured': adam_d, 'bound': FACTOR * adam_d},
            'cases': {name: {q: _entry(d) for q, d in precision_distances(c).items()} for name, c in cases.items()},
            'train': {q: _entry(d) for q, d in train_distances().items()}}


def load():
    with open(PATH) as fh:
        return json.load(fh)


if __name__ == '__main__':
    with open(PATH, 'w') as fh:
        json.dump(measure(), fh, indent=1, sort_keys=True)
    print(f'wrote {PATH}')
