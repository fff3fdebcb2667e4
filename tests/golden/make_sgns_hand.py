"""Writes tests/golden/sgns_hand.json: SPEC-SGNS worked through on two sessions (3 and 2 tokens), 5 aids (one without an
event), d = 4, ws = 1, neg = 1, t = 0 -- in scalar Python (ints, math, lists), sharing no code with
tests/sgns_restatement.py. One sequential step and one batch step over all tokens from the same start tables.

    python tests/golden/make_sgns_hand.py
"""
import json
import math
import os
import struct

MASK = 0xFFFFFFFFFFFFFFFF
AID = [0, 1, 2, 3, 1]
SESS_OFF = [0, 3, 5]
N_AIDS, D, WS, NEG, SEED, EPOCH, LR = 5, 4, 1, 1, 11, 0, 0.05
IN = [[0.25, -0.125, 0.0625, 0.1875], [-0.1875, 0.25, 0.125, -0.0625], [0.125, 0.125, -0.25, 0.0625],
      [-0.0625, -0.1875, 0.1875, 0.25], [0.03125, 0.0625, -0.03125, 0.125]]
OUT = [[0.125, 0.0625, -0.0625, 0.25], [-0.25, 0.125, 0.1875, -0.125], [0.0625, -0.1875, 0.125, 0.0625],
       [0.1875, 0.25, -0.125, -0.0625], [-0.125, 0.03125, 0.0625, 0.1875]]


def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def splitmix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


# vocabulary: counts, t = 0 (every aid with an event is always kept), weights floor(sqrt(count) * 2^16)
count = [0] * N_AIDS
for a in AID:
    count[a] += 1
keep_q = [0xFFFFFFFF if c > 0 else 0 for c in count]
weight = [int(math.floor(math.sqrt(c) * 65536.0)) if c > 0 else 0 for c in count]
cum, run = [], 0
for w in weight:
    run += w
    cum.append(run)
total = cum[-1]

base = splitmix(SEED ^ ((EPOCH * 0xD1342543DE82EF95) & MASK))
event_key = [splitmix(base ^ ((e * 0xA0761D6478BD642F) & MASK)) for e in range(len(AID))]


def stream_key(e, stream, w):
    return splitmix(event_key[e] ^ ((((stream << 20) | w) * 0xE7037ED1A0B428DB) & MASK))


# plan: everything is kept (keep_q = 2^32 - 1 >= any 32-bit draw); radius 1 + floor(hi32 * 1 / 2^32) = 1
kept = [keep_q[AID[e]] != 0 and (stream_key(e, 1, 0) >> 32) <= keep_q[AID[e]] for e in range(len(AID))]
assert all(kept)
tok_off = SESS_OFF
radius = [1 + (((stream_key(e, 2, 0) >> 32) * WS) >> 32) for e in range(len(AID))]
assert radius == [1] * 5
# contexts at offsets -1, +1 clipped: token 0: [1]; 1: [0, 2]; 2: [1]; 3: [4]; 4: [3]
contexts = [[1], [0, 2], [1], [4], [3]]
tok_left = [0, 1, 1, 0, 1]
pair_off = [0, 1, 3, 4, 5, 6]

pairs = []          # (centre token, context aid, negative aid)
for c in range(5):
    for k, ct in enumerate(contexts[c]):
        ctx = AID[ct]
        negative = (ctx + 1) % N_AIDS
        for att in range(16):
            kk = stream_key(c, 3, (k << 10) | (0 << 4) | att)
            u = (kk * total) >> 64
            pick = 0
            while cum[pick] <= u:          # the first aid whose cumulative weight exceeds u
                pick += 1
            if pick != ctx:
                negative = pick
                break
        pairs.append((c, ctx, negative))
lr = f32(LR)


def sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


def sequential():
    In = [row[:] for row in IN]
    Out = [row[:] for row in OUT]
    loss = 0.0
    for c in range(5):
        h = In[AID[c]][:]
        for (cc, ctx, ngt) in pairs:
            if cc != c:
                continue
            grad = [0.0] * D
            for label, t in ((1.0, ctx), (0.0, ngt)):
                o = Out[t][:]
                x = sum(h[i] * o[i] for i in range(D))
                g = lr * (label - sigmoid(x))
                loss += -math.log(sigmoid(x)) if label == 1.0 else -math.log(sigmoid(-x))
                for i in range(D):
                    grad[i] += g * o[i]
                Out[t] = [f32(o[i] + g * h[i]) for i in range(D)]
            h = [h[i] + grad[i] for i in range(D)]
        In[AID[c]] = [f32(v) for v in h]
    return In, Out, loss


def batch():
    gin = [[0.0] * D for _ in range(N_AIDS)]
    gout = [[0.0] * D for _ in range(N_AIDS)]
    loss = 0.0
    for (c, ctx, ngt) in pairs:
        h = IN[AID[c]]
        for label, t in ((1.0, ctx), (0.0, ngt)):
            o = OUT[t]
            x = sum(h[i] * o[i] for i in range(D))
            g = lr * (label - sigmoid(x))
            loss += -math.log(sigmoid(x)) if label == 1.0 else -math.log(sigmoid(-x))
            for i in range(D):
                gin[AID[c]][i] += g * o[i]
                gout[t][i] += g * h[i]
    In = [[f32(IN[a][i] + gin[a][i]) for i in range(D)] for a in range(N_AIDS)]
    Out = [[f32(OUT[a][i] + gout[a][i]) for i in range(D)] for a in range(N_AIDS)]
    return In, Out, loss


seq_in, seq_out, seq_loss = sequential()
bat_in, bat_out, bat_loss = batch()
out = dict(aid=AID, sess_off=SESS_OFF, n_aids=N_AIDS, d=D, ws=WS, neg=NEG, seed=SEED, epoch=EPOCH, lr=LR, In=IN, Out=OUT,
           count=count, keep_q=keep_q, weight=weight, cum=cum, tok_aid=AID, tok_src=list(range(5)), tok_off=tok_off,
           radius=radius, tok_left=tok_left, pair_off=pair_off, ctx=[p[1] for p in pairs], neg_aid=[p[2] for p in pairs],
           sequential=dict(In=seq_in, Out=seq_out, loss=seq_loss), batch=dict(In=bat_in, Out=bat_out, loss=bat_loss))
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sgns_hand.json')
with open(path, 'w') as fh:
    json.dump(out, fh, indent=1)
print('wrote', path, 'pairs', pairs)
