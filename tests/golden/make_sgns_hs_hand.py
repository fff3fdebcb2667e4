"""Writes tests/golden/sgns_hs_hand.json: SPEC-SGNS-HS worked through by hand on 5 aids, and one pair's update at d = 4 in
scalar Python (math, lists), sharing no code with tests/sgns_hs_restatement.py.

The tree, by hand. Counts by aid: [4, 1, 2, 1, 2]. Leaves by (count descending, aid ascending):
    leaf 0 = aid 0 (4), leaf 1 = aid 2 (2), leaf 2 = aid 4 (2), leaf 3 = aid 1 (1), leaf 4 = aid 3 (1);  V = 5
cnt = [4, 2, 2, 1, 1 | S, S, S, S] (S = sentinel), p1 = 4, p2 = 5. Each step takes min1 then min2: the leaf p1 if
cnt[p1] < cnt[p2], else the inner node p2 (a tie takes the inner node); min2 gets bit 1.
    a = 0: leaf 4 (1 < S), leaf 3 (1 < S)          -> node 5 = 2, bit[leaf 3] = 1
    a = 1: node 5 (leaf 2: 2 < 2 fails), leaf 2    -> node 6 = 4, bit[leaf 2] = 1
    a = 2: leaf 1 (2 < 4), node 6 (leaf 0: 4 < 4 fails) -> node 7 = 6, bit[node 6] = 1
    a = 3: leaf 0 (4 < 6), node 7 (no leaf left)   -> node 8 = 10 (the root), bit[node 7] = 1
Inner id = node - 5: the root is 3. Paths from the root, with the bit of the child taken below each path node:
    aid 0: [3]          bits 0        code 0b0    = 0
    aid 2: [3, 2]       bits 1 0      code 0b01   = 1      (bit j in bit position j: read right to left)
    aid 4: [3, 2, 1]    bits 1 1 1    code 0b111  = 7
    aid 1: [3, 2, 1, 0] bits 1 1 0 1  code 0b1011 = 11
    aid 3: [3, 2, 1, 0] bits 1 1 0 0  code 0b0011 = 3
Kraft: 1/2 + 1/4 + 1/8 + 1/16 + 1/16 = 1. Weighted length 4*1 + 2*2 + 2*3 + 1*4 + 1*4 = 22 = 2 + 4 + 6 + 10.

The pair: one session [aid 0, aid 1], ws = 1, t = 0, neg = 0; the launch holds centre token 0 alone, whose one pair has the
context aid 1: its path [3, 2, 1, 0] with labels 1 - bit = [0, 0, 1, 0] on Syn1, then Out[1] with label 1, then h += grad.
No row repeats, so the sequential and the batch step give the same tables.

    python tests/golden/make_sgns_hs_hand.py
"""
import json
import math
import os
import struct

COUNT = [4, 1, 2, 1, 2]
PATHS = {0: [3], 1: [3, 2, 1, 0], 2: [3, 2], 3: [3, 2, 1, 0], 4: [3, 2, 1]}
CODE = [0, 11, 1, 3, 7]
INNER_COUNT = [2, 4, 6, 10]
D, LR, SEED, EPOCH = 4, 0.05, 3, 0
AID, SESS_OFF = [0, 1], [0, 2]
IN = [[0.25, -0.125, 0.0625, 0.1875], [-0.1875, 0.25, 0.125, -0.0625], [0.125, 0.125, -0.25, 0.0625],
      [-0.0625, -0.1875, 0.1875, 0.25], [0.03125, 0.0625, -0.03125, 0.125]]
OUT = [[0.125, 0.0625, -0.0625, 0.25], [-0.25, 0.125, 0.1875, -0.125], [0.0625, -0.1875, 0.125, 0.0625],
       [0.1875, 0.25, -0.125, -0.0625], [-0.125, 0.03125, 0.0625, 0.1875]]
SYN1 = [[0.5, -0.25, 0.125, 0.0625], [-0.125, 0.375, 0.25, -0.5], [0.0625, 0.125, -0.375, 0.25], [0.25, 0.5, -0.0625, -0.125]]


def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


path_off, path_node = [0], []
for a in range(5):
    path_node += PATHS[a]
    path_off.append(len(path_node))
assert path_off == [0, 1, 5, 7, 11, 14]

lr = f32(LR)
centre, ctx = 0, 1
h = IN[centre][:]
grad = [0.0] * D
Syn1 = [row[:] for row in SYN1]
Out = [row[:] for row in OUT]
loss = 0.0
targets = [(Syn1, n, 1.0 - ((CODE[ctx] >> j) & 1)) for j, n in enumerate(PATHS[ctx])] + [(Out, ctx, 1.0)]
assert [t[2] for t in targets] == [0.0, 0.0, 1.0, 0.0, 1.0]
for tab, t, label in targets:
    o = tab[t][:]
    x = sum(h[i] * o[i] for i in range(D))
    g = lr * (label - sigmoid(x))
    loss += -math.log(sigmoid(x)) if label == 1.0 else -math.log(sigmoid(-x))
    for i in range(D):
        grad[i] += g * o[i]
    tab[t] = [f32(o[i] + g * h[i]) for i in range(D)]
In = [row[:] for row in IN]
In[centre] = [f32(h[i] + grad[i]) for i in range(D)]

out = dict(count=COUNT, min_count=1, V=5, n_inner=4, path_off=path_off, path_node=path_node, code=CODE, max_len=4,
           inner_count=INNER_COUNT, aid=AID, sess_off=SESS_OFF, d=D, ws=1, neg=0, seed=SEED, epoch=EPOCH, lr=LR, In=IN, Out=OUT,
           Syn1=SYN1, t0=0, t1=1, after=dict(In=In, Out=Out, Syn1=Syn1, loss=loss))
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sgns_hs_hand.json')
with open(path, 'w') as fh:
    json.dump(out, fh, indent=1)
print('wrote', path, 'loss', loss)
