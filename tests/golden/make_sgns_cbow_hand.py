"""Writes tests/golden/sgns_cbow_hand.json: one PV-DM centre of SPEC-DOC2VEC (which contains SPEC-CBOW: the same inputs plus
the doc row) worked out at d = 4 in scalar Python (math, lists), sharing no code with tests/sgns_cbow_restatement.py.

One session [aid 0, aid 1, aid 2], ws = 1, t = 0, neg = 0, the tree of tests/golden/make_sgns_hs_hand.py (counts
[4, 1, 2, 1, 2]; the path of aid 1 is [3, 2, 1, 0] with code 0b1011). The launch holds centre token 1 alone (aid 1, left = 1,
two contexts):
    inputs   In[0], In[2], Doc[0]  (pair order, the doc row last), n = 3
    h        ((In[0] + In[2]) + Doc[0]), divided by 3 for MEAN and FASTTEXT
    targets  the path of the CENTRE's aid 1 on Syn1 with labels 1 - bit = [0, 0, 1, 0], then Out[1] with label 1
    u        grad (SUM, FASTTEXT) or grad / 3 (MEAN); In[0] += u, In[2] += u, Doc[0] += u
No row repeats, so the sequential and the batch step give the same tables. `after` holds the three variants.

    python tests/golden/make_sgns_cbow_hand.py
"""
import json
import math
import os
import struct

COUNT = [4, 1, 2, 1, 2]
PATH_OFF, PATH_NODE = [0, 1, 5, 7, 11, 14], [3, 3, 2, 1, 0, 3, 2, 3, 2, 1, 0, 3, 2, 1]
CODE = [0, 11, 1, 3, 7]
D, LR, SEED, EPOCH = 4, 0.05, 3, 0
AID, SESS_OFF = [0, 1, 2], [0, 3]
IN = [[0.25, -0.125, 0.0625, 0.1875], [-0.1875, 0.25, 0.125, -0.0625], [0.125, 0.125, -0.25, 0.0625],
      [-0.0625, -0.1875, 0.1875, 0.25], [0.03125, 0.0625, -0.03125, 0.125]]
OUT = [[0.125, 0.0625, -0.0625, 0.25], [-0.25, 0.125, 0.1875, -0.125], [0.0625, -0.1875, 0.125, 0.0625],
       [0.1875, 0.25, -0.125, -0.0625], [-0.125, 0.03125, 0.0625, 0.1875]]
SYN1 = [[0.5, -0.25, 0.125, 0.0625], [-0.125, 0.375, 0.25, -0.5], [0.0625, 0.125, -0.375, 0.25], [0.25, 0.5, -0.0625, -0.125]]
DOC = [[0.3125, -0.0625, 0.1875, -0.25]]


def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


lr = f32(LR)
after = {}
for variant, mean_h, mean_u in (('sum', False, False), ('mean', True, True), ('fasttext', True, False)):
    In, Out, Syn1, Doc = ([row[:] for row in M] for M in (IN, OUT, SYN1, DOC))
    h = [(IN[0][i] + IN[2][i]) + DOC[0][i] for i in range(D)]
    if mean_h:
        h = [v / 3.0 for v in h]
    grad, loss = [0.0] * D, 0.0
    # Syn1[3] label 0, Syn1[2] label 0, Syn1[1] label 1, Syn1[0] label 0, then Out[1] label 1
    for tab, t, label in ((Syn1, 3, 0.0), (Syn1, 2, 0.0), (Syn1, 1, 1.0), (Syn1, 0, 0.0), (Out, 1, 1.0)):
        o = tab[t][:]
        x = sum(h[i] * o[i] for i in range(D))
        g = lr * (label - sigmoid(x))
        loss += -math.log(sigmoid(x)) if label == 1.0 else -math.log(sigmoid(-x))
        for i in range(D):
            grad[i] += g * o[i]
        tab[t] = [f32(o[i] + g * h[i]) for i in range(D)]
    u = [v / 3.0 for v in grad] if mean_u else grad
    In[0] = [f32(IN[0][i] + u[i]) for i in range(D)]
    In[2] = [f32(IN[2][i] + u[i]) for i in range(D)]
    Doc[0] = [f32(DOC[0][i] + u[i]) for i in range(D)]
    after[variant] = dict(In=In, Out=Out, Syn1=Syn1, Doc=Doc, loss=loss)

out = dict(count=COUNT, min_count=1, n_inner=4, path_off=PATH_OFF, path_node=PATH_NODE, code=CODE, aid=AID, sess_off=SESS_OFF, d=D,
           ws=1, neg=0, seed=SEED, epoch=EPOCH, lr=LR, In=IN, Out=OUT, Syn1=SYN1, Doc=DOC, t0=1, t1=2, after=after)
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sgns_cbow_hand.json')
with open(path, 'w') as fh:
    json.dump(out, fh, indent=1)
print('wrote', path, {k: v['loss'] for k, v in after.items()})
