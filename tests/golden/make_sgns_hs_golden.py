"""Writes tests/golden/sgns_hs_golden.npz: the purity of the restatement's sequential hs + ns trainer
(tests/sgns_hs_restatement.py, SPEC-SGNS-HS) on the planted-cluster sessions of tests/sgns_inputs.py for five seeds
(CPU only, well under a minute per seed).

    python tests/golden/make_sgns_hs_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import sgns_hs_restatement as hr                                # noqa: E402
import sgns_inputs as si                                        # noqa: E402
from otto_amd.gensim_fasttext import skipgram as sg            # noqa: E402

_, _, cluster = si.planted_sessions()
purity, losses = [], []
for seed in si.GOLDEN_SEEDS:
    In, _, _, ls = hr.train_sequential_hs(seed, sg.vocab_tables, sg.init_tables, sg.learning_rate)
    purity.append(si.purity_from_ids(si.knn_numpy(In, 10), cluster))
    losses.append(ls)
    print('seed', seed, 'purity', purity[-1], 'losses', ls, flush=True)
purity = np.array(purity)
assert purity.min() >= 0.5, f'planted structure too weak: {purity}'
np.savez(os.path.join(HERE, 'sgns_hs_golden.npz'), seeds=np.array(si.GOLDEN_SEEDS), purity=purity, losses=np.array(losses))
print('wrote sgns_hs_golden.npz', purity)
