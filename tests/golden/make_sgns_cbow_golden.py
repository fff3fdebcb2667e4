"""Writes tests/golden/sgns_cbow_golden.npz: the neighbour purity of the restatement's sequential trainer
(tests/sgns_cbow_restatement.py, SPEC-CBOW and SPEC-DOC2VEC) on the planted-cluster sessions of tests/sgns_inputs.py for five
seeds: of In for CBOW-mean (3 epochs), of In and Doc for PV-DM-mean and of Doc for DBOW (10 epochs each). A session's
cluster is its first aid's cluster. CPU only, a few minutes in all.

    python tests/golden/make_sgns_cbow_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import sgns_cbow_inputs as ci                                   # noqa: E402
import sgns_cbow_restatement as cr                              # noqa: E402
import sgns_inputs as si                                        # noqa: E402
from otto_amd.gensim_fasttext import skipgram as sg            # noqa: E402

aid, sess_off, cluster = si.planted_sessions()
doc_cluster = ci.doc_clusters(aid, sess_off, cluster)
out = {}
for name, arch, variant, epochs in ci.LEARN:
    aid_purity, doc_purity, losses = [], [], []
    for seed in si.GOLDEN_SEEDS:
        tabs, ls = cr.train_sequential(seed, arch, variant, epochs, sg.vocab_tables, sg.init_tables, sg.init_doc, sg.learning_rate)
        if arch != cr.DBOW:
            aid_purity.append(si.purity_from_ids(si.knn_numpy(tabs['In'], 10), cluster))
        if arch != cr.CBOW:
            doc_purity.append(si.purity_from_ids(ci.knn_gram(tabs['Doc'], 10), doc_cluster))
        losses.append(ls)
        print(name, 'seed', seed, 'aid purity', aid_purity[-1:], 'doc purity', doc_purity[-1:], 'losses', ls, flush=True)
    for kind, values in (('aid', aid_purity), ('doc', doc_purity)):
        if values:
            values = np.array(values)
            assert values.min() >= 0.5, f'{name}: planted structure too weak in the {kind} vectors: {values}'
            out[f'{name}_{kind}_purity'] = values
    out[f'{name}_losses'] = np.array(losses)
np.savez(os.path.join(HERE, 'sgns_cbow_golden.npz'), seeds=np.array(si.GOLDEN_SEEDS), **out)
print('wrote sgns_cbow_golden.npz', {k: v for k, v in out.items() if k.endswith('purity')})
