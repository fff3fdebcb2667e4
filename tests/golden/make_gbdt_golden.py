"""Writes tests/golden/gbdt_golden.npz: what tests/gbdt_restatement.py computes for one small seeded problem, to pin the
restatement itself (tests/test_gbdt_cpu.py compares a fresh run with it).

    python tests/golden/make_gbdt_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import gbdt_restatement as gr  # noqa: E402

PARAMS = dict(num_leaves=8, min_data_in_leaf=5, lambdarank_norm=True, learning_rate=0.2)


def compute():
    rng = np.random.default_rng(20231)
    X, label, query_off = gr.random_problem(rng, 40, 4, min_len=3, max_len=25)
    edges = [gr.fit_edges(X[:, f]) for f in range(4)]
    bins = gr.bin_rows(X, edges)
    grad, hess, _ = gr.lambdarank(np.zeros(X.shape[0]), label, query_off)
    q, exps = gr.quantize(grad, hess)
    res = gr.train(bins, label, query_off, edges, PARAMS, num_boost_round=3)
    out = dict(X=X, label=label, query_off=query_off, bins=bins, grad0=grad, hess0=hess, q0=q, exp0=np.array(exps),
               n_trees=np.array(len(res['trees'])), train_score=res['train_score'], train_leaf=res['train_leaf'])
    for k in ('split_feature', 'split_bin', 'default_left', 'left_child', 'right_child', 'threshold', 'leaf_value', 'leaf_count'):
        out[k] = np.concatenate([t[k] for t in res['trees']])
    return out


if __name__ == '__main__':
    np.savez_compressed(os.path.join(HERE, 'gbdt_golden.npz'), **compute())
    print('wrote gbdt_golden.npz')
