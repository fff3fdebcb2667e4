"""Writes tfidf_script_golden.json: what the two prediction loops of the reference's own ``src/tfidf/inference.py`` give on
the corpora of ``tests/tfidf_inputs.py`` when they are fed the AID-direction similarity matrix, so that tests can compare
against them where the reference is not installed.

    python tests/golden/make_tfidf_golden.py /path/to/reference/src

The script is one ``__main__`` block that reads pickles, so it cannot be imported or run whole. Its lines 40-52 (routing
of the sessions, prediction columns) and 54-96 (the recency loop and the tf-idf loop) are read from the file, de-indented
and executed here over a frame built from the corpus, with ``similarity_matrix = cosine_similarity(X.T,
dense_output=False)`` in place of the session x session matrix of its line 37. A session whose last aid
is below 10 is not in the vocabulary and the script's ``aid2idx[...]`` raises ``KeyError``: such sessions are routed away
from the loop, the raise is checked on each of them, and they are recorded with kind ``key_error`` and their distinct
aids. Only data is stored: per corpus the kind and the prediction list of every session.
"""
import json
import logging
import os
import sys
import textwrap
from collections import defaultdict

import numpy as np
import pandas as pd
from sklearn.feature_extraction.text import TfidfVectorizer
from sklearn.metrics.pairwise import cosine_similarity
from tqdm import tqdm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tfidf_inputs as I  # noqa: E402

CORPORA = {'edges': None, 'common_aid': 11}


def script_lines(reference_src, first, last):
    """lines first..last (1-based, inclusive) of the script, de-indented"""
    with open(os.path.join(reference_src, 'tfidf', 'inference.py')) as f:
        lines = f.readlines()
    return textwrap.dedent(''.join(lines[first - 1:last]))


def run(reference_src, common_aid):
    (aid, typ, off), _ = I.sklearn_corpus(common_aid=common_aid)
    S = len(off) - 1
    sessions = [aid[int(off[s]):int(off[s + 1])].tolist() for s in range(S)]
    types = [typ[int(off[s]):int(off[s + 1])].tolist() for s in range(S)]
    vec = TfidfVectorizer()
    X = vec.fit_transform([' '.join(str(a) for a in s) for s in sessions])
    scope = {'np': np, 'pd': pd, 'json': json, 'logging': logging, 'tqdm': tqdm, 'defaultdict': defaultdict,
             'df_train_labels': pd.DataFrame({'aid': sessions, 'type': types}),
             'aid2idx': {int(a): i for a, i in vec.vocabulary_.items()},
             'idx2aid': {i: int(a) for a, i in vec.vocabulary_.items()},
             'similarity_matrix': cosine_similarity(X.T, dense_output=False)}
    exec(script_lines(reference_src, 40, 52), scope)
    df = scope['df_train_labels']
    out_of_vocabulary = (df['prediction_type'] == 'tfidf') & df['aid'].apply(lambda a: a[-1] not in scope['aid2idx'])
    loops = script_lines(reference_src, 54, 96)
    for idx in df.index[out_of_vocabulary]:                  # the script's own loop raises on each of them
        probe = dict(scope, df_train_labels=df.loc[[idx]].copy())
        try:
            exec(loops, probe)
        except KeyError:
            continue
        raise AssertionError(f'session {idx}: the script did not raise')
    df.loc[out_of_vocabulary, 'prediction_type'] = 'key_error'
    exec(loops, scope)
    df = scope['df_train_labels']
    rows = []
    for s in range(S):
        kind = df.at[s, 'prediction_type']
        if kind == 'key_error':
            rows.append([kind, [int(a) for a in np.unique(sessions[s])]])
        else:
            assert df.at[s, 'click_predictions'] == df.at[s, 'cart_predictions'] == df.at[s, 'order_predictions']
            rows.append([kind, [int(a) for a in df.at[s, 'click_predictions']]])
    return rows


def main(reference_src):
    logging.disable(logging.CRITICAL)
    out = {name: run(reference_src, common) for name, common in CORPORA.items()}
    path = os.path.join(HERE, 'tfidf_script_golden.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    for name, rows in out.items():
        print(name, len(rows), 'sessions:', {k: sum(1 for r in rows if r[0] == k) for k in ('recency_weight', 'tfidf', 'key_error')})
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
