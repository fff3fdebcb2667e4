"""``python trainer.py <config_path relative to settings.MODELS>``: the reference's ``src/gensim_fasttext/trainer.py``.

Reads the reference's ``models/fasttext/config.yaml`` (``model_name: FastText``) and ``models/word2vec/config.yaml``
(``model_name: Word2Vec``) and trains skip-gram negative-sampling aid embeddings on the device (SPEC-SGNS, DESIGN.md
section 3i). Sessions come from ``settings.DATA / 'train.pkl'`` and ``'test.pkl'`` through ``events.frame_to_events_device``
(the reference's fastText branch reads a ``sentences.txt`` made of the same two frames). Writes
``<model_directory>/aid_embeddings.npy`` (float32 [n_aids, dim], the input vectors) and ``aid_embeddings.vec`` (word2vec
text format, in-vocabulary aids by count descending then aid ascending). ``fasttext.bin`` / ``word2vec.model`` are not
written.

:func:`resolve` maps a config to one of three trainers. ``fasttext_args``, ``word2vec_args`` and ``train_args`` are the
skip-gram mapping and refuse everything else with ``ValueError``: ``model: cbow``, ``loss`` other than ``ns``, ``minn`` /
``maxn`` above 0 (fastText); ``sg: 0`` or ``negative: 0`` (Word2Vec, with or without ``hs: 1``: hierarchical softmax alone
is not built for skip-gram); ``Doc2Vec``. ``hs: 1`` with ``negative > 0`` (the reference's own Word2Vec file) trains
hierarchical softmax next to the negative-sampling part (SPEC-SGNS-HS), over the word2vec.c tree rather than gensim's
heap; that departure is logged once.

:func:`resolve` additionally takes fastText ``model: cbow`` and gensim ``sg: 0`` (SPEC-CBOW) and ``Doc2Vec`` (SPEC-DOC2VEC:
``dm: 1`` PV-DM, ``dm: 0`` PV-DBOW), where ``hs: 1`` may also stand alone (``negative: 0``). Doc2Vec is the one model that
yields a session vector: ``doc_embeddings.npy`` (float32 [S, dim]) and ``doc_sessions.npy`` (the session id of each row).
Still refused: ``dm_concat``, ``dbow_words``, ``dm_tag_count`` other than 1, sub-words, ``loss`` other than ``ns``.

``--save-model`` (``run(save_model=True)``) makes a Doc2Vec run also write what inference needs: ``out_embeddings.npy``,
``syn1.npy`` (with ``hs: 1``), ``aid_counts.npy`` and ``model.json`` (the hyper-parameters). ``--infer <frame.pkl|.parquet>``
(:func:`infer`) reads those files and embeds the frame's sessions, none of which the model has to have seen
(SPEC-DOC2VEC-INFER), into ``doc_embeddings_inferred.npy`` and ``doc_sessions_inferred.npy``.
"""
import argparse
import json
import logging
import pathlib

import numpy as np
import yaml

from .. import settings
from . import skipgram

_HS_WARNED = False


def fasttext_args(model_args):
    """The :func:`skipgram.train` keywords of a fastText ``model_args`` mapping (fastText's defaults where absent)."""
    a = dict(model_args)
    if a.get('model', 'skipgram') != 'skipgram':
        raise ValueError(f"model: {a.get('model')!r} is not built (only skipgram)")
    if a.get('loss', 'ns') != 'ns':
        raise ValueError(f"loss: {a.get('loss')!r} is not built (only ns)")
    if int(a.get('minn', 0)) > 0 or int(a.get('maxn', 0)) > 0:
        raise ValueError('sub-word n-grams (minn / maxn > 0) are not built')
    return dict(dim=int(a.get('dim', 100)), ws=int(a.get('ws', 5)), neg=int(a.get('neg', 5)), epochs=int(a.get('epoch', 5)),
                lr=float(a.get('lr', 0.05)), t=float(a.get('t', 1e-4)), min_count=int(a.get('minCount', 5)), ns_exponent=0.5,
                seed=int(a.get('seed', 0)))


def word2vec_args(model_args):
    """The :func:`skipgram.train` keywords of a gensim ``Word2Vec`` ``model_args`` mapping (gensim's defaults where
    absent)."""
    global _HS_WARNED
    a = dict(model_args)
    if int(a.get('sg', 0)) != 1:
        raise ValueError('sg: 0 (cbow) is not built (only skip-gram)')
    if int(a.get('negative', 5)) <= 0:
        raise ValueError('negative: 0 leaves hierarchical softmax alone, which is not built')
    if int(a.get('hs', 0)) and not _HS_WARNED:
        _HS_WARNED = True
        logging.warning('hs: 1 -- hierarchical softmax is trained next to the negative-sampling part, over the word2vec.c '
                        "tree (two cursors over the sorted counts) rather than gensim's heap")
    return dict(dim=int(a.get('vector_size', 100)), ws=int(a.get('window', 5)), neg=int(a['negative'] if 'negative' in a else 5),
                epochs=int(a.get('epochs', 5)), lr=float(a.get('alpha', 0.025)), t=float(a.get('sample', 1e-3)),
                min_count=int(a.get('min_count', 5)), ns_exponent=float(a.get('ns_exponent', 0.75)), seed=int(a.get('seed', 1)))


def hs_requested(config):
    """True when ``config`` (the whole YAML mapping) asks for hierarchical softmax: ``Word2Vec`` with ``hs: 1``."""
    model = config['model']
    return model['model_name'] == 'Word2Vec' and bool(int(dict(model.get('model_args') or {}).get('hs', 0)))


def train_args(config):
    """``config`` (the whole YAML mapping) -> the :func:`skipgram.train` keywords."""
    name = config['model']['model_name']
    if name == 'FastText':
        return fasttext_args(config['model']['model_args'])
    if name == 'Word2Vec':
        return word2vec_args(config['model']['model_args'])
    if name == 'Doc2Vec':
        raise ValueError('Doc2Vec is not built as skip-gram (resolve maps it to train_doc2vec)')
    raise ValueError('Invalid model_name')


def _objective(hs, neg):
    if not hs and neg <= 0:
        raise ValueError('negative: 0 without hs: 1 leaves nothing to train against')
    return dict(neg=max(neg, 0), hs=hs)


def _gensim_common(a):
    """What Word2Vec(sg=0) and Doc2Vec share: gensim's defaults where absent."""
    hs, neg = bool(int(a.get('hs', 0))), int(a['negative'] if 'negative' in a else 5)
    return dict(dim=int(a.get('vector_size', 100)), ws=int(a.get('window', 5)), epochs=int(a.get('epochs', 5)),
                lr=float(a.get('alpha', 0.025)), t=float(a.get('sample', 1e-3)), min_count=int(a.get('min_count', 5)),
                ns_exponent=float(a.get('ns_exponent', 0.75)), seed=int(a.get('seed', 1)), **_objective(hs, neg))


def resolve(config):
    """``config`` (the whole YAML mapping) -> ``(arch, kwargs)``: ``'skipgram'`` with the :func:`skipgram.train` keywords
    (the skip-gram mapping above, its refusals included), ``'cbow'`` with :func:`skipgram.train_cbow`'s, or ``'doc2vec'``
    with :func:`skipgram.train_doc2vec`'s. ``hs`` is among the keywords.

    fastText ``model: cbow`` is the FASTTEXT variant; gensim ``sg: 0`` takes ``cbow_mean`` (default 1); ``Doc2Vec`` takes
    ``dm`` (default 1) and ``dm_mean``, where an absent or null ``dm_mean`` means the mean (SPEC-DOC2VEC's build
    decision). ``hs: 1`` with ``negative: 0`` is accepted by the two new archs. Refused: ``dm_concat``, ``dbow_words``,
    ``dm_tag_count`` other than 1, sub-words, ``loss`` other than ``ns``, and no objective at all."""
    model = config['model']
    name, a = model['model_name'], dict(model.get('model_args') or {})
    if name == 'FastText' and a.get('model', 'skipgram') == 'cbow':
        kw = fasttext_args({**a, 'model': 'skipgram'})      # the same keywords and the same refusals (loss, sub-words)
        kw.update(_objective(False, kw['neg']), variant=skipgram.CBOW_FASTTEXT)
        return 'cbow', kw
    if name == 'Word2Vec' and int(a.get('sg', 0)) == 0:
        variant = skipgram.CBOW_MEAN if int(a.get('cbow_mean', 1)) else skipgram.CBOW_SUM
        return 'cbow', dict(_gensim_common(a), variant=variant)
    if name == 'Doc2Vec':
        if int(a.get('dm_concat', 0)):
            raise ValueError('dm_concat: 1 is not built')
        if int(a.get('dbow_words', 0)):
            raise ValueError('dbow_words: 1 is not built')
        if int(a.get('dm_tag_count', 1)) != 1:
            raise ValueError('dm_tag_count other than 1 is not built (one tag, the session, per document)')
        dm_mean = a.get('dm_mean')
        return 'doc2vec', dict(_gensim_common(a), dm=int(a.get('dm', 1)), dm_mean=1 if dm_mean is None else int(dm_mean))
    return 'skipgram', dict(train_args(config), hs=hs_requested(config))


MODEL_FILES = dict(In='aid_embeddings.npy', Out='out_embeddings.npy', Syn1='syn1.npy', count='aid_counts.npy', hyper='model.json')


def write_model(model, directory):
    """Write the files of ``--save-model`` (``aid_embeddings.npy`` is the run's own file and is not written again)."""
    directory = pathlib.Path(directory)
    np.save(directory / MODEL_FILES['Out'], model.host('Out'))
    if model.hs:
        np.save(directory / MODEL_FILES['Syn1'], model.host('Syn1'))
    np.save(directory / MODEL_FILES['count'], model.count)
    with open(directory / MODEL_FILES['hyper'], 'w') as fh:
        json.dump(model.hyper(), fh, indent=1, sort_keys=True)


def read_model(directory):
    """The :class:`skipgram.Doc2VecModel` of a directory that a ``--save-model`` run wrote."""
    directory = pathlib.Path(directory)
    with open(directory / MODEL_FILES['hyper']) as fh:
        hyper = json.load(fh)
    In = np.load(directory / MODEL_FILES['In']) if int(hyper['dm']) else None
    Syn1 = np.load(directory / MODEL_FILES['Syn1']) if hyper['hs'] else None
    return skipgram.doc2vec_model(In, np.load(directory / MODEL_FILES['Out']), Syn1, np.load(directory / MODEL_FILES['count']), **hyper)


def infer(config, df, device='cuda:0', passes=None, alpha=None, min_alpha=1e-4):
    """Embed the sessions of ``df`` (a frame, a list of frames, or the path of a ``.pkl`` / ``.parquet`` frame) with the
    Doc2Vec model that ``run(config, save_model=True)`` saved; returns ``(Doc', session ids, model_root_directory)`` and
    writes ``doc_embeddings_inferred.npy`` (float32 [S, dim]) and ``doc_sessions_inferred.npy``. The session id keys every
    draw, so a session's row does not depend on the frame it arrives in. Events whose aid the model does not know (never
    seen in training, below ``min_count``, or past its id space) are dropped."""
    if resolve(config)[0] != 'doc2vec':
        raise ValueError('infer needs a Doc2Vec config: no other model yields a session vector')
    from ..events import frame_to_events_device
    model_root_directory = pathlib.Path(settings.MODELS / config['persistence']['model_directory'])
    model = read_model(model_root_directory)
    if isinstance(df, (str, pathlib.Path)):
        import pandas as pd
        df = pd.read_parquet(df) if str(df).endswith('.parquet') else pd.read_pickle(df)
    ev = frame_to_events_device(df, device=device)
    aid = ev.aid
    if ev.n_aids > model.n_aids:                          # an aid past the model's id space is out of its vocabulary
        import torch
        known = aid < model.n_aids
        pos = torch.zeros(aid.numel() + 1, dtype=torch.int64, device=aid.device)
        pos[1:] = torch.cumsum(known, 0)
        aid, sess_off = aid[known].contiguous(), pos[ev.sess_off]
    else:
        sess_off = ev.sess_off
    ids = ev.session_ids
    Doc, _ = skipgram.infer_doc2vec(aid, sess_off, model, passes=passes, alpha=alpha, min_alpha=min_alpha, sess_key=ids)
    Doc, ids = Doc.cpu().numpy(), (ids.cpu().numpy() if hasattr(ids, 'cpu') else np.asarray(ids))
    np.save(model_root_directory / 'doc_embeddings_inferred.npy', Doc)
    np.save(model_root_directory / 'doc_sessions_inferred.npy', ids)
    logging.info(f'{len(ids)} session vectors inferred and saved to {model_root_directory}')
    return Doc, ids, model_root_directory


def run(config, df=None, device='cuda:0', n_aids=None, tokens_per_launch=1 << 24, save_model=False):
    """Train and write the files; returns ``(In, losses, model_root_directory)``. ``df``: a frame or a list of frames
    with ``session``, ``aid``, ``ts``, ``type`` (default: ``train.pkl`` + ``test.pkl`` under ``settings.DATA``).
    Doc2Vec also writes ``doc_embeddings.npy`` (float32 [S, dim]) and ``doc_sessions.npy`` (the session id of each row);
    the first entry of the result is then that session table, and PV-DBOW, which trains no aid vectors, writes no aid
    files. ``save_model=True`` (Doc2Vec alone; ``ValueError`` otherwise) also writes the files :func:`infer` reads."""
    arch, kw = resolve(config)                            # refusals come before any file or device is touched
    if save_model and arch != 'doc2vec':
        raise ValueError('save_model: only a Doc2Vec model is saved for inference')
    from ..events import frame_to_events_device
    model_root_directory = pathlib.Path(settings.MODELS / config['persistence']['model_directory'])
    model_root_directory.mkdir(parents=True, exist_ok=True)
    if df is None:
        import pandas as pd
        df = [pd.read_pickle(settings.DATA / 'train.pkl'), pd.read_pickle(settings.DATA / 'test.pkl')]
    ev = frame_to_events_device(df, device=device, n_aids=n_aids)
    logging.info(f'Sentences Dataset - sentences: {ev.n_sessions} - tokens: {ev.n_events}')
    Doc = model = None
    if arch == 'doc2vec':
        out = skipgram.train_doc2vec(ev.aid, ev.sess_off, ev.n_aids, tokens_per_launch=tokens_per_launch, return_model=save_model, **kw)
        Doc, In, _, losses = out[:4]
        model = out[-1] if save_model else None
    else:
        fn = skipgram.train_cbow if arch == 'cbow' else skipgram.train
        In, _, losses = fn(ev.aid, ev.sess_off, ev.n_aids, tokens_per_launch=tokens_per_launch, **kw)[:3]
    for ep, ls in enumerate(losses):
        logging.info(f'epoch {ep}: mean loss {ls:.6f}')
    In = In.cpu().numpy()
    if Doc is not None:
        Doc = Doc.cpu().numpy()
        np.save(model_root_directory / 'doc_embeddings.npy', Doc)
        ids = ev.session_ids
        np.save(model_root_directory / 'doc_sessions.npy', ids.cpu().numpy() if hasattr(ids, 'cpu') else np.asarray(ids))
    if Doc is None or kw['dm']:
        count, _, _ = skipgram.vocab_tables(ev.aid, ev.n_aids, kw['min_count'], kw['t'], kw['ns_exponent'])
        count[count < max(kw['min_count'], 1)] = 0
        np.save(model_root_directory / 'aid_embeddings.npy', In)
        skipgram.save_vec(model_root_directory / 'aid_embeddings.vec', In, count)
    if model is not None:
        write_model(model, model_root_directory)
    logging.info(f"{config['model']['model_name']} embeddings finished training and saved to {model_root_directory}")
    return (In if Doc is None else Doc), losses, model_root_directory


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('config_path', type=str)
    parser.add_argument('--save-model', action='store_true', help='Doc2Vec: also write the files --infer reads')
    parser.add_argument('--infer', type=str, default=None, metavar='FRAME', help='a .pkl or .parquet frame of sessions to embed '
                        'with the saved Doc2Vec model, instead of training')
    args = parser.parse_args()
    config = yaml.load(open(settings.MODELS / args.config_path, 'r'), Loader=yaml.FullLoader)
    if args.infer is not None:
        infer(config, args.infer)
    else:
        run(config, save_model=args.save_model)
