"""The TF-IDF similarity model of ``src/tfidf/inference.py`` on the device: every session is predicted either by the recency
branch (at least ``min_unique`` distinct aids) or by its distinct aids followed by the aids most similar to its last aid.

The reference indexes the session x session similarity matrix with the vocabulary index of the last aid and maps the
session numbers it finds back through the vocabulary. What is built here is what its comment and its
routing intend: the aid x aid cosine over the sessions (``similarity.similar_aids``). Differences kept on purpose: self is
excluded by id (the reference drops the first entry of the argsort), only aids with a positive similarity follow (the
reference's argsort fills up with unrelated aids of similarity 0), and a last aid below ``min_aid`` has no neighbours (the
reference raises ``KeyError``). As in the reference the three event types share one list, and the two halves of a list
are not de-duplicated against each other.

    python -m otto_amd.tfidf.inference validation --events val.parquet [--seed 42]
    python -m otto_amd.tfidf.inference submission --events test.parquet --out tfidf_submission.csv.gz
"""
import logging

from .. import _lib
from . import similarity

RECENCY_CURVE = (0.1, 1.0)                   # src/tfidf/inference.py:63-64: one curve for clicks and for carts / orders
TYPE_COEFFICIENT = (1.0, 6.0, 3.0)           # :54


def predictions(aid, typ, sess_off, n_aids, n_similar=49, n_pred=20, min_unique=20, min_aid=similarity.SKLEARN_MIN_AID):
    """Events ``aid`` int32 [E], ``typ`` uint8 [E], ``sess_off`` int64 [S + 1] on a ROCm device -> ``(pred int32 [S, n_pred]
    padded with -1, n int32 [S], recency bool [S])``. Sessions with at least ``min_unique`` distinct aids: the first
    ``n_pred`` of ``covisitation.candidates.recency_candidates`` (curve (0.1, 1), coefficients {0: 1, 1: 6, 2: 3}). Every
    other session: its distinct aids, ascending, then the ``n_similar`` aids most similar to its last aid
    (:func:`similarity.similar_aids` over the ``min_aid`` vocabulary), cut to ``n_pred``."""
    import torch
    from ..covisitation.candidates import recency_candidates
    dev = aid.device
    if dev.type != 'cuda':
        raise _lib.OttoError('tfidf.predictions needs tensors on a ROCm device (no CPU fallback)')
    n_similar, n_pred, min_unique = int(n_similar), int(n_pred), int(min_unique)
    if n_pred < 1 or min_unique < 1:
        raise ValueError('n_pred and min_unique must be positive')
    S = int(sess_off.numel()) - 1
    # the distinct aids of every session: the rows of a count that drops nothing
    u_off, u_col, _, _ = similarity.count(aid, sess_off, n_aids, min_aid=0)
    n_unique = u_off[1:] - u_off[:-1]
    recency = n_unique >= min_unique
    length = sess_off[1:] - sess_off[:-1]
    slot = torch.arange(n_pred, device=dev, dtype=torch.int64)[None, :]
    pred = torch.full((S, n_pred), -1, dtype=torch.int32, device=dev)
    if aid.numel() == 0:
        return pred, torch.zeros(S, dtype=torch.int32, device=dev), recency
    # recency branch: the head of every session's most_common list
    r_cand, _, r_n = recency_candidates(aid, typ, sess_off, curves=(RECENCY_CURVE,), type_coef=TYPE_COEFFICIENT)
    r_n = torch.clamp(r_n.to(torch.int64), max=n_pred)
    take = recency[:, None] & (slot < r_n[:, None])
    src = (sess_off[:-1, None] + slot).clamp(max=aid.numel() - 1)
    pred = torch.where(take, r_cand[0][src], pred)
    # similarity branch: distinct aids, then the neighbours of the last aid
    m = similarity.fit_transform(aid, sess_off, n_aids, min_aid)
    last = aid[(sess_off[1:] - 1).clamp(min=0)]
    wanted = ~recency & (length > 0)
    queries, inverse = torch.unique(last[wanted], return_inverse=True)
    nb_of = torch.zeros(S, dtype=torch.int64, device=dev)
    nb_of[wanted] = inverse
    if queries.numel():
        nb, _, nb_n = similarity.similar_aids(m, queries.to(torch.int32).contiguous(), k=n_similar)
    else:
        nb = torch.full((1, n_similar), -1, dtype=torch.int32, device=dev)
        nb_n = torch.zeros(1, dtype=torch.int32, device=dev)
    own = ~recency[:, None] & (slot < n_unique[:, None])
    src = (u_off[:-1, None] + slot).clamp(max=u_col.numel() - 1)             # a count that drops nothing: one entry at least
    pred = torch.where(own, u_col[src], pred)
    t = slot - n_unique[:, None]                               # position inside the neighbour list
    follow = wanted[:, None] & (t >= 0) & (t < nb_n.to(torch.int64)[nb_of][:, None])
    pred = torch.where(follow, nb[nb_of[:, None], t.clamp(min=0, max=n_similar - 1)], pred)
    n = torch.where(recency, r_n, torch.clamp(n_unique + torch.where(wanted, nb_n.to(torch.int64)[nb_of], 0), max=n_pred))
    return pred.contiguous(), n.to(torch.int32), recency


def _main(argv=None):
    import argparse
    import torch
    from .. import events as ev_mod
    from ..ranker import evaluate
    parser = argparse.ArgumentParser(prog='python -m otto_amd.tfidf.inference')
    parser.add_argument('mode', choices=('validation', 'submission'))
    parser.add_argument('--events', nargs='+', required=True, help='parquet split files or .jsonl files of the sessions to predict')
    parser.add_argument('--out', help='submission mode: the csv.gz to write')
    parser.add_argument('--seed', type=int, default=42, help='validation mode: the seed of the cutoffs')
    parser.add_argument('--device', default='cuda:0')
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    dev = _lib.rocm_device(args.device, 'tfidf.inference')
    read = ev_mod.jsonl_to_events_device if args.events[0].endswith('.jsonl') else ev_mod.parquet_to_events_device
    events = read(args.events, device=dev)
    if args.mode == 'validation':
        logging.info('Running TF-IDF similarity model in validation mode')
        cutoff, _ = evaluate.cutoffs(events, args.seed)
        events, labels = evaluate.split(events, cutoff)
    elif not args.out:
        parser.error('submission mode needs --out')
    pred, n, recency = predictions(events.aid, events.type, events.sess_off, events.n_aids)
    logging.info(f'{int(recency.sum())} sessions are predicted with recency weight, {int((~recency).sum())} with tfidf')
    if args.mode == 'validation':
        scores = evaluate.evaluate({name: (pred, n) for name in evaluate.TYPES}, labels)
        logging.info('TF-IDF similarity model validation scores\n' +
                     '\n'.join(f'{name} recall@20: {scores[name]:.4f}' for name in evaluate.TYPES) +
                     f'\nweighted recall@20: {scores["weighted"]:.4f}')
        return scores
    from .. import submission
    session_id = events.session_ids.to(torch.int32).contiguous()
    stats = submission.write_csv(args.out, [submission.format_rows(session_id, [(pred, n)] * 3, [0, 1, 2], interleave=True, header=True)])
    logging.info(f"{args.out}: {stats['bytes']} bytes of text, {stats['file_bytes']} bytes written")
    return stats


if __name__ == '__main__':
    _main()
