"""The most-frequent-aid lists on the device (``otto_freq_*`` of ``include/otto_submit.h``): per
(type, aid) event counts and their top k, all types together and per type.

Reference code replaced: ``src/baseline/frequency_statistics.py`` (``groupby`` -> ``count`` -> ``sort_values`` ->
``head(20)`` -> ``to_dict`` -> ``json.dump``). The lists go into ``candidates.predictions(most_frequent=...)`` as they are.
Ties of the count are ordered by ascending aid; the reference's ``sort_values`` leaves them unpinned.
"""
import json
import os

ROWS = ('all', 'click', 'cart', 'order')
MAX_K = 64                                     # OTTO_SUBMIT_MAX_K
# The reference's script writes settings.DATA / 'statistics', its consumers (src/covisitation/inference.py:44,76-83) read
# settings.DATA / 'aid_frequencies' (SURVEY.md section 9). The default is the one that is read.
DEFAULT_DIRECTORY = 'aid_frequencies'


def count_events(aid, typ, n_aids, counts=None):
    """``counts`` int32 [3, n_aids] (the bit patterns of uint32; a new zeroed tensor when None) += the events ``aid`` int32
    / ``typ`` uint8 on the device. Raises ``OttoError`` for an aid outside [0, n_aids) or a type above 2."""
    import torch
    from . import _lib
    aid = _lib.need(aid, 'aid', torch.int32, 1)
    dev = aid.device
    typ = _lib.need(typ, 'type', torch.uint8, 1, device=dev, numel=aid.numel())
    n_aids = int(n_aids)
    if counts is None:
        counts = torch.zeros((3, n_aids), dtype=torch.int32, device=dev)
    else:
        _lib.need(counts, 'counts', torch.int32, 2, device=dev, numel=3 * n_aids)
    _lib.call('otto_freq_count', dev, aid, typ, int(aid.numel()), n_aids, counts)
    return counts


def top_lists(counts, k=20):
    """``counts`` int32 [3, n_aids] -> ``{'all' | 'click' | 'cart' | 'order': (aids int32 [n], counts int64 [n])}`` as NumPy
    arrays, n <= k: by (count descending, aid ascending), aids that never occur left out."""
    import torch
    from . import _lib
    _lib.need(counts, 'counts', torch.int32, 2)
    if counts.shape[0] != 3:
        raise ValueError('counts: expected [3, n_aids]')
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k must be in [1, {MAX_K}] (got {k})')
    dev = counts.device
    top_aid = torch.empty((4, k), dtype=torch.int32, device=dev)
    top_count = torch.empty((4, k), dtype=torch.int64, device=dev)
    n = torch.empty(4, dtype=torch.int32, device=dev)
    _lib.call('otto_freq_topk', dev, counts, int(counts.shape[1]), k, top_aid, top_count, n)
    top_aid, top_count, n = top_aid.cpu().numpy(), top_count.cpu().numpy(), n.cpu().numpy()
    return {name: (top_aid[r, :n[r]].copy(), top_count[r, :n[r]].copy()) for r, name in enumerate(ROWS)}


def most_frequent(aid, typ, n_aids, k=20, counts=None):
    """Count the events into ``counts`` (``None``: from zero; the tensor a call on the training events returned: the
    reference's "all" split) and list the ``k`` most frequent aids: ``(counts, lists)`` of :func:`count_events` and
    :func:`top_lists`. ``lists['click'][0]`` is what ``candidates.predictions`` takes as ``most_frequent``."""
    counts = count_events(aid, typ, n_aids, counts)
    return counts, top_lists(counts, k)


def json_bytes(aids, counts):
    """The bytes of ``json.dump({aid: count}, f, indent=2)`` for one list (integer keys are written as strings)."""
    return json.dumps({str(int(a)): int(c) for a, c in zip(aids, counts)}, indent=2).encode()


def write_json(directory, split, lists, k=20):
    """``{split}_{k}_most_frequent_aids.json`` and ``{split}_{k}_most_frequent_{click,cart,order}_aids.json`` under
    ``directory`` (created when missing), byte for byte what the reference's script writes. ``directory=None``:
    ``settings.DATA / 'aid_frequencies'``, where the covisitation inference reads them. Returns the paths."""
    if directory is None:
        from . import settings
        directory = settings.DATA / DEFAULT_DIRECTORY
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name in ROWS:
        file = f'{split}_{k}_most_frequent_aids.json' if name == 'all' else f'{split}_{k}_most_frequent_{name}_aids.json'
        paths.append(os.path.join(directory, file))
        with open(paths[-1], 'wb') as f:
            f.write(json_bytes(*lists[name]))
    return paths
