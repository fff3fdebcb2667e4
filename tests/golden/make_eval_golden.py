"""Writes eval_golden.npz: the labels the reference's own ``validation.get_labels`` gives at EVERY index of a few hundred
seeded sessions, so that tests can compare against them where the reference is not installed.

    python tests/golden/make_eval_golden.py /path/to/reference/src

The reference module imports ``settings`` at the top; a stub in ``sys.modules`` is enough. Only data is stored:
aid int32, typ uint8, sess_off int64 (the inputs); per event position e (session s, index i, e = sess_off[s] + i) the
labels ``get_labels(...)[i]``: click int64 [E] (-1 for None / []), cart_off / order_off int64 [E+1] with cart_aid /
order_aid int32 sorted ascending (None / NaN / [] stored as empty).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def sessions():
    rng = np.random.default_rng(20230131)
    out = []
    for s in range(300):
        n = int(rng.integers(1, 12)) if s % 10 else int(rng.integers(12, 80))
        n_aids = int(rng.choice((3, 10, 1000)))
        out.append((rng.integers(0, n_aids, n).astype(np.int32), rng.choice(3, n, p=(0.6, 0.25, 0.15)).astype(np.uint8)))
    return out


def as_list(v):
    if v is None or (isinstance(v, float) and np.isnan(v)):
        return []
    return sorted(int(x) for x in v) if isinstance(v, (list, tuple, set)) else [int(v)]


def main(reference_src):
    sys.modules.setdefault('settings', types.ModuleType('settings'))
    sys.path.insert(0, reference_src)
    import validation
    data = sessions()
    click, carts, orders = [], [], []
    for aids, typs in data:
        for lab in validation.get_labels(aids=aids.tolist(), event_types=typs.tolist()):
            c = as_list(lab[0])
            click.append(c[0] if c else -1)
            carts.append(as_list(lab[1]))
            orders.append(as_list(lab[2]))
    csr = lambda ls: (np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64),
                      np.asarray([v for x in ls for v in x], dtype=np.int32))
    cart_off, cart_aid = csr(carts)
    order_off, order_aid = csr(orders)
    np.savez_compressed(os.path.join(HERE, 'eval_golden.npz'),
                        aid=np.concatenate([a for a, _ in data]), typ=np.concatenate([t for _, t in data]),
                        sess_off=np.concatenate([[0], np.cumsum([len(a) for a, _ in data])]).astype(np.int64),
                        click=np.asarray(click, dtype=np.int64), cart_off=cart_off, cart_aid=cart_aid, order_off=order_off,
                        order_aid=order_aid)


if __name__ == '__main__':
    main(sys.argv[1])
