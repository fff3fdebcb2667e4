"""Label assembly on the host (SPEC-LABELS, include/otto_labels.h): the NumPy restatement (tests/pqlist_restatement.py)
against the reference's ``map`` + three left merges + ``fillna`` in pandas on every input of the GPU tests, the conditions
those inputs must meet, and the restatement's refusals."""
import numpy as np
import pytest

import pqlist_inputs as I
import pqlist_restatement as R

SIZES = (0, 1, 64, 65, 3000)


def csr(lists):
    lens = np.array([len(l) for l in lists], dtype=np.int64)
    return np.r_[0, np.cumsum(lens)].astype(np.int64), np.array([v for l in lists for v in l], dtype=np.int64), np.zeros(len(lists), dtype=np.uint8)


def same(got, want):
    for (go, ga), (wo, wa) in zip(got, want):
        assert np.array_equal(go, wo) and np.array_equal(ga, wa) and ga.dtype == np.int32


@pytest.mark.parametrize('S', SIZES)
def test_restatement_equals_the_pandas_chain(S):
    ids, sess, typ, lists = I.label_rows(S, seed=S)
    off, value, null = csr(lists)
    got, dropped = R.labels_assemble(sess, typ, off, value, null, ids, 5000)
    assert dropped == 0
    same(got, R.labels_reference(I.label_frame(sess, typ, lists), ids))
    keep = ids[::2]                                                              # half the sessions are not in the list
    got, dropped = R.labels_assemble(sess, typ, off, value, null, keep, 5000)
    assert dropped == int((~np.isin(sess, keep)).sum())
    same(got, R.labels_reference(I.label_frame(sess, typ, lists), keep))


def test_the_inputs_hold_what_they_are_there_for():
    ids, sess, typ, lists = I.label_rows(3000, seed=3000)
    per = {int(s): set() for s in ids}
    for s, t in zip(sess, typ):
        per[int(s)].add(int(t))
    assert any(len(v) == 0 for v in per.values()) and any(len(v) == 3 for v in per.values()) and any(len(v) == 1 for v in per.values())
    assert not np.array_equal(sess, np.sort(sess))                               # shuffled file order
    assert max(len(l) for l, t in zip(lists, typ) if t == 1) == 300
    assert any(len(set(l)) < len(l) for l in lists)                              # a repeated aid, which is kept


def test_null_and_empty_lists_are_empty_lists():
    sess = np.array([5, 5, 7, 9], dtype=np.int64)
    typ = np.array([0, 1, 1, 2], dtype=np.uint8)
    off = np.array([0, 1, 1, 1, 3], dtype=np.int64)
    value = np.array([4, 8, 8], dtype=np.int64)
    null = np.array([0, 1, 0, 0], dtype=np.uint8)
    got, dropped = R.labels_assemble(sess, typ, off, value, null, [5, 6, 7], 10)
    assert dropped == 1
    assert got[0][0].tolist() == [0, 1, 1, 1] and got[0][1].tolist() == [4]
    assert got[1][0].tolist() == [0, 0, 0, 0] and got[2][0].tolist() == [0, 0, 0, 0]
    got, _ = R.labels_assemble(sess, typ, off, value, null, [9], 10)
    assert got[2][1].tolist() == [8, 8]


def test_restatement_refusals():
    ids, sess, typ, lists = I.label_rows(65, seed=1)
    off, value, null = csr(lists)
    for name, edit, row, code in refusal_edits(sess, typ, off, value):
        s, t, v = sess.copy(), typ.copy(), value.copy()
        edit(s, t, v)
        with pytest.raises(R.LabelRefused) as e:
            R.labels_assemble(s, t, off, v, null, ids, 5000)
        assert (e.value.row, e.value.code) == (row, code), name


def refusal_edits(sess, typ, off, value):
    """(name, edit(session, type, value), smallest offending row, reason) over rows of :func:`pqlist_inputs.label_rows`"""
    first = {}
    dup = next(r for r in range(len(sess)) if first.setdefault((int(sess[r]), int(typ[r])), r) != r or
               any(sess[q] == sess[r] and typ[q] != typ[r] for q in range(r)))
    mate = next(q for q in range(dup) if sess[q] == sess[dup])
    full = [r for r in range(len(sess)) if off[r + 1] > off[r]]

    def e_type(s, t, v): t[40] = 3; t[90] = 200
    def e_dup(s, t, v): t[dup] = t[mate]
    def e_high(s, t, v): v[off[full[30]]] = 5000
    def e_neg(s, t, v): v[off[full[50] + 1] - 1] = -1; v[off[full[70]]] = 2 ** 40
    def e_sess(s, t, v): s[33] = 2 ** 31; s[34] = -2 ** 31 - 1
    def e_both(s, t, v): t[60] = 9; s[60] = 2 ** 40; v[off[full[10]]] = -4
    return [('type', e_type, 40, R.TYPE), ('duplicate', e_dup, dup, R.DUP), ('value high', e_high, full[30], R.VALUE),
            ('value negative', e_neg, full[50], R.VALUE), ('session', e_sess, 33, R.SESSION),
            ('several', e_both, full[10] if full[10] < 60 else 60, R.VALUE if full[10] < 60 else R.SESSION)]
