"""Conditions on the inputs of the calling-contract cases (tests/contract_cases.py), checked with the restatements alone:
a stale read can only be seen if the decoy's answer differs from the real one in every output, the decoy must be an input
of identical shapes, and the cases together must reach every entry point that takes a stream."""
import numpy as np
import pytest

import contract_cases as cc


@pytest.fixture(scope='module')
def inputs():
    made = {}

    def get(case, seed, scale=1):
        key = (case.name, seed, scale)
        if key not in made:
            made[key] = case.make(seed, scale)
        return made[key]
    return get


@pytest.mark.parametrize('case', cc.CASES, ids=lambda c: c.name)
def test_real_and_decoy_have_equal_shapes_and_dtypes(case, inputs):
    real, decoy = inputs(case, cc.REAL_SEED), inputs(case, cc.DECOY_SEED)
    assert list(real) == list(decoy)
    for k in real:
        a, b = real[k], decoy[k]
        if isinstance(a, np.ndarray):
            assert isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype, (case.name, k)
        elif isinstance(a, (bytes, bytearray)):
            assert len(a) == len(b), (case.name, k)
        else:
            assert a == b, (case.name, k, 'a scalar is part of the shape')
    again = case.make(cc.REAL_SEED)
    for k in real:
        assert cc.same_bytes(real[k], again[k]), (case.name, k, 'make is not a function of the seed')


@pytest.mark.parametrize('case', cc.CASES, ids=lambda c: c.name)
def test_double_size_decoy_is_larger_in_some_input(case, inputs):
    decoy, decoy2 = inputs(case, cc.DECOY_SEED), inputs(case, cc.DECOY_SEED, 2)
    assert list(decoy) == list(decoy2)
    size = lambda v: v.size if isinstance(v, np.ndarray) else len(v) if isinstance(v, (bytes, bytearray)) else 0
    assert any(size(decoy2[k]) >= 1.9 * size(decoy[k]) > 0 for k in decoy), case.name


@pytest.mark.parametrize('case', cc.CASES, ids=lambda c: c.name)
def test_restated_outputs_of_real_and_decoy_differ_in_every_tensor(case, inputs):
    real, decoy = case.restate(inputs(case, cc.REAL_SEED)), case.restate(inputs(case, cc.DECOY_SEED))
    assert len(real) == len(decoy) > 0
    for i, (a, b) in enumerate(zip(real, decoy)):
        if i in case.shape_outputs:
            continue
        assert not cc.same_bytes(a, b), f'{case.name}: output {i} is the same for the decoy; a stale read could not be seen'
    if not case.custom_check:
        case.check(inputs(case, cc.REAL_SEED), real)          # check() accepts the restatement's own outputs ...
        with pytest.raises(AssertionError):
            case.check(inputs(case, cc.REAL_SEED), decoy)      # ... and not the decoy's


@pytest.mark.parametrize('case', [c for c in cc.CASES if c.refusals], ids=lambda c: c.name)
def test_refusal_edits_keep_the_shapes(case, inputs):
    real = inputs(case, cc.REAL_SEED)
    for name, (edit, call, match) in case.refusals.items():
        if edit is None:
            continue                                          # the call writes its own bad file
        bad = edit(real)
        assert list(bad) == list(real), (case.name, name)
        changed = [k for k in real if not cc.same_bytes(bad[k], real[k])]
        assert changed, (case.name, name, 'the edit changes nothing')
        for k in real:
            assert np.shape(bad[k]) == np.shape(real[k]) and np.asarray(bad[k]).dtype == np.asarray(real[k]).dtype, (case.name, name, k)


def test_case_names_are_unique():
    assert len({c.name for c in cc.CASES}) == len(cc.CASES)


def test_every_streamed_entry_point_has_a_case_or_a_reasoned_exemption():
    streamed = cc.streamed_entry_points()
    covered = set()
    for c in cc.CASES:
        covered |= set(c.entry_points)
    assert covered <= streamed, f'cases name entry points that take no stream: {sorted(covered - streamed)}'
    assert set(cc.EXEMPT) <= streamed, sorted(set(cc.EXEMPT) - streamed)
    assert not covered & set(cc.EXEMPT), sorted(covered & set(cc.EXEMPT))
    for name, reason in cc.EXEMPT.items():
        assert reason.startswith(('needs several ranks', 'diagnostic only')) and '\n' not in reason, name
    missing = streamed - covered - set(cc.EXEMPT)
    assert not missing, f'{len(missing)} entry points that take a stream have neither a case nor an exemption: {sorted(missing)}'
