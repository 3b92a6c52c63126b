"""Planes below one tile: the CPU oracle against the float64 model (np_restatement.DetectorModel) on every case of
detector_cases.small_cases() -- one-octave planes from 4 x 1 up, the smallest pyramids with a second and a third octave,
the input stages, batches of eight and keypoint lists on them.  At these sizes every index is a clamped or a wrapped one
(replicated filter borders, the 1-D wrap of the det-H neighbours, "past the plane reads 0"), and a keypoint's window may
hold no sample at all; tests/test_small_images_gpu.py runs the same checker on the HIP path.

The two wrong-rule switches these cases are there for are shown to be caught in tests/test_detector_model.py (CATCHES).
"""
from contextlib import closing

import pytest

import detector_cases as dc
from oracle_lib import OracleSession

CASES = list(dc.small_cases())


@pytest.mark.parametrize("name", CASES)
def test_oracle_follows_the_model(name):
    case = dc.small_cases()[name]
    with closing(OracleSession(threads=4, **case.kw)) as o:
        st = dc.check_against_model(o, case)
    print(name, st)
    dc.check_small_statistics(st, case)


def test_the_set_is_not_planes_only():
    """At least ten cases have 8 or more detections, and the feature counts stated per case are the oracle's."""
    busy = 0
    for name, case in dc.small_cases().items():
        if case.keys is not None:
            continue
        stack, at = dc.case_input(case)
        with closing(OracleSession(threads=4, keep_levels=False, **case.kw)) as o:
            n = o.run(stack, fmt=case.fmt)[at]
            busy += len(o.rawlist(at)) >= 8
        assert n == case.min_features, name
    assert busy >= 10, busy


def test_the_key_lists_meet_empty_windows():
    """Every key on a plane of one or two rows, and the keys of _user_keys beyond the border at first_octave -1: the
    cases the empty-window rule is stated for exist."""
    from hessgpu_amd import _abi   # noqa: F401  (the cases' key dtype)

    for name, want in (("keypoint list 4x1 defaults orient=1", 40), ("keypoint list 7x2 half_sift orient=0", 40),
                       ("keypoint list 64x1 normalize 0 orient=1", 40), ("keypoint list 12x3 first_octave -1 orient=1", 9),
                       ("keypoint list 17x23 first_octave -1 orient=0", 1), ("keypoint list 36x5 defaults orient=1", 0)):
        case = dc.small_cases()[name]
        with closing(OracleSession(threads=4, **case.kw)) as o:
            st = dc.check_against_model(o, case)
        assert st["empty_windows"] == want, (name, st)


def test_the_constant_stack_has_empty_images_between_others():
    stack = dc.constant_stack(65, 33)
    with closing(OracleSession(threads=4, keep_levels=False, **dc.NOISE_KW)) as o:
        n = o.run(stack)
    assert [n[j] for j in (0, 3, 4, 7)] == [0, 0, 0, 0] and min(n[j] for j in (1, 2, 5, 6)) > 0, n
