"""The banks of tests/guided_pair_cases.py on the CPU oracle alone: the properties the GPU tests of
hess_matcher_match_pairs_guided (tests/test_match_pairs_guided_gpu.py) rely on.  Integer results: every comparison is exact."""
import numpy as np
import pytest

import guided_cases as gc
import guided_pair_cases as gp
from oracle_lib import oracle_match


def _oracle(c, h, f, dm, rm, mutual, d1=None, loc1=None):
    d1 = c.d1 if d1 is None else d1
    loc1 = c.loc1 if loc1 is None else loc1
    return oracle_match(d1, c.d2, loc1, c.loc2, c.H, c.F, hdistmax=h, fdistmax=f, distmax=dm, ratiomax=rm, mutual_best=mutual,
                        max_match=len(d1))


def _has(matches, i, j=None):
    return any(int(a) == i and (j is None or int(b) == j) for a, b in matches)


def test_the_case_bank_pairs_are_the_cases():
    sets, locs, pairs, cases = gp.case_bank()
    assert len(sets) == len(locs) == 2 * len(cases) and pairs.tolist() == [[2 * k, 2 * k + 1] for k in range(len(cases))]
    for k, cs in enumerate(cases):
        assert sets[2 * k].shape == (cs[0], 128) and sets[2 * k + 1].shape == (cs[1], 128)
        assert locs[2 * k].shape == (cs[0], 2) and locs[2 * k + 1].shape == (cs[1], 2)
    H, F, hd, fd = gp.geometry(cases, [k % 4 for k in range(len(cases))])
    assert H.shape == F.shape == (len(cases), 3, 3) and hd.dtype == fd.dtype == np.float32
    assert len({H[k].tobytes() for k in range(len(cases))}) == 3      # the three geometries


@pytest.mark.parametrize("n1,n2,geometry", gp.SEAM_CASES)
def test_row_shifted_pair_moves_every_match_and_keeps_the_leaks(n1, n2, geometry):
    c, s = gc.case(n1, n2, geometry), gp.shifted(n1, n2, geometry)
    assert s.d1.shape == (n1 + gp.SHIFT, 128) and not s.d1[:gp.SHIFT].any() and np.array_equal(s.d1[gp.SHIFT:], c.d1)
    rows = {name: (i, ip, ipp) for name, i, ip, ipp, _ in s.triples}
    assert rows["A"] == (251, 252, 260) and rows["B"] == (283, 284, 292) and rows["C"][0] // 8 == (n1 + gp.SHIFT - 1) // 8
    for k, (h, f) in enumerate(gc.pick_thresholds(n1, n2, geometry)):
        for dm, rm, mutual in gc.CONFIGS:
            ref, got = _oracle(c, h, f, dm, rm, mutual), _oracle(s, h, f, dm, rm, mutual)
            assert len(ref) and np.array_equal(got, gp.shift_matches(ref)), (k, dm, rm, mutual)
            if k == 0 and (dm, rm) == (2.0, 2.0):
                for name, i, ip, ipp, j in s.triples:
                    assert _has(got, ip, j) and not _has(got, ipp), (name, mutual)


@pytest.mark.parametrize("n1,n2,geometry", gp.SEAM_CASES)
def test_trailing_row_trap(n1, n2, geometry):
    t = gp.trap(n1, n2, geometry)
    assert np.array_equal(t.follower[1][:4], np.repeat(gc.case(n1, n2, geometry).loc1[296:297], 4, 0))
    for k in (0, 2):                                  # both gates, and the H gate alone
        h, f = gc.pick_thresholds(n1, n2, geometry)[k]
        for mutual in (True, False):
            ref = _oracle(t, h, f, 2.0, 2.0, mutual)
            assert len(ref) and not _has(ref, t.ipp, t.j), (k, mutual)
            wrong = _oracle(t, h, f, 2.0, 2.0, mutual, *t.appended)
            assert _has(wrong, t.ipp, t.j), (k, mutual)      # what reading on into the next set's locations gives


def test_zero_matrices_match_nothing_even_with_the_bounds_off():
    c = gc.case(65, 63, "affine")
    zero = np.zeros((3, 3), np.float32)
    kw = dict(hdistmax=gc.OFF, fdistmax=gc.OFF, distmax=2.0, ratiomax=2.0, mutual_best=False, max_match=c.n1)
    assert len(oracle_match(c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, **kw))
    assert len(oracle_match(c.d1, c.d2, c.loc1, c.loc2, zero, c.F, **kw)) == 0
    assert len(oracle_match(c.d1, c.d2, c.loc1, c.loc2, c.H, zero, **kw)) == 0
