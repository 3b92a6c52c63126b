"""tests/refit_cases.py on the CPU: the float64 model of the refit (include/hess_abi.h, step 6) and the conditions under which
the chosen inputs let tests/test_matcher_refit_gpu.py decide: every step well conditioned, no step undecided, the quality
cases at least halve the error, the rejected case ends in a decided reject."""
import numpy as np
import pytest

import geom_cases as g
import refit_cases as rc


@pytest.mark.parametrize("key", list(rc.NOISY))
def test_noisy_chain_is_decided_and_conditioned(key):
    c = rc.noisy(*key, rc.NOISY[key])
    ch = rc.chain64(c, 4)
    assert ch.steps and rc.chain_is_sound(ch), [(st.stop, getattr(st, "kappa", None), getattr(st, "verdict", None)) for st in ch.steps]
    assert all(st.stop is None and st.verdict == "accept" for st in ch.steps)
    assert int(ch.S.sum()) >= int(ch.S0.sum()) >= g.K[c.model]
    if key in rc.QUALITY:
        before, after = rc.rms(c, ch.M0), rc.rms(c, ch.M)
        print(f"{c.name}: rms {before:.3f} -> {after:.3f}, inliers {int(ch.S0.sum())} -> {int(ch.S.sum())} of {int(c.planted.sum())}, "
              f"{ch.refits} refits")
        assert 2 * after <= before


def test_rejected_chain_ends_in_a_decided_reject():
    c = rc.noisy(*rc.REJECTED)
    ch = rc.chain64(c, 4)
    assert rc.chain_is_sound(ch)
    assert ch.refits >= 1 and ch.steps[-1].stop is None and ch.steps[-1].verdict == "reject"
    assert ch.steps[-1].hi < ch.steps[-1].before == int(ch.S.sum())


@pytest.mark.parametrize("model", ("H", "F"))
def test_candidate_is_the_eigenvector_of_the_normal_matrix(model):
    """solve64 on the inliers (an SVD of the design matrix) and the eigenvector of N = A^T A brought back to pixel coordinates
    are the same matrix; the moment sums rebuild N."""
    c = rc.noisy(model, 300, 1.0, 1)
    M, S, _ = rc.ransac64(c)
    nm = rc.normal64(model, c.p1[S], c.p2[S])
    C = rc.candidate64(model, c.p1, c.p2, S, M)
    assert g.distance(rc.denormalise64(model, nm.x, nm), C) <= 1e-9 * max(nm.kappa, 1.0)
    assert (C * M).sum() >= 0 and abs(np.linalg.norm(C) - 1) <= 1e-12
    s = rc.moments(model, nm.a, nm.b)
    N = np.zeros((9, 9))
    for i in range(3):
        for k in range(3):
            for j in range(3):
                for l in range(3):
                    if model == "F":
                        v = s[6 * rc._sym(i, j) + rc._sym(k, l)]
                    else:
                        blk = (min(i, j), max(i, j))
                        v = {(0, 0): s[rc._sym(k, l)], (1, 1): s[rc._sym(k, l)], (0, 2): -s[6 + rc._sym(k, l)],
                             (1, 2): -s[12 + rc._sym(k, l)], (2, 2): s[18 + rc._sym(k, l)]}.get(blk, 0.0)
                    N[3 * i + k, 3 * j + l] = v
    assert np.abs(N - nm.N).max() <= 1e-12 * np.abs(nm.N).max()


def test_exact_cases_are_a_fixed_point_of_the_model():
    for name in ("H 300", "F 300", "clean"):
        c = g.case(name)
        ch = rc.chain64(c, 8)
        assert ch.refits == 1 and np.array_equal(ch.S, ch.S0) and np.array_equal(ch.S0, c.planted), name
        assert ch.steps[0].kappa <= rc.MAX_KAPPA


def test_stops_of_the_model():
    c = g.case("H 300")
    few = np.zeros(c.n, bool)
    few[:3] = True
    assert rc.step64("H", c.p1, c.p2, few, np.eye(3), c.bound).stop == "few"
    same = np.repeat(c.p1[:1], 8, 0)
    assert rc.step64("H", same, same, np.ones(8, bool), np.eye(3), c.bound).stop == "degenerate"
