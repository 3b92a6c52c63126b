"""The inputs of the geometry-estimation tests (tests/geom_cases.py) on the CPU: the library's sampling rule is the stated
one, and every planted case can be solved -- enough all-inlier hypotheses, each of which classifies every correspondence as
planted when solved in float64, and no contaminated hypothesis that does as well."""
import numpy as np
import pytest

import geom_cases as g


def test_library_sampling_rule_equals_the_python_rule():
    from hessgpu_amd.matcher import geom_sample

    for seed in (0, 1, 11, 0x9E3779B9, 0xFFFFFFFF):
        for k in (1, 4, 8):
            for n in (k, k + 1, 9, 65, 4096, 1 << 20):
                if n < k:
                    continue
                for t in (0, 1, 255, 256, 65535):
                    got = geom_sample(seed, t, k, n).tolist()
                    assert got == g.sample(seed, t, k, n), (seed, t, k, n)
                    assert len(set(got)) == k and min(got) >= 0 and max(got) < n, (seed, t, k, n)


def test_library_sampling_refuses_what_it_cannot_draw():
    from hessgpu_amd import HessError
    from hessgpu_amd.matcher import geom_sample

    for t, k, n in ((0, 4, 3), (0, 0, 5), (0, 9, 20), (-1, 4, 10)):
        with pytest.raises(HessError):
            geom_sample(1, t, k, n)


def test_python_rule_draws_distinct_indices_in_range():
    for seed in range(3):
        for k in (4, 8):
            for n in (k, k + 1, 17, 300):
                for t in range(64):
                    s = g.sample(seed, t, k, n)
                    assert len(set(s)) == k and 0 <= min(s) and max(s) < n


def test_gate_many_is_the_gate_of_guided_cases():
    for name in ("H 300", "F 300"):
        c = g.case(name)
        for M in (c.truth, g.solve64(c.model, c.p1[:8], c.p2[:8])):
            a, b = g.gate64(c.model, M, c.p1, c.p2), g.gate_many(c.model, M, c.p1, c.p2)
            assert np.allclose(a, b, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", g.PLANTED)
def test_planted_case_can_be_found(name):
    c = g.case(name)
    k, want = g.K[c.model], int(c.planted.sum())
    assert len(c.allin) >= min(g.MIN_ALL_INLIER, c.T), (name, c.seed, len(c.allin))
    assert np.array_equal(c.p1, c.loc1[c.matches[:, 0]]) and np.array_equal(c.p2, c.loc2[c.matches[:, 1]])
    if c.n > k:
        v = g.gate64(c.model, c.truth, c.p1, c.p2)
        assert v[c.planted].max() < c.bound / 100 and v[~c.planted].min() >= 4 * c.bound
    best_contaminated = 0
    for t in range(c.T):
        s = g.sample(c.seed, t, k, c.n)
        passed = g.gate_many(c.model, g.solve64(c.model, c.p1[s], c.p2[s]), c.p1, c.p2) < c.bound
        if t in c.allin:
            assert np.array_equal(passed, c.planted), (name, t, int(passed.sum()), want)
        else:
            best_contaminated = max(best_contaminated, int(passed.sum()))
    print(f"{name}: seed {c.seed}, planted {want} of {c.n}, {len(c.allin)} all-inlier hypotheses of {c.T}, "
          f"best contaminated count {best_contaminated}")
    assert best_contaminated < want or c.n == k


def test_below_k_and_clean_cases():
    for name in g.BELOW:
        c = g.case(name)
        assert c.n == g.K[c.model] - 1 and len(c.matches) == c.n and not c.allin
    c = g.case("clean")
    assert c.planted.all() and c.n == 64
    M = g.solve64("H", c.p1[g.sample(c.seed, 0, 4, c.n)], c.p2[g.sample(c.seed, 0, 4, c.n)])
    assert g.gate64("H", M, c.p1, c.p2).max() < 1e-6
