"""The inputs of the geometry-estimation tests (tests/geom_cases.py) on the CPU: the library's sampling rule is the stated
one, and every planted case can be solved -- enough all-inlier hypotheses, each of which classifies every correspondence as
planted when solved in float64, and no contaminated hypothesis that does as well.  For tests/test_matcher_estimate_model_gpu.py:
one hypothesis alone (unmix, alone), the batched float64 solve, the validity of every separated case and the table of wrong
winner rules each of them tells from the rule, the condition on the noisy scene, the degenerate inputs."""
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


def test_unmix_inverts_mix():
    words = [0, 1, 0x9E3779B9, 0x80000000, g.M32] + np.random.default_rng(0).integers(0, 1 << 32, 5000).tolist()
    for v in words:
        assert g.mix(g.unmix(v)) == v and g.unmix(g.mix(v)) == v, hex(v)


def test_alone_is_the_hypothesis_on_its_own_by_the_library_sampling():
    from hessgpu_amd.matcher import geom_sample

    for seed in (0, 1, 11, 0x9E3779B9, 0xFFFFFFFF):
        for t in (0, 255, 256, 65535):
            assert 0 <= g.alone(seed, t) <= g.M32
            for k, n in ((4, 4), (4, 64), (8, 300), (8, 1 << 20)):
                want = geom_sample(seed, t, k, n).tolist()
                assert geom_sample(g.alone(seed, t), 0, k, n).tolist() == want == g.sample(seed, t, k, n), (seed, t, k, n)


def test_samples_is_the_python_rule_on_arrays():
    for seed in (0, 1, 0xFFFFFFFF):
        for k, n in ((4, 4), (4, 64), (8, 16), (8, 300), (8, 1 << 20)):
            assert g.samples(seed, 600, k, n).tolist() == [g.sample(seed, t, k, n) for t in range(600)], (seed, k, n)


def test_batched_solve_equals_the_solve_of_one_sample():
    """H against solve64 itself.  F: solve64 makes the normalised matrix rank 2, the rule (step 5) the matrix in pixel
    coordinates, which is another matrix when the sample holds outliers; the batched solve follows the rule, so it is held
    against solve(rank2=False) finished by finish64, and against solve64 on all-inlier samples, where both agree."""
    for name in ("H 300", "F 300", "H 65"):
        c = g.case(name)
        k = g.K[c.model]
        idx = g.samples(c.seed, 256, k, c.n)
        h = g.solve_many(c.model, c.p1[idx], c.p2[idx])
        assert not h.bad.any()
        looked = 0
        for t in list(range(0, 256, 5)) + [t for t in c.allin if t < 256]:
            if h.kappa[t] > 1e6:
                continue
            A = g.solve(c.model, c.p1[idx[t]], c.p2[idx[t]], rank2=False)
            for got, ref in ((h.M0[t], A), (h.M[t], g.finish64(c.model, A))):
                assert min(np.linalg.norm(got - ref), np.linalg.norm(got + ref)) <= 1e-11 * h.kappa[t], (name, t, h.kappa[t])
            if c.model == "H" or t in c.allin:
                ref = g.solve64(c.model, c.p1[idx[t]], c.p2[idx[t]])
                tol = 1e-11 if c.model == "H" else 1e-6
                assert min(np.linalg.norm(h.M[t] - ref), np.linalg.norm(h.M[t] + ref)) <= tol * h.kappa[t], (name, t)
            looked += 1
        assert looked >= 40
    # a sample of coincident points is a non-finite system
    p = np.ones((1, 4, 2))
    assert g.solve_many("H", p, p).bad.all()


@pytest.mark.parametrize("name", g.SOLO)
def test_single_hypotheses_to_compare_with_float64(name):
    """At most 10 % of the samples are skipped for their conditioning; every other one fits its own k points far inside the
    bound (so the kernel must return a model for it), and numpy's float32 solve of it is close to the float64 one."""
    c, h = g.case(name), g.solo(name)
    assert not h.bad.any() and len(h.use) == 256
    d32 = g.distance(h.M32, h.M)
    r = d32[h.use] / (h.kappa[h.use] * 2.0 ** -24)
    print(f"{name}: {int((~h.use).sum())} of 256 samples skipped (kappa > {g.KAPPA_MAX:g}), kappa median {np.median(h.kappa):.1f} "
          f"max used {h.kappa[h.use].max():.0f}; numpy float32 distance / (kappa 2^-24): median {np.median(r):.2f} max {r.max():.2f}")
    assert (~h.use).mean() <= 0.10
    assert h.own[h.use].max() < c.bound / 100


def _where(t):
    return f"t* {t} (block {t // 256}, wavefront {t % 256 // 64}, lane {t % 64})"


@pytest.mark.parametrize("name", tuple(g.SEPARATED))
def test_separated_case_is_valid(name):
    """The validity condition, restated: S = max hi; t* the first t with lo = S; hi < S before it; every t with lo < S has
    hi <= S - 2.  Then the property that gives the case its name."""
    c = g.separated(name)
    k, T, lo, hi = g.K[c.model], c.T, c.lo, c.hi
    assert np.array_equal(c.p1, c.loc1[c.matches[:, 0]]) and np.array_equal(c.p2, c.loc2[c.matches[:, 1]])
    v = g.gate64(c.model, c.truth, c.p1, c.p2)
    assert v[c.planted].max() < c.bound / 100 and v[~c.planted].min() >= 4 * c.bound
    assert (hi >= lo).all()
    if c.kind == "dead":
        full = 256 * ((T + 255) // 256)
        assert T % 256 and len(lo) == full
        S_all = int(hi.max())
        assert S_all == c.S_all == int(c.planted.sum())
        assert not (lo[:T] == S_all).any() and (lo[T:] == S_all).any()
        assert c.S_live == int(hi[:T].max()) and k <= c.S_live < S_all
        print(f"{name}: seed {c.seed}, T {T}, dead lanes {np.flatnonzero(lo == S_all).tolist()} reach {S_all}, live ones at most {c.S_live}")
        return
    assert len(lo) == T
    S = int(hi.max())
    ties = np.flatnonzero(lo == S)
    assert len(ties) and S == c.S == int(c.planted.sum())
    ts = int(ties[0])
    assert ts == c.tstar and (hi[:ts] < S).all()
    assert hi[lo < S].max(initial=-2) <= S - 2
    assert g._established(c.kind, T, ts, ties)
    idx = g.samples(c.seed, T, k, c.n)
    assert np.array_equal(g.gate_many(c.model, g.solve(c.model, c.p1[idx[ts]], c.p2[idx[ts]], rank2=False), c.p1, c.p2) < c.bound / 2,
                          c.planted)
    if c.model == "F":
        for t in range(ts + 1):
            if c.planted[idx[t]].all():
                assert g._screen(c.model, c.p1, c.p2, c.planted, idx[t], c.bound), (name, t)
    print(f"{name}: seed {c.seed}, T {T}, S {S}, {_where(ts)}, {len(ties)} ties {ties[:6].tolist()}, "
          f"best of the others {int(hi[lo < S].max(initial=0))}")


def test_every_wrong_winner_rule_is_told_apart():
    told = {rule: [] for rule in g.WRONG_WINNER_RULES}
    for name in g.SEPARATED:
        c = g.separated(name)
        s = g.lane_scores(c)
        if c.kind == "dead":
            assert g.right_winner(s, c.T) < c.T
        else:
            assert g.right_winner(s, c.T) == c.tstar, name
        for rule, fn in g.WRONG_WINNER_RULES.items():
            t = fn(s, c.T)
            if (t >= c.T) if c.kind == "dead" else (t != c.tstar):
                told[rule].append(f"{name} ({t})")
    for rule, where in told.items():
        print(f"{rule}: {', '.join(where) or 'NOWHERE'}")
    assert all(told.values()), [r for r, w in told.items() if not w]


def test_noisy_scene_has_few_close_decisions():
    """A condition on the input, with the model's own float32 solve: at most 5 % of the hypotheses have a correspondence
    within 2 x guided_cases.margins of the bound, and the model's best hypothesis has none."""
    c = g.noisy()
    assert c.n == 200 and c.T == 512 and int(c.planted.sum()) == 100
    idx = g.samples(c.seed, c.T, 4, c.n)
    close, count = np.zeros(c.T, int), np.zeros(c.T, int)
    for t in range(c.T):
        M = g.solve("H", c.p1[idx[t]], c.p2[idx[t]], np.float32).astype(np.float32)
        if not np.isfinite(M).all():
            continue
        close[t] = int(g.near_bound("H", M, c.p1, c.p2, c.bound, 2.0).sum())
        count[t] = int((g.gate64("H", M, c.p1, c.p2) < c.bound).sum())
    best = int(np.argmax(count))
    print(f"noisy H: scene seed {g.NOISY_SCENE_SEED}, {int((close > 0).sum())} of {c.T} hypotheses with a close decision, best "
          f"hypothesis {best} with {count[best]} inliers, {len(np.unique(count))} different scores")
    assert (close > 0).mean() <= 0.05 and close[best] == 0
    assert count[best] >= 60 and len(np.unique(count)) >= 20          # a model to find, and a range of scores


def test_degenerate_inputs_are_what_they_say():
    for model in ("H", "F"):
        k = g.K[model]
        c = g.degenerate("same pair", model)
        assert len(np.unique(c.matches, axis=0)) == 1 and c.none
        c = g.degenerate("collinear", model)
        for p in (c.p1,) + ((c.p2,) if model == "F" else ()):
            assert np.abs(p[:, 1].astype(np.float64) - (0.5 * p[:, 0].astype(np.float64) + 20)).max() < 1e-3
        c = g.degenerate("repeated", model)
        rep = (c.matches == np.unique(c.matches, axis=0, return_counts=True)[0][
            np.argmax(np.unique(c.matches, axis=0, return_counts=True)[1])]).all(1)
        assert abs(rep.mean() - 0.6) < 0.02
        idx = g.samples(c.seed, c.T, k, len(c.matches))
        assert c.tstar is not None and c.tstar >= (1 if model == "H" else 0)
        assert (rep[idx[:c.tstar]].sum(1) <= 1).all() and rep[idx[c.tstar]].sum() <= 1
        h = g.hypotheses(model, c.p1, c.p2, c.seed, c.T, c.bound)
        S, ts, ties = g.winner(h.lo, h.hi)
        assert ts == c.tstar and S >= int(rep.sum()) + k - 1
        print(f"repeated {model}: seed {c.seed}, t* {c.tstar}, S {S} of {len(c.matches)}, {len(ties)} ties, "
              f"{int((rep[idx].sum(1) >= 2).sum())} of {c.T} samples with two copies or more")
        c = g.degenerate("all non-finite", model)
        assert not np.isfinite(c.p1).all(1).any() and c.none
        assert g.solve_many(model, c.p1[g.samples(c.seed, c.T, k, len(c.p1))], c.p2[g.samples(c.seed, c.T, k, len(c.p1))]).bad.all()
        c = g.degenerate("some non-finite", model)
        fin = np.isfinite(c.p1).all(1) & np.isfinite(c.p2).all(1)
        assert (~fin).sum() == 6 and np.isnan(c.loc1).any() and np.isinf(c.loc1).any() and np.isnan(c.loc2).any()


def test_which_planted_cases_pin_the_first_all_inlier_hypothesis():
    loose = tuple(name for name in g.PLANTED if not g.first_all_inlier_is_sound(name))
    print("the first all-inlier hypothesis does not pass the conditioning screen in:", loose or "no case")
    assert loose == g.FIRST_NOT_PINNED


def test_below_k_and_clean_cases():
    for name in g.BELOW:
        c = g.case(name)
        assert c.n == g.K[c.model] - 1 and len(c.matches) == c.n and not c.allin
    c = g.case("clean")
    assert c.planted.all() and c.n == 64
    M = g.solve64("H", c.p1[g.sample(c.seed, 0, 4, c.n)], c.p2[g.sample(c.seed, 0, 4, c.n)])
    assert g.gate64("H", M, c.p1, c.p2).max() < 1e-6
