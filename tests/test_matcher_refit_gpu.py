"""The estimator's least-squares refit (hess_geom_params.refit; include/hess_abi.h, step 6; geom_refit_kernel in hess_geom.hip)
through the ABI as it is, held to the float64 model of tests/refit_cases.py (checked on the CPU by tests/test_refit_cases.py).

Step by step: for R = 1, 2, 3 the call with refit = R is compared with the float64 candidate formed from the mask and the matrix
that the device itself returned for refit = R - 1.  Where the model's count interval says accept, the device's matrix lies within
8 x 2^-24 of the candidate in Frobenius norm (2^-24: one float32 rounding of a unit-norm matrix; 8: the factor of the estimator's
own tests; the eigen solve in double adds about 1e-15 kappa, below it for the kappa <= 1e6 that every step is asserted to have), has
the rule's sign, counts as one more refit, and its mask is the gate on the returned matrix.  Where it says reject, or the rule
stopped before (too few inliers, a degenerate normalisation, the same mask twice), the bytes are those of refit = R - 1.  An
undecided step (the interval straddles the count before) is skipped; test_few_steps_were_skipped bounds them.

Measured on an MI355X: profiles/r20_refit.txt."""
import ctypes as C

import numpy as np
import pytest

import geom_cases as g
import refit_cases as rc

pytestmark = pytest.mark.gpu

STATS = {"steps": 0, "skipped": 0, "ratio": 0.0, "where": None}
NOISY = [k + (s,) for k, s in rc.NOISY.items()] + [rc.REJECTED]
EXACT = tuple(g.PLANTED) + ("clean",)


def _desc(n, salt):
    return np.random.RandomState(1234 + salt).randint(0, 60, size=(n, 128)).astype(np.uint8)


def _slots(m, loc1, loc2):
    m.set_descriptors(0, _desc(len(loc1), 0))
    m.set_descriptors(1, _desc(len(loc2), 1))
    m.set_locations(0, loc1)
    m.set_locations(1, loc2)


def _matcher(loc1, loc2, max_sift=8192):
    from hessgpu_amd.matcher import Matcher

    m = Matcher(0, max_sift=max_sift)
    _slots(m, loc1, loc2)
    return m


def _raw(m, matches, model, bound, hypotheses, seed, refit):
    """hess_matcher_estimate -> (status, the result record, the mask bytes); the outputs start from a pattern."""
    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, _geom_params

    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2)
    p = _geom_params(model, bound, hypotheses, seed, refit)
    res = np.full(1, -1, dtype=np.int8).repeat(GEOM_RESULT_DTYPE.itemsize).view(GEOM_RESULT_DTYPE)
    mask = np.full(max(len(mt), 1), 7, dtype=np.uint8)
    rc_ = m.L.hess_matcher_estimate(m.h, len(mt), mt.ctypes.data, p.ctypes.data, res.ctypes.data, mask.ctypes.data)
    return rc_, res, mask[:len(mt)]


def _call(m, c, refit):
    return _raw(m, c.matches, c.model, c.bound, c.T, c.seed, refit)


def _fields(r):
    res = r[1]
    return (res["M"][0].reshape(3, 3), int(res["inliers"][0]), int(res["hypothesis"][0]), int(res["reserved"][0, 0]),
            int(res["reserved"][0, 1]))


def _same(a, b):
    """The matrix, the mask, the counts and the number of refits, byte for byte."""
    return a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _mask_is_the_gate(c, M, mask, inl):
    assert set(np.unique(mask)) <= {0, 1} and inl == int(mask.sum())
    ok, band = g.decide64(c.model, M, c.p1, c.p2, c.bound)
    assert np.array_equal(mask.astype(bool)[~band], ok[~band]), c.name


def _step_by_step(c, conditioned=True):
    """The check of the module's docstring on case c -> the calls with refit = 0..3.  conditioned: kappa <= 1e6 is a condition on
    the input and asserted; without it a step above 1e6 (k exact points: lambda_2 is as small as the sample is close to
    degenerate) is held to everything but the distance, which is promised up to 1e6 only."""
    m = _matcher(c.loc1, c.loc2)
    calls = [_call(m, c, 0)]
    assert calls[0][0] == 0
    M0, inl0, hyp0, refits0, first0 = _fields(calls[0])
    assert refits0 == 0 and first0 == 0
    stopped = False                                      # the rule ended at an earlier step
    for R in (1, 2, 3):
        prev, cur = calls[-1], _call(m, c, R)
        calls.append(cur)
        assert cur[0] == 0
        Mp, inlp, hypp, refp, _ = _fields(prev)
        M, inl, hyp, refits, first = _fields(cur)
        assert hyp == hyp0
        if hyp0 < 0:
            assert not cur[1]["reserved"].any() and cur[1]["M"].tobytes() == prev[1]["M"].tobytes() and not cur[2].any()
            continue
        assert first == inl0
        if stopped or refp < R - 1:
            assert cur[1]["M"].tobytes() == prev[1]["M"].tobytes() and cur[2].tobytes() == prev[2].tobytes() and refits == refp, (c.name, R)
            continue
        st = rc.step64(c.model, c.p1, c.p2, prev[2].astype(bool), Mp, c.bound)
        STATS["steps"] += 1
        if st.stop is not None or st.verdict == "reject":
            stopped = True
            assert cur[1]["M"].tobytes() == prev[1]["M"].tobytes() and cur[2].tobytes() == prev[2].tobytes() and refits == refp, \
                (c.name, R, st.stop)
            continue
        assert st.kappa <= rc.MAX_KAPPA or not conditioned, (c.name, R, st.kappa)
        if st.verdict == "undecided":
            STATS["skipped"] += 1
            stopped = refits == refp                     # (whichever way the device decided, the later steps follow it)
            continue
        d = float(np.linalg.norm(M.astype(np.float64) - st.C))
        if st.kappa > rc.MAX_KAPPA:
            print(f"{c.name}, step {R}: kappa {st.kappa:.3g} above 1e6, |M - C|_F / (8 x 2^-24) = {d / rc.TOL:.4f} not asserted")
        else:
            if d / rc.TOL > STATS["ratio"]:
                STATS["ratio"], STATS["where"] = d / rc.TOL, (c.name, R, st.kappa)
            assert d <= rc.TOL, (c.name, R, d, rc.TOL, st.kappa)
        assert (M.astype(np.float64) * Mp.astype(np.float64)).sum() >= 0
        assert refits == R and inl >= inlp
        _mask_is_the_gate(c, M, cur[2], inl)
        stopped = np.array_equal(cur[2], prev[2])        # the same set: the rule stops after accepting
    again = _call(m, c, 3)
    m.close()
    assert _same(again, calls[3])                        # a function of the inputs
    return calls


@pytest.mark.parametrize("key", NOISY, ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{k[3]}")
def test_noisy_step_by_step_never_worse_and_better(key):
    c = rc.noisy(*key)
    calls = _step_by_step(c)
    m = _matcher(c.loc1, c.loc2)
    four = _call(m, c, 4)
    m.close()
    M0, inl0, hyp0, _, _ = _fields(calls[0])
    M4, inl4, hyp4, refits4, first4 = _fields(four)
    assert four[0] == 0 and hyp0 >= 0
    assert inl4 >= inl0 and first4 == inl0 and hyp4 == hyp0 and 1 <= refits4 <= 4
    _mask_is_the_gate(c, M4, four[2], inl4)
    before, after = rc.rms(c, M0), rc.rms(c, M4)
    print(f"{c.name}: inliers {inl0} -> {inl4} of {int(c.planted.sum())} planted, {refits4} refits, rms gate value on the noise-free "
          f"inliers {before:.4f} -> {after:.4f}, refits of the calls 1..3: {[_fields(r)[3] for r in calls[1:]]}")
    if key[:3] in rc.QUALITY and key != rc.REJECTED:
        assert after < before, (c.name, before, after)


@pytest.mark.parametrize("model", ("H", "F"))
@pytest.mark.parametrize("n", rc.SEAMS)
def test_seams_step_by_step(model, n):
    """Lists cut from the 5000-match cases: k, the lane stride and the wavefront tail (255, 256, 257), the LDS chunk (2048,
    2049)."""
    c = rc.sublist(f"{model} 5000", g.K[model] if n is None else n)
    calls = _step_by_step(c)
    print(f"{c.name}: inliers {[_fields(r)[1] for r in calls]}, refits {[_fields(r)[3] for r in calls]}")
    m = _matcher(c.loc1, c.loc2)
    four = _call(m, c, 4)
    m.close()
    assert four[0] == 0 and _fields(four)[1] >= _fields(calls[0])[1] and _fields(four)[2] == _fields(calls[0])[2]
    if n is not None:                                    # (exact inliers: the first refit is accepted)
        assert _fields(calls[0])[2] >= 0 and _fields(calls[1])[3] == 1


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_are_a_fixed_point(name):
    c = g.case(name)
    calls = _step_by_step(c, conditioned=False)
    m = _matcher(c.loc1, c.loc2)
    eight = _call(m, c, 8)
    m.close()
    M, inl, hyp, refits, first = _fields(eight)
    assert eight[0] == 0 and refits == 1 and first == _fields(calls[0])[1] == inl
    assert eight[2].tobytes() == calls[0][2].tobytes() and _same(eight, calls[1])


@pytest.mark.parametrize("name", g.BELOW)
def test_below_k_has_no_model(name):
    c = g.case(name)
    m = _matcher(c.loc1, c.loc2)
    r = _call(m, c, 4)
    m.close()
    M, inl, hyp, refits, first = _fields(r)
    assert r[0] == 0 and hyp == -1 and inl == 0 and not M.any() and not r[2].any() and refits == 0 and first == 0


@pytest.mark.parametrize("model", ("H", "F"))
def test_three_hundred_bank_pairs_equal_single_pairs(model):
    """256 pairs per chunk: pairs 250..260 alternate n >= k and n < k, 280..299 are all below k.  Every pair equals the single-
    pair call with seed + p byte for byte, refit = 2; for H the bank's locations then come through the device form as well."""
    import torch

    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, Matcher

    c = rc.noisy(model, 65, 1.0, rc.NOISY[(model, 65, 1.0)])
    k, T, refit = g.K[model], 64, 2
    locs = [c.loc1, c.loc2]
    below = [c.matches[:k - 1], c.matches[:0], c.matches[:1]]
    matches = []
    for p in range(300):
        small = (250 <= p <= 260 and p % 2 == 1) or p >= 280
        matches.append(below[p % 3] if small else c.matches[:c.n - p % 5])
    single = _matcher(c.loc1, c.loc2, 4096)
    ref = [_raw(single, mt, model, c.bound, T, c.seed + p, refit) for p, mt in enumerate(matches)]
    single.close()
    m = Matcher(0, max_sift=4096)
    m.set_bank([_desc(len(a), q) for q, a in enumerate(locs)])

    def check():
        got = m.estimate_pairs([(0, 1)] * 300, matches, model, c.bound, hypotheses=T, seed=c.seed, refit=refit, info=True)
        refitted = 0
        for p, ((M, mask, hyp, info), (rc_, res, rmask)) in enumerate(zip(got, ref)):
            assert rc_ == 0 and M.tobytes() == res["M"][0].tobytes() and hyp == int(res["hypothesis"][0]), p
            assert np.array_equal(mask, rmask.astype(bool)), p
            assert info == {"inliers": int(res["inliers"][0]), "refits": int(res["reserved"][0, 0]),
                            "ransac_inliers": int(res["reserved"][0, 1])}, p
            if len(matches[p]) < k:
                assert hyp == -1 and not M.any() and info == {"inliers": 0, "refits": 0, "ransac_inliers": 0}, p
            refitted += info["refits"] > 0
        return refitted

    m.set_bank_locations(locs)
    refitted = check()
    print(f"{model}: {refitted} of 300 pairs with an accepted refit")
    assert refitted >= 30
    if model == "H":
        keys = np.full((sum(len(a) for a in locs), 6), 1e30, np.float32)
        keys[:, :2] = np.concatenate(locs)
        dk = torch.from_numpy(keys).to("cuda:0")
        torch.cuda.synchronize()
        m.set_bank_locations(None)
        m.set_bank_locations_device(dk.data_ptr(), 24)
        assert check() == refitted
    m.close()
    assert GEOM_RESULT_DTYPE.itemsize == 52


@pytest.mark.parametrize("model", ("H", "F"))
@pytest.mark.parametrize("kind", g.DEGENERATE)
def test_degenerate_input(kind, model):
    c = g.degenerate(kind, model)
    m = _matcher(c.loc1, c.loc2)
    zero, two, again = _call(m, c, 0), _call(m, c, 2), _call(m, c, 2)
    m.close()
    assert zero[0] == two[0] == 0 and _same(two, again)
    M0, inl0, hyp0, _, _ = _fields(zero)
    M, inl, hyp, refits, first = _fields(two)
    print(f"{c.name}: hypothesis {hyp}, inliers {inl0} -> {inl} of {len(c.matches)}, {refits} refits")
    assert hyp == hyp0 and inl >= inl0 and 0 <= refits <= 2
    assert set(np.unique(two[2])) <= {0, 1} and inl == int(two[2].sum())
    if hyp < 0:
        assert not M.any() and not two[2].any() and refits == 0 and first == 0
    else:
        assert first == inl0 and np.isfinite(M).all() and abs(np.linalg.norm(M.astype(np.float64)) - 1.0) <= 1e-6
        ok, band = g.decide64(c.model, M, c.p1, c.p2, c.bound)
        assert np.array_equal(two[2].astype(bool)[~band], ok[~band])
    # Coincident points: every sample has a mean distance of zero, its hypothesis is not finite and scores 0, so there is no
    # model and the refit never starts.  The stop of step b needs inliers that coincide under a finite model, which the gate
    # does not produce; the stop itself is run on the header's host form (tests/test_geom_refit_cpu.py).
    if kind == "same pair":
        assert hyp == -1 and refits == 0


def test_arguments():
    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, _geom_params

    c = g.case("H 65")
    m = _matcher(c.loc1, c.loc2)
    L, h = m.L, m.h
    res = np.zeros(1, GEOM_RESULT_DTYPE)
    good = _call(m, c, 1)

    def refused(word, p):
        assert L.hess_matcher_estimate(h, c.n, c.matches.ctypes.data, p.ctypes.data, res.ctypes.data, None) == -1, word
        assert word in (L.hess_matcher_last_error(h) or b"").decode(), (word, L.hess_matcher_last_error(h))
        ab, cnt = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)
        assert L.hess_matcher_estimate_pairs(h, 1, ab.ctypes.data, 0, None, cnt.ctypes.data, p.ctypes.data, res.ctypes.data, None) == -1
        assert word in (L.hess_matcher_last_error(h) or b"").decode(), (word, L.hess_matcher_last_error(h))

    for refit in (-1, 9, 1 << 20):
        refused("refit", _geom_params("H", c.bound, c.T, c.seed, refit))
    for word in (1, 2, 3):
        for refit in (0, 1):
            p = _geom_params("H", c.bound, c.T, c.seed, refit)
            p["reserved"][0, word] = 1
            refused("reserved", p)
    again, zero = _call(m, c, 1), _call(m, c, 0)
    m.close()
    assert _same(again, good) and _fields(good)[3] == 1 and _fields(good)[4] == _fields(zero)[1]
    assert zero[0] == 0 and not zero[1]["reserved"].any()


def test_python_surface():
    c = rc.noisy("F", 300, 0.5, rc.NOISY[("F", 300, 0.5)])
    m = _matcher(c.loc1, c.loc2)
    raw0, raw4 = _call(m, c, 0), _call(m, c, 4)
    plain = m.estimate(c.matches, "F", c.bound, hypotheses=c.T, seed=c.seed)
    three = m.estimate(c.matches, "F", c.bound, hypotheses=c.T, seed=c.seed, refit=4)
    four = m.estimate(c.matches, "F", c.bound, hypotheses=c.T, seed=c.seed, refit=4, info=True)
    m.close()
    assert len(plain) == 3 and plain[0].tobytes() == raw0[1]["M"][0].tobytes() and np.array_equal(plain[1], raw0[2].astype(bool))
    assert len(three) == 3 and len(four) == 4 and three[0].tobytes() == four[0].tobytes() == raw4[1]["M"][0].tobytes()
    assert np.array_equal(four[1], raw4[2].astype(bool)) and four[2] == plain[2]
    M, inl, hyp, refits, first = _fields(raw4)
    assert four[3] == {"inliers": inl, "refits": refits, "ransac_inliers": first} and refits >= 1 and first == _fields(raw0)[1]


def test_class_and_flat_surfaces():
    """siftmatch_estimate_refit returns the bytes of hess_matcher_estimate; siftmatch_estimate what it did before."""
    import siftgpu_lib

    c = rc.noisy("F", 65, 0.5, rc.NOISY[("F", 65, 0.5)])
    m = _matcher(c.loc1, c.loc2)
    zero, two = _call(m, c, 0), _call(m, c, 2)
    m.close()
    assert zero[0] == two[0] == 0 and _fields(two)[3] >= 1
    L = siftgpu_lib.lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    for fn, rt, args in [("siftmatch_create", vp, [i32]), ("siftmatch_destroy", None, [vp]),
                         ("siftmatch_set_descriptors_u8", None, [vp, i32, i32, vp]),
                         ("siftmatch_set_locations", None, [vp, i32, vp, i32]),
                         ("siftmatch_estimate", i32, [vp, i32, i32, vp, vp, f32, vp, i32, C.c_uint]),
                         ("siftmatch_estimate_refit", i32, [vp, i32, i32, vp, vp, f32, vp, i32, C.c_uint, i32])]:
        getattr(L, fn).restype = rt
        getattr(L, fn).argtypes = args
    hnd = L.siftmatch_create(4096)
    d1, d2 = _desc(len(c.loc1), 0), _desc(len(c.loc2), 1)
    L.siftmatch_set_descriptors_u8(hnd, 0, len(d1), d1.ctypes.data)
    L.siftmatch_set_descriptors_u8(hnd, 1, len(d2), d2.ctypes.data)
    L.siftmatch_set_locations(hnd, 0, c.loc1.ctypes.data, 0)
    L.siftmatch_set_locations(hnd, 1, c.loc2.ctypes.data, 0)
    args = (hnd, g.MODEL_ID[c.model], c.n, c.matches.ctypes.data)
    for want, call in ((two, lambda M, inl: L.siftmatch_estimate_refit(*args, M.ctypes.data, c.bound, inl.ctypes.data, c.T, c.seed, 2)),
                       (zero, lambda M, inl: L.siftmatch_estimate_refit(*args, M.ctypes.data, c.bound, inl.ctypes.data, c.T, c.seed, 0)),
                       (zero, lambda M, inl: L.siftmatch_estimate(*args, M.ctypes.data, c.bound, inl.ctypes.data, c.T, c.seed))):
        M, inl = np.full(9, 5, np.float32), np.full(c.n, 5, np.uint8)
        n = call(M, inl)
        assert n == int(want[1]["inliers"][0]) and M.tobytes() == want[1]["M"][0].tobytes() and np.array_equal(inl, want[2])
    M = np.full(9, 5, np.float32)
    assert L.siftmatch_estimate_refit(*args, M.ctypes.data, c.bound, None, c.T, c.seed, 9) == 0 and not M.any()      # refused
    L.siftmatch_destroy(hnd)


def test_few_steps_were_skipped():
    """Over the whole file at most one step in ten may be undecided; none is expected.  Selected alone (or in a worker of its
    own) it walks the noisy cases itself, so it never passes on nothing."""
    if not STATS["steps"]:
        for key in NOISY:
            _step_by_step(rc.noisy(*key))
    assert STATS["steps"] > 0
    print(f"{STATS['steps']} steps compared with float64, {STATS['skipped']} undecided; largest |M - C|_F / (8 x 2^-24): "
          f"{STATS['ratio']:.4f} at {STATS['where']}")
    assert 10 * STATS["skipped"] <= STATS["steps"]
