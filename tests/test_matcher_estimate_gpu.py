"""Two-view geometry on the GPU (hess_matcher_estimate / _estimate_pairs, hess_geom.hip) on the inputs of
tests/geom_cases.py, which tests/test_geom_cases.py checks on the CPU: the planted model is found exactly, the mask is the
guided gate's decision on the returned matrix (held against the float64 gates of guided_cases outside their rounding margins),
ties go to the lowest hypothesis, the result is a function of the inputs, bank pairs equal single pairs, errors change
nothing."""
import ctypes as C

import numpy as np
import pytest

import geom_cases as g

pytestmark = pytest.mark.gpu


def _desc(n, salt):
    return np.random.RandomState(1234 + salt).randint(0, 60, size=(n, 128)).astype(np.uint8)


def _matcher(loc1, loc2, max_sift=8192):
    from hessgpu_amd.matcher import Matcher

    m = Matcher(0, max_sift=max_sift)
    _slots(m, loc1, loc2)
    return m


def _slots(m, loc1, loc2):
    m.set_descriptors(0, _desc(len(loc1), 0))
    m.set_descriptors(1, _desc(len(loc2), 1))
    m.set_locations(0, loc1)
    m.set_locations(1, loc2)


def _raw(m, matches, model, bound, hypotheses=0, seed=0):
    """hess_matcher_estimate -> (status, the result record, the mask bytes)."""
    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, _geom_params

    mt = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1, 2)
    p = _geom_params(model, bound, hypotheses, seed)
    res = np.full(1, -1, dtype=np.int8).repeat(GEOM_RESULT_DTYPE.itemsize).view(GEOM_RESULT_DTYPE)
    mask = np.full(max(len(mt), 1), 7, dtype=np.uint8)
    rc = m.L.hess_matcher_estimate(m.h, len(mt), mt.ctypes.data, p.ctypes.data, res.ctypes.data, mask.ctypes.data)
    return rc, res, mask[:len(mt)]


def _case_raw(m, c, seed=None):
    return _raw(m, c.matches, c.model, c.bound, c.T, c.seed if seed is None else seed)


@pytest.mark.parametrize("name", g.PLANTED)
def test_planted_model_is_found(name):
    c = g.case(name)
    m = _matcher(c.loc1, c.loc2)
    rc, res, mask = _case_raw(m, c)
    assert rc == 0
    assert m.last_ms() > 0
    m.close()
    M = res["M"][0].reshape(3, 3)
    hyp, inl = int(res["hypothesis"][0]), int(res["inliers"][0])
    print(f"{name}: hypothesis {hyp}, inliers {inl} of planted {int(c.planted.sum())}")
    if name in g.FIRST_NOT_PINNED:                       # (its first all-inlier sample is badly conditioned in float32)
        assert hyp in c.allin, (name, hyp, c.allin[:8])
    else:
        assert hyp == c.allin[0], (name, hyp, c.allin[:8])
    assert inl == int(c.planted.sum()) == int(mask.sum())
    assert np.array_equal(mask.astype(bool), c.planted) and set(np.unique(mask)) <= {0, 1}
    assert abs(np.linalg.norm(M.astype(np.float64)) - 1.0) <= 1e-6
    assert not res["reserved"].any()
    if c.model == "F":
        assert np.linalg.svd(M.astype(np.float64))[1][2] <= 1e-6
    # the mask against the independent model
    ok, band = g.decide64(c.model, M, c.p1, c.p2, c.bound)
    assert int(band.sum()) <= 2, (name, int(band.sum()))
    assert np.array_equal(mask.astype(bool)[~band], ok[~band])


def test_tie_goes_to_the_lowest_hypothesis():
    c = g.case("clean")
    m = _matcher(c.loc1, c.loc2)
    rc, res, mask = _case_raw(m, c)
    m.close()
    assert rc == 0 and int(res["hypothesis"][0]) == 0
    assert int(res["inliers"][0]) == c.n and mask.all()


@pytest.mark.parametrize("name", g.BELOW + ("empty H", "empty F"))
def test_below_k_there_is_no_model(name):
    c = g.case(name.replace("empty", "").strip() + " below k" if name.startswith("empty") else name)
    matches = c.matches[:0] if name.startswith("empty") else c.matches
    m = _matcher(c.loc1, c.loc2)
    rc, res, mask = _raw(m, matches, c.model, c.bound, c.T, 3)
    m.close()
    assert rc == 0
    assert int(res["hypothesis"][0]) == -1 and int(res["inliers"][0]) == 0
    assert not res["M"].any() and not res["reserved"].any() and not mask.any()


def test_result_is_a_function_of_the_inputs():
    for name in ("H 300", "F 300"):
        c = g.case(name)
        m = _matcher(c.loc1, c.loc2)
        a, b = _case_raw(m, c), _case_raw(m, c)
        assert a[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        # another seed whose all-inlier hypotheses are other indices
        other = next(s for s in range(c.seed + 1, c.seed + 1000)
                     if len(g.all_inlier(c.model, c.n, c.T, s, c.planted)) >= g.MIN_ALL_INLIER
                     and not set(g.all_inlier(c.model, c.n, c.T, s, c.planted)) & set(c.allin))
        rc, res, mask = _case_raw(m, c, seed=other)
        m.close()
        assert rc == 0 and int(res["hypothesis"][0]) in g.all_inlier(c.model, c.n, c.T, other, c.planted)
        assert int(res["hypothesis"][0]) != int(a[1]["hypothesis"][0])
        assert np.array_equal(mask.astype(bool), c.planted)


def _bank(model):
    """Four location sets and the pairs (0, 1), (1, 0), (2, 2), (0, 3) with their matches; (0, 3) has none."""
    big, small = g.case(f"{model} 300"), g.case(f"{model} 65")
    locs = [big.loc1, big.loc2, np.concatenate([small.loc1, small.loc2]),
            np.random.RandomState(9).rand(10, 2).astype(np.float32) * 100]
    shifted = small.matches + np.array([0, len(small.loc1)], np.int32)
    matches = [big.matches, np.ascontiguousarray(big.matches[:, ::-1]), np.ascontiguousarray(shifted, dtype=np.int32),
               np.zeros((0, 2), np.int32)]
    return locs, [(0, 1), (1, 0), (2, 2), (0, 3)], matches, big


def _same(got, ref):
    for q, ((M, mask, hyp), (rc, res, rmask)) in enumerate(zip(got, ref)):
        assert rc == 0
        assert M.tobytes() == res["M"][0].tobytes(), q
        assert np.array_equal(mask, rmask.astype(bool)) and hyp == int(res["hypothesis"][0]), q


@pytest.mark.parametrize("model", ("H", "F"))
def test_bank_pairs_equal_single_pairs(model):
    import torch

    from hessgpu_amd import HessError
    from hessgpu_amd.matcher import Matcher

    locs, pairs, matches, big = _bank(model)
    T, seed = big.T, big.seed
    single = Matcher(0, max_sift=4096)
    ref = []
    for p, ((a, b), mt) in enumerate(zip(pairs, matches)):
        _slots(single, locs[a], locs[b])
        ref.append(_raw(single, mt, model, big.bound, T, seed + p))
    single.close()
    assert np.array_equal(ref[0][2].astype(bool), big.planted) and int(ref[2][1]["hypothesis"][0]) >= 0
    assert int(ref[3][1]["hypothesis"][0]) == -1

    m = Matcher(0, max_sift=4096)
    sets = [_desc(len(a), k) for k, a in enumerate(locs)]
    m.set_bank(sets)
    m.set_bank_locations(locs)
    got = m.estimate_pairs(pairs, matches, model, big.bound, hypotheses=T, seed=seed)
    assert m.last_ms() > 0
    _same(got, ref)
    # the raw call with a max_match above every count: the rest of each mask row is zero
    mm = 320
    buf, cnt = np.zeros((4, mm, 2), np.int32), np.array([len(x) for x in matches], np.int32)
    for k, x in enumerate(matches):
        buf[k, :len(x)] = x
    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, _geom_params
    prm, res = _geom_params(model, big.bound, T, seed), np.zeros(4, GEOM_RESULT_DTYPE)
    mask = np.full((4, mm), 9, np.uint8)
    ab = np.array(pairs, np.int32)
    assert m.L.hess_matcher_estimate_pairs(m.h, 4, ab.ctypes.data, mm, buf.ctypes.data, cnt.ctypes.data, prm.ctypes.data,
                                           res.ctypes.data, mask.ctypes.data) == 0
    for q in range(4):
        assert res[q].tobytes() == ref[q][1].tobytes()
        assert np.array_equal(mask[q, :cnt[q]], ref[q][2]) and not mask[q, cnt[q]:].any()
    # typed storage: the locations stay in the caller's order
    m.set_bank_types([np.random.RandomState(k).randint(0, 4, size=len(a)).astype(np.uint16) for k, a in enumerate(locs)])
    _same(m.estimate_pairs(pairs, matches, model, big.bound, hypotheses=T, seed=seed), ref)
    m.set_bank_types(None)
    # locations from key records on the device, 24 bytes apart
    keys = np.zeros((sum(len(a) for a in locs), 6), np.float32)
    keys[:, :2] = np.concatenate(locs)
    keys[:, 2:] = 1e30
    dk = torch.from_numpy(keys).to("cuda:0")
    torch.cuda.synchronize()
    m.set_bank_locations(None)
    with pytest.raises(HessError) as e:
        m.estimate_pairs(pairs, matches, model, big.bound, hypotheses=T, seed=seed)
    assert e.value.code == -5
    m.set_bank_locations_device(dk.data_ptr(), 24)
    _same(m.estimate_pairs(pairs, matches, model, big.bound, hypotheses=T, seed=seed), ref)
    # loading descriptors again removes the locations
    m.set_bank(sets)
    with pytest.raises(HessError) as e:
        m.estimate_pairs(pairs, matches, model, big.bound, hypotheses=T, seed=seed)
    assert e.value.code == -5 and "locations" in str(e.value)
    m.close()


def test_bank_locations_are_cut_at_max_sift_like_the_descriptors():
    """Sets longer than max_sift: the locations of the rows kept, set by set, although the caller's records are back to back
    at their full counts (host and device form)."""
    import torch

    from hessgpu_amd.matcher import Matcher

    c = g.case("H 65")                                           # 72 and 68 rows
    cut = 60
    locs = [c.loc1, c.loc2, c.loc1[::-1].copy()]
    keep = c.matches[(c.matches < cut).all(1)]
    assert len(keep) >= 30
    pairs, matches = [(0, 1), (2, 1)], [keep, np.ascontiguousarray(np.stack([71 - c.matches[:, 0], c.matches[:, 1]], 1))]
    matches[1] = matches[1][(matches[1] < cut).all(1)]
    single = Matcher(0, max_sift=cut)
    ref = []
    for p, ((a, b), mt) in enumerate(zip(pairs, matches)):
        _slots(single, locs[a], locs[b])
        ref.append(_raw(single, mt, "H", c.bound, c.T, 5 + p))
    single.close()
    assert all(int(r[1]["hypothesis"][0]) >= 0 for r in ref)
    m = Matcher(0, max_sift=cut)
    m.set_bank([_desc(len(a), k) for k, a in enumerate(locs)])
    m.set_bank_locations(locs)
    _same(m.estimate_pairs(pairs, matches, "H", c.bound, hypotheses=c.T, seed=5), ref)
    wide = np.ascontiguousarray(np.concatenate([np.concatenate(locs), np.full((sum(map(len, locs)), 1), 3.0, np.float32)], 1))
    dw = torch.from_numpy(wide).to("cuda:0")
    torch.cuda.synchronize()
    m.set_bank_locations_device(dw.data_ptr(), 12)
    _same(m.estimate_pairs(pairs, matches, "H", c.bound, hypotheses=c.T, seed=5), ref)
    # a match that names a row beyond the cut is outside its set
    from hessgpu_amd import HessError
    with pytest.raises(HessError) as e:
        m.estimate_pairs(pairs, [c.matches, matches[1]], "H", c.bound, hypotheses=c.T, seed=5)
    assert e.value.code == -1
    m.close()


def test_errors_change_nothing():
    import torch

    from hessgpu_amd.matcher import GEOM_RESULT_DTYPE, Matcher, _geom_params

    locs, pairs, matches, big = _bank("H")
    c = big
    m = Matcher(0, max_sift=4096)
    L, h = m.L, m.h
    prm = _geom_params("H", c.bound, c.T, c.seed)
    res = np.zeros(4, GEOM_RESULT_DTYPE)
    mt = c.matches
    mm = 320
    buf, cnt = np.zeros((4, mm, 2), np.int32), np.array([len(x) for x in matches], np.int32)
    for k, x in enumerate(matches):
        buf[k, :len(x)] = x
    ab = np.array(pairs, np.int32)
    flat = np.ascontiguousarray(np.concatenate(locs))

    def refused(code, word, fn, *args):
        assert fn(h, *args) == code, (fn.__name__, word)
        assert word in (L.hess_matcher_last_error(h) or b"").decode(), (word, L.hess_matcher_last_error(h))
        if baseline:                                     # the next valid call answers as before
            again = _case_raw(m, c)
            assert again[0] == 0 and again[1].tobytes() == baseline[0][1].tobytes() and again[2].tobytes() == baseline[0][2].tobytes()

    baseline = []

    def est(p=prm, n=None, mtc=mt, out=res):
        return (len(mtc) if n is None else n, mtc.ctypes.data, None if p is None else p.ctypes.data,
                None if out is None else out.ctypes.data, None)

    def estp(p=prm, abp=ab, cn=cnt, bf=buf, out=res, maxm=mm):
        return (len(abp), abp.ctypes.data, maxm, bf.ctypes.data, cn.ctypes.data, None if p is None else p.ctypes.data,
                None if out is None else out.ctypes.data, None)

    # no locations yet: slots without descriptors, slots with descriptors only, a bank that is not loaded
    refused(-5, "locations", L.hess_matcher_estimate, *est())
    refused(-5, "descriptors", L.hess_matcher_bank_set_locations, flat.ctypes.data, 8)
    refused(-5, "descriptors", L.hess_matcher_bank_set_locations_device, flat.ctypes.data, 8)
    m.set_descriptors(0, _desc(len(c.loc1), 0))
    m.set_descriptors(1, _desc(len(c.loc2), 1))
    m.set_locations(0, c.loc1)
    refused(-5, "slot 1", L.hess_matcher_estimate, *est())
    m.set_locations(1, c.loc2)
    m.set_bank([_desc(len(a), k) for k, a in enumerate(locs)])
    refused(-5, "locations", L.hess_matcher_estimate_pairs, *estp())
    m.set_bank_locations(locs)
    good = _case_raw(m, c)
    good_pairs = m.estimate_pairs(pairs, matches, "H", c.bound, hypotheses=c.T, seed=c.seed)
    assert good[0] == 0 and np.array_equal(good[2].astype(bool), c.planted)
    baseline.append(good)

    def bad(**kw):
        p = prm.copy()
        for k, v in kw.items():
            p[k] = v
        return p

    reserved = prm.copy()
    reserved["reserved"][0, 2] = 1
    for word, p in (("params", None), ("model", bad(model=0)), ("model", bad(model=3)), ("hypotheses", bad(hypotheses=-1)),
                    ("hypotheses", bad(hypotheses=65537)), ("reserved", reserved), ("bound", bad(bound=0.0)),
                    ("bound", bad(bound=-1.0)), ("bound", bad(bound=np.inf)), ("bound", bad(bound=np.nan))):
        refused(-1, word, L.hess_matcher_estimate, *est(p=p))
        refused(-1, word, L.hess_matcher_estimate_pairs, *estp(p=p))
    refused(-1, "out", L.hess_matcher_estimate, *est(out=None))
    refused(-1, "out", L.hess_matcher_estimate_pairs, *estp(out=None))
    for i, col, v in ((0, 0, -1), (5, 0, len(c.loc1)), (299, 1, len(c.loc2)), (7, 1, -3)):
        wrong = mt.copy()
        wrong[i, col] = v
        refused(-1, f"match {i}", L.hess_matcher_estimate, *est(mtc=wrong))
        wb = buf.copy()
        wb[0, i, col] = v
        refused(-1, f"match {i} of pair 0", L.hess_matcher_estimate_pairs, *estp(bf=wb))
    for q, v in ((0, 4), (3, -1)):
        wab = ab.copy()
        wab.reshape(-1)[q] = v
        refused(-1, "outside the bank", L.hess_matcher_estimate_pairs, *estp(abp=wab))
    for q, v in ((1, -1), (2, mm + 1)):
        wc = cnt.copy()
        wc[q] = v
        refused(-1, f"counts[{q}]", L.hess_matcher_estimate_pairs, *estp(cn=wc))
    for stride in (0, 4, 6, 10, 23):
        refused(-1, "stride_bytes", L.hess_matcher_bank_set_locations, flat.ctypes.data, stride)
        refused(-1, "stride_bytes", L.hess_matcher_bank_set_locations_device, flat.ctypes.data, stride)
    refused(-1, "device memory", L.hess_matcher_bank_set_locations_device, flat.ctypes.data, 8)
    dl = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.synchronize()
    refused(-1, "aligned", L.hess_matcher_bank_set_locations_device, dl.data_ptr() + 2, 8)
    refused(-1, "allocation", L.hess_matcher_bank_set_locations_device, dl.data_ptr(), 1 << 26)
    # nothing changed: the slots' and the bank's answers are the ones from before
    again = _case_raw(m, c)
    assert again[0] == 0 and again[1].tobytes() == good[1].tobytes() and again[2].tobytes() == good[2].tobytes()
    for (M, mask, hyp), (M0, mask0, hyp0) in zip(m.estimate_pairs(pairs, matches, "H", c.bound, hypotheses=c.T, seed=c.seed), good_pairs):
        assert M.tobytes() == M0.tobytes() and np.array_equal(mask, mask0) and hyp == hyp0
    # set_dim to the other length removes the bank's locations with everything else
    baseline.clear()
    m.set_dim(64)
    refused(-5, "locations", L.hess_matcher_estimate_pairs, *estp())
    refused(-5, "locations", L.hess_matcher_estimate, *est())
    m.close()


def test_estimate_geometry_of_the_siftgpu_surface():
    """SiftMatchGPU::EstimateGeometry through its flat mirror equals the C ABI."""
    import siftgpu_lib

    for name in ("H 65", "F 65"):
        c = g.case(name)
        m = _matcher(c.loc1, c.loc2)
        rc, res, mask = _case_raw(m, c)
        m.close()
        assert rc == 0
        L = siftgpu_lib.lib()
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        for fn, rt, args in [("siftmatch_create", vp, [i32]), ("siftmatch_destroy", None, [vp]),
                             ("siftmatch_set_descriptors_u8", None, [vp, i32, i32, vp]),
                             ("siftmatch_set_locations", None, [vp, i32, vp, i32]),
                             ("siftmatch_estimate", i32, [vp, i32, i32, vp, vp, f32, vp, i32, C.c_uint])]:
            getattr(L, fn).restype = rt
            getattr(L, fn).argtypes = args
        hnd = L.siftmatch_create(4096)
        d1, d2 = _desc(len(c.loc1), 0), _desc(len(c.loc2), 1)
        L.siftmatch_set_descriptors_u8(hnd, 0, len(d1), d1.ctypes.data)
        L.siftmatch_set_descriptors_u8(hnd, 1, len(d2), d2.ctypes.data)
        L.siftmatch_set_locations(hnd, 0, c.loc1.ctypes.data, 0)
        L.siftmatch_set_locations(hnd, 1, c.loc2.ctypes.data, 0)
        M, inl = np.full(9, 5, np.float32), np.full(c.n, 5, np.uint8)
        n = L.siftmatch_estimate(hnd, g.MODEL_ID[c.model], c.n, c.matches.ctypes.data, M.ctypes.data, c.bound, inl.ctypes.data,
                                 c.T, c.seed)
        assert n == int(res["inliers"][0]) == int(c.planted.sum())
        assert M.tobytes() == res["M"][0].tobytes() and np.array_equal(inl, mask)
        # an error (an unknown model) and a pair without a model: 0 and a zero matrix
        assert L.siftmatch_estimate(hnd, 7, c.n, c.matches.ctypes.data, M.ctypes.data, c.bound, None, c.T, c.seed) == 0
        assert not M.any()
        assert L.siftmatch_estimate(hnd, g.MODEL_ID[c.model], 2, c.matches.ctypes.data, M.ctypes.data, c.bound, None, 0, 0) == 0
        assert not M.any()
        L.siftmatch_destroy(hnd)
