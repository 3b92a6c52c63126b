"""Guided matching on the GPU (match_dot_kernel with gates, hess_matcher_set_locations, SiftMatchGPU::GetGuidedSiftMatch)
against the CPU oracle on the inputs of tests/guided_cases.py, which tests/test_guided_cases.py checks on the CPU: no gate
decision depends on float32 rounding, the oracle equals an independent float64 model, results are not empty, differ from
the unguided ones and show the 8-row-block leak.  Integer results: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import guided_cases as gc
import matcher_cases as mc
from oracle_lib import oracle_match

pytestmark = pytest.mark.gpu


def _load(m, c):
    m.set_descriptors(0, c.d1)
    m.set_descriptors(1, c.d2)
    m.set_locations(0, c.loc1)
    m.set_locations(1, c.loc2)


def _kw(h, f, dm, rm, mutual, max_match):
    return dict(hdistmax=h, fdistmax=f, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=max_match)


def _oracle(c, H, F, **kw):
    return oracle_match(c.d1, c.d2, c.loc1, c.loc2, H, F, **kw)


@pytest.mark.parametrize("n1,n2,geometry", gc.CASES)
def test_guided_match_equals_the_oracle(n1, n2, geometry):
    """Every threshold pair and configuration, at full length and with a max_match below the count."""
    from hessgpu_amd.matcher import Matcher

    cs = (n1, n2, geometry)
    c = gc.case(*cs)
    m = Matcher(0, max_sift=max(n1, n2))
    _load(m, c)
    for k, (h, f) in enumerate(gc.pick_thresholds(*cs)):
        for dm, rm, mutual in gc.CONFIGS:
            ref = _oracle(c, c.H, c.F, **_kw(h, f, dm, rm, mutual, n1))
            assert (len(ref) == 0) == ((cs, k) in gc.EMPTY), (cs, h, f, dm, rm, mutual, len(ref))
            got = m.match(H=c.H, F=c.F, **_kw(h, f, dm, rm, mutual, n1))
            assert np.array_equal(got, ref), (cs, h, f, dm, rm, mutual, mc.first_difference(ref, got))
            cut = len(ref) // 2
            if cut:
                got = m.match(H=c.H, F=c.F, **_kw(h, f, dm, rm, mutual, cut))
                assert len(got) == cut and np.array_equal(got, ref[:cut]), (cs, h, f, dm, rm, mutual, cut)
    m.close()


def test_locations_with_a_gap_and_cut_at_max_sift():
    from hessgpu_amd.matcher import Matcher

    cs = (300, 333, "projective")
    c = gc.case(*cs)
    h, f = gc.pick_thresholds(*cs)[0]
    kw = _kw(h, f, 2.0, 2.0, False, 300)
    ref = _oracle(c, c.H, c.F, **kw)
    m = Matcher(0, max_sift=400)
    _load(m, c)
    rng = np.random.RandomState(3)
    for gap in (0, 3):           # (x, y) and `gap` floats that must not be read as locations
        wide = [np.concatenate([l, rng.rand(len(l), gap).astype(np.float32) * 999], 1) for l in (c.loc1, c.loc2)]
        m.set_locations(0, wide[0], gap=gap)
        m.set_locations(1, wide[1], gap=gap)
        got = m.match(H=c.H, F=c.F, **kw)
        assert len(ref) > 0 and np.array_equal(got, ref), (gap, mc.first_difference(ref, got))
    m.close()
    # max_sift below both sizes: descriptors AND locations are the first max_sift of what was passed (SiftMatchCU.cpp:76, 108)
    small = Matcher(0, max_sift=200)
    _load(small, c)
    cut = oracle_match(c.d1[:200], c.d2[:200], c.loc1[:200], c.loc2[:200], c.H, c.F, **kw)
    got = small.match(H=c.H, F=c.F, **kw)
    assert len(cut) > 0 and not np.array_equal(cut, ref[ref[:, 0] < 200])
    assert np.array_equal(got, cut), mc.first_difference(cut, got)
    small.close()


def test_guided_and_unguided_calls_on_one_handle():
    """2049 x 2081 is above 3 Mi products: the unguided call runs on the matrix cores and allocates no score matrix, the guided
    one stays on match_dot_kernel and needs one of 4 Mi entries.  Then the states a handle can be in."""
    from hessgpu_amd import _abi
    from hessgpu_amd.matcher import Matcher
    from hessgpu_amd.session import HessError

    cs = (2049, 2081, "affine")
    c = gc.case(*cs)
    th = gc.pick_thresholds(*cs)
    m = Matcher(0, max_sift=2081)
    _load(m, c)
    plain = dict(distmax=2.0, ratiomax=2.0, mutual_best=True, max_match=c.n1)
    plain_ref = oracle_match(c.d1, c.d2, **plain)
    # other matrices with the same exact decisions: H / 2 and 2 F are powers of two away
    H2, F2 = c.H * np.float32(0.5), c.F * np.float32(2.0)
    steps = [(None, None, None), (c.H, c.F, th[0]), (None, None, None), (H2, F2, th[3]), (c.H, c.F, th[1])]
    for H, F, t in steps:
        if H is None:
            ref, got = plain_ref, m.match(**plain)
        else:
            kw = _kw(t[0], t[1], 2.0, 2.0, True, c.n1)
            ref, got = _oracle(c, H, F, **kw), m.match(H=H, F=F, **kw)
            assert not np.array_equal(ref, plain_ref)
        assert len(ref) > 0 and np.array_equal(got, ref), (t, mc.first_difference(ref, got))
    # H without F is an argument error, before and after the locations are gone
    for H, F in ((c.H, None), (None, c.F)):
        with pytest.raises(HessError) as e:
            m.match(H=H, F=F)
        assert e.value.code == _abi.HESS_ERR_ARG
    # set_descriptors resets the locations of its slot: a guided call then returns no match (SiftMatchCU.cpp:76, 131)
    m.set_descriptors(1, c.d2)
    assert len(m.match(H=c.H, F=c.F, **_kw(th[0][0], th[0][1], 2.0, 2.0, True, c.n1))) == 0
    assert np.array_equal(m.match(**plain), plain_ref)
    m.set_locations(1, c.loc2)
    kw = _kw(th[0][0], th[0][1], 2.0, 2.0, False, c.n1)
    assert np.array_equal(m.match(H=c.H, F=c.F, **kw), _oracle(c, c.H, c.F, **kw))
    m.close()


def test_guided_match_is_the_same_every_time():
    """The block rule goes through an LDS atomic count per (8-row block, column); only `> 0` is read.  50 runs, mutual and not."""
    from hessgpu_amd.matcher import Matcher

    for cs in ((300, 333, "affine"), (300, 333, "projective")):
        c = gc.case(*cs)
        h, f = gc.pick_thresholds(*cs)[0]
        m = Matcher(0, max_sift=333)
        _load(m, c)
        for mutual in (True, False):
            kw = _kw(h, f, 2.0, 2.0, mutual, c.n1)
            first = m.match(H=c.H, F=c.F, **kw)
            ref = _oracle(c, c.H, c.F, **kw)
            assert len(ref) > 0 and np.array_equal(first, ref), (cs, mutual, mc.first_difference(ref, first))
            for k in range(50):
                assert np.array_equal(m.match(H=c.H, F=c.F, **kw), first), (cs, mutual, k)
        m.close()


def test_siftmatchgpu_guided_through_the_c_mirror():
    """SiftMatchGPU::SetFeautreLocation / GetGuidedSiftMatch: a missing matrix is the identity with a bound of 1e20, no matrix
    at all is the plain match (SiftMatch.cpp:663-676), both matrices are hess_matcher_match."""
    import siftgpu_lib
    from hessgpu_amd.matcher import Matcher

    L = siftgpu_lib.lib()
    f32, vp, i32 = C.c_float, C.c_void_p, C.c_int
    for name, res, args in [("siftmatch_create", vp, [i32]), ("siftmatch_destroy", None, [vp]),
                            ("siftmatch_set_descriptors_f32", None, [vp, i32, i32, vp]),
                            ("siftmatch_set_locations", None, [vp, i32, vp, i32]),
                            ("siftmatch_get_match", i32, [vp, i32, vp, f32, f32, i32]),
                            ("siftmatch_get_guided_match", i32, [vp, i32, vp, vp, vp, f32, f32, f32, f32, i32])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    eye = np.eye(3, dtype=np.float32)
    for cs in ((300, 333, "projective"), (300, 333, "affine")):
        c = gc.case(*cs)
        th = gc.pick_thresholds(*cs)
        fl = [(d.astype(np.float32) / np.float32(512.0)) for d in (c.d1, c.d2)]     # quantises back to the bytes
        hnd = L.siftmatch_create(512)
        for k in (0, 1):
            L.siftmatch_set_descriptors_f32(hnd, k, len(fl[k]), fl[k].ctypes.data)
        wide = [np.ascontiguousarray(np.concatenate([l, np.full((len(l), 2), 7.0, np.float32)], 1)) for l in (c.loc1, c.loc2)]
        L.siftmatch_set_locations(hnd, 0, wide[0].ctypes.data, 2)                   # gap 2: SetFeatureLocation(keys)
        L.siftmatch_set_locations(hnd, 1, c.loc2.ctypes.data, 0)
        buf = np.zeros((c.n1, 2), np.int32)

        def guided(H, F, h, f, mutual):
            n = L.siftmatch_get_guided_match(hnd, c.n1, buf.ctypes.data, None if H is None else H.ctypes.data,
                                             None if F is None else F.ctypes.data, 2.0, 2.0, h, f, int(mutual))
            return buf[:n].copy()

        m = Matcher(0, max_sift=512)
        _load(m, c)
        for mutual in (True, False):
            h, f = th[0]
            both = _oracle(c, c.H, c.F, **_kw(h, f, 2.0, 2.0, mutual, c.n1))
            got = guided(c.H, c.F, h, f, mutual)
            assert len(both) > 0 and np.array_equal(got, both), (cs, mutual, mc.first_difference(both, got))
            assert np.array_equal(got, m.match(H=c.H, F=c.F, **_kw(h, f, 2.0, 2.0, mutual, c.n1)))
            # H alone: the F bound passed is ignored (th[2] is the case's H-only pair)
            h_only = _oracle(c, c.H, eye, **_kw(th[2][0], gc.OFF, 2.0, 2.0, mutual, c.n1))
            got = guided(c.H, None, th[2][0], 1.0e-3, mutual)
            assert len(h_only) > 0 and np.array_equal(got, h_only), (cs, mutual, mc.first_difference(h_only, got))
            # F alone: the H bound passed is ignored (th[1] is the F-only pair)
            f_only = _oracle(c, eye, c.F, **_kw(gc.OFF, th[1][1], 2.0, 2.0, mutual, c.n1))
            got = guided(None, c.F, 1.0e-3, th[1][1], mutual)
            assert len(f_only) > 0 and np.array_equal(got, f_only), (cs, mutual, mc.first_difference(f_only, got))
            # neither: the plain match
            plain = oracle_match(c.d1, c.d2, distmax=2.0, ratiomax=2.0, mutual_best=mutual, max_match=c.n1)
            got = guided(None, None, 1.0e-3, 1.0e-3, mutual)
            assert np.array_equal(got, plain), (cs, mutual, mc.first_difference(plain, got))
            n = L.siftmatch_get_match(hnd, c.n1, buf.ctypes.data, 2.0, 2.0, int(mutual))
            assert np.array_equal(buf[:n], plain)
            assert len({both.tobytes(), h_only.tobytes(), f_only.tobytes(), plain.tobytes()}) == 4
        m.close()
        L.siftmatch_destroy(hnd)
