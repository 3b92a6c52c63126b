"""One matcher through every entry point that takes the plan buffer, the output buffer, the pinned slots or the locations, in
an order in which each call finds what another kind of call left behind: every result equals, byte for byte, that of the same
call on a fresh matcher that has made no other call.  Then the rules by which locations end: a slot's with new descriptors for
that slot, the bank's with a new bank."""
import numpy as np
import pytest

import geom_cases as gcs
import matcher_cases as mc
import verify_cases as vc

pytestmark = pytest.mark.gpu

T, SEED = 300, 11
BIG, TYPED = 1800, 300          # 1800 x 1800 > MATRIX_CORE_ABOVE: the untyped single pair through the plan buffer


def _hm():
    from hessgpu_amd import matcher as hm
    return hm


def _fresh():
    m = _hm().Matcher(0)
    m.set_bank(vc.bank()[0])
    m.set_bank_locations(vc.bank()[1])
    return m


def _params():
    return _hm().Matcher._verify_params("H", gcs.BOUND["H"], T, SEED, 1, None, True, vc.DISTMAX, vc.RATIOMAX, True)


def _verify(m, n):
    return b"".join(a.tobytes() for a in m.verify_pairs_raw(vc.many_pairs(n), _params(), 70, inlier=True, putative=True))


def _big_pair(m):
    rng = np.random.RandomState(23)
    d1 = mc.descriptor_rows(BIG, rng)
    d2 = mc.descriptor_rows(BIG, rng)
    d2[::3] = mc.noisy(d1, rng)[::3]
    m.set_descriptors(0, d1)
    m.set_descriptors(1, d2)
    return m.match(BIG)


def _typed_pair(m):
    rng = np.random.RandomState(24)
    d1 = mc.descriptor_rows(TYPED, rng)
    d2 = mc.noisy(d1, rng)
    m.set_descriptors(0, d1)
    m.set_descriptors(1, d2)
    m.set_types(0, rng.randint(0, 4, TYPED).astype(np.uint16))
    m.set_types(1, rng.randint(0, 4, TYPED).astype(np.uint16))
    return m.match(TYPED)


def _guided_list(m):
    pairs = vc.many_pairs(130)
    return m.match_pairs_guided(pairs, H=np.tile(gcs.H_TRUE, (len(pairs), 1, 1)), hdistmax=gcs.BOUND["H"], max_match=70)


def _estimate_list(m, matches):
    res = m.estimate_pairs(vc.many_pairs(130), matches, "H", gcs.BOUND["H"], hypotheses=T, seed=SEED, refit=1, info=True)
    return b"".join(M.tobytes() + mask.tobytes() + repr((hyp, sorted(info.items()))).encode() for M, mask, hyp, info in res)


def _guided_pair(m, locations=(0, 1)):
    d1, d2, l1, l2 = vc.pair_sets("H 65")
    m.set_descriptors(0, d1)
    m.set_descriptors(1, d2)
    for k in locations:
        m.set_locations(k, (l1, l2)[k])
    return m.match(len(d1), H=gcs.H_TRUE, F=np.eye(3), hdistmax=gcs.BOUND["H"], fdistmax=_hm().GUIDED_OFF)


def _lists(ms):
    return b"|".join(a.tobytes() for a in ms)


def _alone(call):
    m = _fresh()
    try:
        return call(m)
    finally:
        m.close()


def test_calls_on_one_matcher_equal_calls_on_fresh_matchers():
    hm = _hm()
    from hessgpu_amd import _abi
    m = _fresh()
    first = _verify(m, 70)                                          # 1: two chunks, one group
    assert first == _alone(lambda f: _verify(f, 70))
    big = _big_pair(m)                                              # 2: the plan buffer, by the single pair
    assert len(big) > 0 and big.tobytes() == _alone(_big_pair).tobytes()
    typed = _typed_pair(m)                                          # 3: run_pairs on the slots, a list of one
    assert 0 < len(typed) < TYPED and typed.tobytes() == _alone(_typed_pair).tobytes()
    guided = _guided_list(m)                                        # 4: three chunks with the geometry table
    assert sum(len(g) for g in guided) > 0 and _lists(guided) == _lists(_alone(_guided_list))
    assert _verify(m, 300) == _alone(lambda f: _verify(f, 300))     # 5: two groups, both pinned slots, larger buffers
    assert _estimate_list(m, guided) == _alone(lambda f: _estimate_list(f, guided))                         # 6
    pair = _guided_pair(m)                                          # 7: the slots' own locations
    assert len(pair) > 0 and pair.tobytes() == _alone(_guided_pair).tobytes()
    assert _verify(m, 70) == first                                  # 8
    # new descriptors for slot 0 end its locations: no guided match (SiftMatchGPU's rule), no estimate
    assert len(_guided_pair(m, locations=(1,))) == 0
    with pytest.raises(hm.HessError) as e:
        m.estimate(pair, "H", gcs.BOUND["H"], hypotheses=T, seed=SEED)
    assert e.value.code == _abi.HESS_ERR_STATE and "slot 0" in str(e.value)
    # a new bank ends the bank's locations
    m.set_bank(vc.bank()[0])
    with pytest.raises(hm.HessError) as e:
        _guided_list(m)
    assert e.value.code == _abi.HESS_ERR_STATE and "locations" in str(e.value)
    m.close()
