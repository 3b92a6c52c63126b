"""What tests/test_verify_pairs_gpu.py relies on in the banks of tests/verify_cases.py, asserted without a GPU from
matcher_cases.Model (the unguided match as a rule) and geom_cases.decide64 (the gate in float64) only: every bank pair's
putative list is a subset of its case's matches with at least 95 % of them, mutual or not; the planted model has at least k
inliers among them, except in the below-k cases, which stay below k."""
import numpy as np
import pytest

import geom_cases as gcs
import matcher_cases as mc
import matcher_cases_half as mh
import verify_cases as vc


@pytest.fixture(scope="module")
def putative():
    """name -> the model's unguided match of the case's two sets, mutual best and not."""
    out = {}
    for name in vc.BANK_CASES:
        d1, d2, _, _ = vc.pair_sets(name)
        M = mc.Model(d1, d2)
        out[name] = tuple(M.match(distmax=vc.DISTMAX, ratiomax=vc.RATIOMAX, mutual=mutual, max_match=1 << 20) for mutual in (True, False))
    return out


@pytest.mark.parametrize("name", vc.BANK_CASES)
def test_putative_matches_are_the_cases_matches(putative, name):
    c, want = gcs.case(name), vc.case_set(name)
    for got in putative[name]:
        have = set(map(tuple, got.tolist()))
        assert have <= want, (name, sorted(have - want)[:5])
        assert len(have) >= vc.MIN_SHARE * c.n, (name, len(have), c.n)


@pytest.mark.parametrize("name", vc.BANK_CASES)
def test_planted_model_is_there_to_find_or_the_pair_stays_below_k(putative, name):
    c = gcs.case(name)
    k = gcs.K[c.model]
    for got in putative[name]:
        if name in vc.BELOW:
            assert len(got) < k, (name, len(got))
            continue
        assert len(got) >= k
        ok, band = gcs.decide64(c.model, c.truth, c.loc1[got[:, 0]], c.loc2[got[:, 1]], c.bound)
        assert int((ok & ~band).sum()) >= k, (name, int(ok.sum()), int(band.sum()))


def test_folded_sets_keep_the_planted_matches():
    """The 64-d bank of the GPU test: the same subsets, at least 95 % of the matches, on the folded rows."""
    for name in ("H 65", "H 300", "F 300"):
        d1, d2, _, _ = vc.pair_sets(name)
        got = mc.Model(mh.fold(d1), mh.fold(d2)).match(distmax=vc.DISTMAX, ratiomax=vc.RATIOMAX, mutual=True, max_match=1 << 20)
        have = set(map(tuple, got.tolist()))
        assert have <= vc.case_set(name) and len(have) >= vc.MIN_SHARE * gcs.case(name).n, (name, len(have))


def test_lists_and_bank_are_what_the_gpu_test_describes():
    sets, locs = vc.bank()
    assert len(sets) == len(locs) == vc.EMPTY_SET + 1 and len(sets[vc.EMPTY_SET]) == 0
    assert all(len(s) == len(l) for s, l in zip(sets, locs))
    pairs, names = vc.bank_pairs()
    assert len(pairs) == len(names) and pairs.max() == vc.EMPTY_SET and any(a == b for a, b in pairs)
    many = vc.many_pairs(300)
    assert len(many) == 300 > 256                                   # crosses the matcher's 64 and the estimator's 256 pairs
    seen = {}
    for p, ab in enumerate(map(tuple, many.tolist())):
        seen.setdefault(ab, []).append(p)
    assert all(len(v) >= 2 for v in seen.values())                  # every (a, b) recurs: seed + p must be the list position
    assert any(v[0] // 64 == v[1] // 64 for v in seen.values())     # ... within a chunk of 64 and
    assert any(v[0] // 64 != v[-1] // 64 and v[0] % 64 != v[-1] % 64 for v in seen.values())   # across chunks at other offsets
    assert any((b, a) in seen for a, b in seen)                     # reversals
    assert len(vc.big()[0][0]) > 4096 and len(vc.big()[0][0]) <= vc.BIG_MAX_SIFT
