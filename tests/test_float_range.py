"""Float pixels of any range on the CPU: the oracle against the float64 model (np_restatement.DetectorModel) on every case
of tests/float_range_cases.py -- luminance in 0 .. 2^8, 2^10, 2^16, 2^-8 .. 2^-20, 0 .. 255, 0 .. 65535, zero-mean and negated,
as luminance, RGB and BGR, with the options that meet the value range, keypoint lists and a batch -- then the exact
homogeneity of the oracle in the amplitude, the lists whose top-K keys are all equal, and the wrong rules.
tests/test_float_range_gpu.py runs the same on the HIP path.

Conditions on every case: 0 flagged candidates and 0 flagged orientations (a flagged item passes with either answer), at least
50 candidates and 8 detections in every pixel case.  On the oracle the cases have 54 to 141 candidates and 39 to 119
detections; the largest deviations are those of the [0, 1] images, relative to the amplitude: Gaussian 3.3e-7, det-H 3.5e-7,
gradient 3.3e-8, theta 2.7e-7, descriptor 7.3e-7 (6.1e-7 of the amplitude with normalize = 0).

Wrong rule -> case that catches it (stage): float_range_cases.CATCHES.
"""
from contextlib import closing

import numpy as np
import pytest

import detector_cases as dc
import float_range_cases as fc
import list_cases as L
import np_restatement as R
from oracle_lib import OracleSession

CASES = list(fc.cases())
PAIRS = fc.pairs()
LISTS = fc.list_cases()


def _oracle(case):
    return OracleSession(threads=4, **case.kw)


@pytest.mark.parametrize("name", CASES)
def test_oracle_follows_the_model(name):
    case = fc.cases()[name]
    with closing(_oracle(case)) as o:
        st = dc.check_against_model(o, case)
    print(name, st)
    fc.check_statistics(st, case)


@pytest.mark.parametrize("name", list(PAIRS))
def test_oracle_is_homogeneous(name):
    """Planes, lists, keypoints and descriptors of A b from those of b, bit for bit (float_range_cases.check_homogeneous)."""
    ca, cb, k, lists = PAIRS[name]
    with closing(_oracle(ca)) as oa, closing(_oracle(cb)) as ob:
        a, b = fc.snapshot(oa, ca), fc.snapshot(ob, cb)
    fc.check_homogeneous(a, b, k, lists, fc.half_regime(ca), fc.half_regime(cb))


def test_beyond_the_pivot_guard_nothing_is_solved():
    """At 2^-14 every offset is 0 and there are more detections than the solved branch gives; at 2^-11 most candidates are
    solved, with the offsets of the unit image, and the few whose pivot fell below 1e-10 have none."""
    raws = {}
    for e in (0, -11, -14):
        case = fc.cases()["float: blobs 1" if e == 0 else f"float: blobs 2^{e}"]
        with closing(_oracle(case)) as o:
            o.run(case.image[None])
            raws[e] = o.rawlist(0)
    off = lambda r: np.stack([r["dx"], r["dy"], r["ds"]], axis=1)
    pos = lambda r: [tuple(v) for v in np.stack([r["level_index"], r["row"], r["col"]], axis=1).tolist()]
    assert (len(raws[0]), len(raws[-11]), len(raws[-14])) == (64, 65, 73)
    assert off(raws[0]).any(axis=1).all() and not off(raws[-14]).any()
    assert set(pos(raws[0])) <= set(pos(raws[-14]))
    unit = dict(zip(pos(raws[0]), off(raws[0]).tolist()))
    solved = [p for p, o in zip(pos(raws[-11]), off(raws[-11]).tolist()) if any(o)]
    assert len(solved) >= 50 and all(unit.get(p) == o for p, o in zip(pos(raws[-11]), off(raws[-11]).tolist()) if any(o))
    assert not L.topk_key(raws[-11]).any() and not L.topk_key(raws[-14]).any()


def test_the_negative_image_mirrors_the_types():
    """det-H is even in the sign of the plane: the same list, the same responses; dark and bright change places."""
    res = {}
    for name in ("float: blobs 1", "float: blobs negated"):
        case = fc.cases()[name]
        with closing(_oracle(case)) as o:
            o.run(case.image[None])
            res[name] = (o.rawlist(0), o.fetch(0)[0])
    (ra, ka), (rb, kb) = res.values()
    for f in ("level_index", "row", "col", "dx", "dy", "ds"):
        assert ra[f].tobytes() == rb[f].tobytes(), f
    assert np.array_equal(ra["packed"] >> 16, rb["packed"] >> 16)
    swap = np.array([1, 0, 2])
    assert np.array_equal(swap[ra["packed"] & 3], rb["packed"] & 3) and len(set((ra["packed"] & 3).tolist())) == 3
    # the same number of orientations per location, each turned by pi within a quantum of the 8-bit angle
    assert len(ka) == len(kb) and ka["x"].tobytes() == kb["x"].tobytes() and ka["s"].tobytes() == kb["s"].tobytes()
    turned = np.abs(np.angle(np.exp(1j * (ka["o"].astype(np.float64) - kb["o"] - R.PI))))
    assert turned.max() <= dc.QUANTUM + dc.TOL_ANGLE, float(turned.max())


def test_the_batch_has_its_own_counts_per_image():
    stack = fc.batch_stack()
    with closing(OracleSession(threads=4, keep_levels=False, dog_threshold=fc.BATCH_THRESHOLD)) as o:
        assert o.run(stack) == fc.BATCH_FEATURES
        assert np.isinf(o.fetch(1)[0]["response"]).all()


# ---- the wrong rules ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", list(fc.CATCHES))
def test_every_wrong_rule_is_caught(rule):
    name, stage = fc.CATCHES[rule]
    case = fc.cases()[name]
    with closing(_oracle(case)) as o, pytest.raises(dc.Mismatch) as e:
        dc.check_against_model(o, case, model=R.DetectorModel(o.params, **R.WRONG_RULES[rule]))
    print(rule, "->", name, ":", e.value)
    assert e.value.stage == stage


# ---- lists whose keys are all equal ------------------------------------------------------------------------------------------

def oracle_runner(case):
    imgs = case.image()

    def run(kw):
        with closing(OracleSession(threads=4, keep_levels=False, **kw)) as o:
            counts = o.run(imgs)
            return L.result_of(o, counts, case.index)

    return run


@pytest.mark.parametrize("name", list(LISTS))
def test_oracle_follows_the_list_model(name):
    case = LISTS[name]
    st = L.check_case(oracle_runner(case), case)
    fc.check_list_reach(st, case, oracle_runner(case))
