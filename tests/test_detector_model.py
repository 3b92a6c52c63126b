"""The CPU oracle against the independent float64 model of the detector (tests/np_restatement.py, DetectorModel), on
every case of tests/detector_cases.py: every option the product offers, not only the defaults on one photograph.

The same checker runs on the HIP path in tests/test_detector_model_gpu.py.  Here it also has to show its teeth: every
wrong-rule switch of the model must make it fail on a named case.

Wrong rule -> case that catches it (stage):
  top-K ties go to the higher index            top-K (detect)
  top-K keyed on the float response            top-K (detect)
  second truncation pass omitted               truncate highest0, truncate highest1 (orient)
  up-sample row end clamps                     first_octave -1, first_octave -2 (gauss)
  first blur not skipped                       first_octave -2 (gauss)
  33-tap clamp omitted                         dog_level_num 1 (gauss)
  subpixel=0 keeps the 0.8 factor              subpixel 0 (detect)
  16-bit RGB does not wrap                     u16 rgb (gauss)
  level binning rounds at whole steps          keypoint list orient=1 (descriptor), keypoint list max_orientation 1 (level)
  lowe_origin offset before the octave scale   lowe_origin (export)
Two switches are NOT caught by any case (test_switches_the_checker_does_not_see), for different reasons:
  half fold refreshes the 37th slot   UNOBSERVABLE.  Slot 36 is read only as the right neighbour of bin 35, and after the
                                      fold bin 35 holds 0, which is neither above a threshold >= 0 nor a strict maximum.
  single peak takes the last maximum  UNPINNED.  '>=' differs from '>' only on an exact tie of the largest vote.  Such ties
                                      can occur -- a point-symmetric patch gives bins b and b + 18 equal votes, and the
                                      smoothing is shift-invariant -- but the checker cannot use them: orientations_ex
                                      flags any two votes within the rounding margin as uncertain, an exact tie
                                      included, and at a flagged item either answer passes.  Whether the float32 sums of
                                      an implementation tie exactly where the float64 ones do depends on its order of
                                      summation, which the model does not state.  So a kernel that takes the last
                                      maximum passes this file; only the bit parity with the oracle holds that rule.
Uncertain share (flagged detections + flagged orientation decisions, of the candidates that pass the exact neighbour
comparisons): 2 of 241 on 'noise 324x223', 0 on every other case; 0 flagged orientations on every keypoint-list case.
"""
from contextlib import closing

import numpy as np
import pytest

import detector_cases as dc
import np_restatement as R
from oracle_lib import OracleSession

CASES = list(dc.cases())

CATCHES = {
    "top-K ties go to the higher index": ("top-K", "detect"),
    "top-K keyed on the float response": ("top-K", "detect"),
    "second truncation pass omitted": ("truncate highest0", "orient"),
    "up-sample row end clamps": ("first_octave -1", "gauss"),
    "first blur not skipped": ("first_octave -2", "gauss"),
    "33-tap clamp omitted": ("dog_level_num 1", "gauss"),
    "subpixel=0 keeps the 0.8 factor": ("subpixel 0", "detect"),
    "16-bit RGB does not wrap": ("u16 rgb", "gauss"),
    "level binning rounds at whole steps": ("keypoint list max_orientation 1", "keylist"),
    "lowe_origin offset before the octave scale": ("lowe_origin", "export"),
}
UNOBSERVABLE = {        # not caught: the first is unobservable, the second unpinned (module docstring)
    "half fold refreshes the 37th slot": ("half_sift", "half_sift max_orientation 1", "keypoint list half_sift"),
    "single peak takes the last maximum": ("max_orientation 1", "keypoint list max_orientation 1", "keypoint list orient=0"),
}


def _oracle(case):
    return OracleSession(threads=4, **case.kw)


@pytest.mark.parametrize("name", CASES)
def test_oracle_follows_the_model(name):
    case = dc.cases()[name]
    with closing(_oracle(case)) as o:
        st = dc.check_against_model(o, case)
    print(name, st)
    dc.check_statistics(st, case)


@pytest.mark.parametrize("rule", list(CATCHES))
def test_every_wrong_rule_is_caught(rule):
    name, stage = CATCHES[rule]
    case = dc.cases()[name]
    with closing(_oracle(case)) as o, pytest.raises(dc.Mismatch) as e:
        dc.check_against_model(o, case, model=R.DetectorModel(o.params, **R.WRONG_RULES[rule]))
    print(rule, "->", name, ":", e.value)
    assert e.value.stage == stage


@pytest.mark.parametrize("rule", list(UNOBSERVABLE))
def test_switches_the_checker_does_not_see(rule):
    """See the module docstring: one has no observable effect, the other hides behind the uncertain margin.  Should one
    of these ever be caught, the reasoning there is wrong: move the switch to CATCHES."""
    for name in UNOBSERVABLE[rule]:
        case = dc.cases()[name]
        with closing(_oracle(case)) as o:
            dc.check_against_model(o, case, model=R.DetectorModel(o.params, **R.WRONG_RULES[rule]), dense=False)


def test_every_switch_is_accounted_for():
    assert set(CATCHES) | set(UNOBSERVABLE) == set(R.WRONG_RULES) and not set(CATCHES) & set(UNOBSERVABLE)


def test_grid_thresholds_fall_inside_a_level():
    """The truncation thresholds cut inside a level and the second pass changes the result; the top-K cut separates
    detections of equal half-precision response."""
    g = dc.dot_grid()
    with closing(OracleSession(threads=4, **dc.GRID_KW)) as o:
        assert o.run(g[None]) == [805]
        raw = o.rawlist(0)
        keys, _ = o.fetch(0)
    det = np.bincount(raw["level_index"], minlength=8).tolist()
    feat = np.bincount(keys["level"], minlength=8).tolist()
    assert det == [345, 219, 34, 1, 50, 10, 2, 7] and feat == [381, 282, 43, 1, 59, 14, 3, 22]
    t = dc.GRID_THRESHOLD
    assert sum(det[2:]) < t < sum(det[1:])                 # the first pass stops inside level 1 and keeps it ...
    assert sum(feat[1:]) - feat[1] > t                     # ... the second, on the features, drops it
    assert det[0] < dc.GRID_THRESHOLD_LOWEST < det[0] + det[1]
    half = np.sort(np.abs((raw["packed"] >> 16).astype(np.uint16).view(np.float16).astype(np.float32)))[::-1]
    assert half[dc.GRID_TOPK - 1] == half[dc.GRID_TOPK]


def test_the_16_bit_case_wraps_and_the_clamps_are_reached():
    c = dc.cases()["u16 rgb"].image.astype(np.int64)
    num = 19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2]
    assert (num >= 1 << 31).mean() > 0.2 and (num < 1 << 31).mean() > 0.2
    m = R.DetectorModel(dict(dog_level_num=1))
    assert 2 * int(np.ceil(4.0 * m.inter[1] - 0.5)) + 1 == 45 and len(m.level_taps(2)) == 33
    m = R.DetectorModel(dict(sigman=1.56))
    assert 2 * int(np.ceil(4.0 * m.initial_sigma(0) - 0.5)) + 1 == 3 and len(m.level_taps(0)) == 5
    assert R.DetectorModel(dict(first_octave=-2)).level_taps(0, -2) is None
    assert R.DetectorModel(dict(first_octave=-5, auto_downscale=1, tex_max_dim=200)).plan(96, 80)[1] == -1
