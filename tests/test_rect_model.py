"""The float64 model of the rectangle descriptors (tests/rect_cases.py) on planes with closed-form answers, and the
checker's teeth: through ModelSession, check_rectangles passes for the right rule and raises for each wrong one -- among
them the oriented descriptor at (x, y, s, o), which is what a caller of flag -1 got before the mode existed.  No GPU."""
import math

import numpy as np
import pytest

import detector_cases as dc
import np_restatement as R
import rect_cases as rc
from hessgpu_amd import _abi


def _plane(h=48, w=64, g0=0.25, theta0=0.0):
    return np.full((h, w), g0), np.full((h, w), theta0, dtype=np.float32).astype(np.float64)


def _axis_sum(c0, spt, n):
    """sum of 1 - |nx| over the pixel centres of one cell's box along one axis, written out sample by sample"""
    total = 0.0
    lo, hi = max(1.5, math.floor(c0 - spt) + 0.5), min(n - 1.5, math.floor(c0 + spt) + 0.5)
    v = lo
    while v <= hi:
        if abs((v - c0) / spt) < 1:
            total += 1 - abs((v - c0) / spt)
        v += 1.0
    return total


def test_constant_plane_two_bins_and_separable_cells():
    # theta = -0.3 pi: bin coordinate 1.2 -> bins 1 and 2 in the ratio 0.8 : 0.2, nothing elsewhere
    g0, X, Y, W, H = 0.25, 10.25, 7.5, 22.0, 13.0
    grad, theta = _plane(g0=g0, theta0=-0.3 * R.PI)
    d = rc.rect_descriptor_ex(grad, theta, X, Y, W, H, normalize=False).reshape(16, 8)
    assert np.all(d[:, [0, 3, 4, 5, 6, 7]] == 0)
    t = float(np.float32(-0.3 * R.PI)) * -4.0 / R.PI
    assert np.allclose(d[:, 1] / d[:, 2], (2 - t) / (t - 1), rtol=1e-12)
    # a rectangle well inside: every cell is g0 * sum(wx) * sum(wy)
    for cell in range(16):
        ix, iy = cell & 3, cell >> 2
        sx = _axis_sum(X + W / 4 * (ix + 0.5), W / 4, grad.shape[1])
        sy = _axis_sum(Y + H / 4 * (iy + 0.5), H / 4, grad.shape[0])
        assert d[cell].sum() == pytest.approx(g0 * sx * sy, rel=1e-12)
    # normalised: unit length, nothing above 0.2 before the second pass
    n = rc.rect_descriptor_ex(grad, theta, X, Y, W, H)
    assert np.sqrt((n * n).sum()) == pytest.approx(1.0, abs=1e-12)


def test_clipping_at_the_border():
    grad, theta = _plane(theta0=-0.3 * R.PI)
    h, w = grad.shape
    d = rc.rect_descriptor_ex(grad, theta, 0.25, 0.5, 20.0, 16.0, normalize=False).reshape(16, 8)
    sx = _axis_sum(0.25 + 5.0 * 0.5, 5.0, w)        # cell column 0: pixel centre 0.5 is outside [1.5, w - 1.5]
    sy = _axis_sum(0.5 + 4.0 * 0.5, 4.0, h)
    assert d[0].sum() == pytest.approx(0.25 * sx * sy, rel=1e-12)
    assert sx < _axis_sum(20.25 + 2.5, 5.0, w)


@pytest.mark.parametrize("half", [False, True])
def test_empty_window(half):
    grad, theta = _plane()
    dim = 64 if half else 128
    for X, Y, W, H in ((10.0, 10.0, 0.0, 12.0), (10.0, 10.0, 12.0, 0.0), (16377.2, 10.0, 12.0, 12.0), (200.0, 100.0, 9.0, 9.0)):
        d = rc.rect_descriptor_ex(grad, theta, X, Y, W, H, half=half)
        assert d.shape == (dim,) and np.all(d == 1.0 / math.sqrt(dim)), (X, Y, W, H)
        z = rc.rect_descriptor_ex(grad, theta, X, Y, W, H, half=half, normalize=False)
        assert z.shape == (dim,) and np.all(z == 0)


def test_half_folding():
    grad, theta = _plane(theta0=0.7 * R.PI)          # -theta 4/pi = -2.8 -> 5.2: bins 5 and 6, folded into 1 and 2
    full = rc.rect_descriptor_ex(grad, theta, 9.0, 8.0, 20.0, 20.0, normalize=False).reshape(16, 8)
    half = rc.rect_descriptor_ex(grad, theta, 9.0, 8.0, 20.0, 20.0, half=True, normalize=False).reshape(16, 4)
    assert np.all(full[:, :5] == 0) and np.all(full[:, 5] > 0) and np.all(full[:, 6] > 0)
    assert np.array_equal(half, full[:, :4] + full[:, 4:])
    assert np.all(half[:, 1] == full[:, 5]) and np.all(half[:, 2] == full[:, 6])


def test_bin_coordinate_eight_and_zero():
    # theta = +1e-9: -theta 4/pi + 8 is 8.0 as a binary32 number -> dropped, or bin 8 = bin 0 with dynamic_indexing
    grad, theta = _plane(theta0=1e-9)
    dropped = rc.rect_descriptor_ex(grad, theta, 9.0, 8.0, 20.0, 20.0, normalize=False)
    assert np.all(dropped == 0)
    di = rc.rect_descriptor_ex(grad, theta, 9.0, 8.0, 20.0, 20.0, dynamic_indexing=True, normalize=False).reshape(16, 8)
    assert np.all(di[:, 0] > 0) and np.all(di[:, 1:] == 0)
    # theta = +0: the bin coordinate is (minus) zero, all of the weight in bin 0 in both modes
    grad, theta = _plane(theta0=0.0)
    for flag in (False, True):
        z = rc.rect_descriptor_ex(grad, theta, 9.0, 8.0, 20.0, 20.0, dynamic_indexing=flag, normalize=False).reshape(16, 8)
        assert np.all(z[:, 0] > 0) and np.all(z[:, 1:] == 0)
        assert np.array_equal(z, di)


def test_record_rules():
    m = R.DetectorModel({})
    k = rc.rect_keys([[10.0, 20.0, 300.0, 7.3]])[0]
    X, Y, W, H = rc.rect_record(m, k, 1.0)
    assert (X, Y) == (10.0, 20.0) and W == 300.0 - 256.0            # the width wraps at 256 level pixels
    assert H == float(np.float32(7.3))                              # the height is not quantised
    X, _, _, _ = rc.rect_record(m, rc.rect_keys([[-7.0, 20.0, 30.0, 30.0]])[0], 1.0)
    assert X > 16000                                                # a negative corner wraps
    assert rc.rect_sigma(k) == float(np.float32(7.3) / np.float32(12))
    assert _abi.KEYS_RECTANGLES == -1 and (_abi.KEYS_NONE, _abi.KEYS_ORIENTED) == (0, 1)


def test_cases_hold_what_they_promise():
    for kw in ({}, dict(first_octave=-1), dict(detector=_abi.DETECTOR_DOG)):
        m = R.DetectorModel(kw)
        for case in rc.cases(kw):
            h, w = case.image.shape[:2]
            _, _, geo, scales = m.plan(w, h)
            keys = case.keys
            levels = [m.bin_key(rc.rect_sigma(k), scales) for k in keys]
            assert all(len(hit) == 1 for hit in levels)
            if len(keys) < 65:
                continue
            assert {hit[0] for hit in levels} == set(range(len(scales) * m.dog)), "a square in every level's bin"
            rec = [rc.rect_record(m, k, scales[hit[0] // m.dog]) for k, hit in zip(keys, levels)]
            box = [1.25 * W for X, Y, W, H in rec if X < 16000]
            assert any(64 < b <= 128 for b in box)
            if w >= 160:
                assert any(b > 128 for b in box), "a box across two band seams"
            assert any(W == 0 for _, _, W, _ in rec) and any(H == 0 for _, _, _, H in rec)
            assert any(H >= 256 for _, _, _, H in rec), "a height the 8.8 fixed point would wrap"
            assert any(float(k["s"]) / scales[hit[0] // m.dog] >= 256 for k, hit in zip(keys, levels)), "a width that wraps"
            assert any(X > 16000 for X, _, _, _ in rec), "a negative corner"
            asp = [float(k["s"]) / float(k["o"]) for k in keys if k["o"] > 0]
            assert max(asp) >= 5 and min(asp) <= 0.2


@pytest.fixture(scope="module")
def blobs_case():
    return rc.cases()[2]        # 65 rectangles on blobs_noise


def test_checker_passes_for_the_right_rule(blobs_case):
    for entry in ("run_keypoints", "set_keypoints"):
        st = rc.check_rectangles(rc.ModelSession(), blobs_case, entry)
        assert st["rectangles"] == 65 and st["worst"] < 1e-6, st
        assert st["empty"] == 4, st      # wholly outside, negative corner, narrower than 1/512, height 0
    st = rc.check_rectangles(rc.ModelSession(half_sift=1, normalize=0, dynamic_indexing=1), blobs_case)
    assert st["worst"] < 1e-6, st


@pytest.mark.parametrize("rule", list(rc.WRONG_RULES))
def test_checker_raises_for_a_wrong_rule(blobs_case, rule):
    with pytest.raises(dc.Mismatch):
        rc.check_rectangles(rc.ModelSession(wrong=rc.WRONG_RULES[rule]), blobs_case)
