"""The bit-for-bit comparison of a product context with the CPU oracle that the GPU parity tests share (a plain helper
module, no tests in it): geometry, every Gaussian / det-H / gradient-theta plane, the raw detection list, keypoints and
descriptors.  The north star's tolerance for descriptors / keypoints is 1e-4; the helpers assert 0 first and report the
largest deviation if that ever fails."""
import numpy as np
import pytest

from hessgpu_amd import _abi

TOL = 1e-4  # BASELINE.json north_star: "keypoints/descriptors matching reference within 1e-4"


def assert_same_features(gk, gd, ok, od, what):
    assert len(gk) == len(ok), f"{what}: feature count {len(gk)} != oracle {len(ok)}"
    assert np.array_equal(gk["level"], ok["level"]) and np.array_equal(gk["type"], ok["type"]), f"{what}: level/type"
    for f in ("x", "y", "s", "o", "response"):
        if not np.array_equal(gk[f], ok[f]):
            d = np.max(np.abs(gk[f].astype(np.float64) - ok[f].astype(np.float64)))
            assert d <= TOL, f"{what}: keypoint field {f} max abs diff {d}"
            pytest.fail(f"{what}: keypoint field {f} within 1e-4 (max {d}) but not bit-exact")
    if od.size:
        if not np.array_equal(gd.view(np.uint32), od.view(np.uint32)):
            d = np.nanmax(np.abs(gd.astype(np.float64) - od.astype(np.float64)))
            bad = np.sum(np.any(gd.view(np.uint32) != od.view(np.uint32), axis=1))
            assert d <= TOL, f"{what}: descriptors max abs diff {d} ({bad} rows differ)"
            pytest.fail(f"{what}: descriptors within 1e-4 (max {d}, {bad} rows) but not bit-exact")


def compare_all(g, o, imgs, what, stages=True, product_imgs=None):
    """Run the product `g` and the oracle `o` and compare every stage bit for bit.  product_imgs: what the product is
    given instead of imgs -- the same pixels in another memory layout (tests/input_layouts.py)."""
    g.keep_levels(stages)   # the top Gaussian level of an octave is only written to HBM on request (hess_debug_keep_levels)
    ng = g.run(imgs if product_imgs is None else product_imgs)
    no = o.run(imgs)
    return compare_results(g, o, ng, no, what, stages)


def compare_results(g, o, ng, no, what, stages=True):
    """The comparison alone, after both sides have run (ng, no: their feature counts per image); stages needs
    g.keep_levels(True) before the product's run."""
    assert g.geometry() == o.geometry()
    if stages:
        # (the difference-of-Gaussians detector has one Gaussian level and one response plane more: D_l for l = 1 .. dog + 2)
        nlev = o.params.dog_level_num + 2 + (1 if o.params.detector == _abi.DETECTOR_DOG else 0)
        for b in range(len(no)):
            for oc in range(len(o.geometry())):
                for l in range(nlev):
                    a, r = g.level(b, oc, l, _abi.DBG_GAUSS), o.level(b, oc, l, _abi.DBG_GAUSS)
                    assert np.array_equal(a.view(np.uint32), r.view(np.uint32)), \
                        f"{what}: gauss img {b} oct {oc} lvl {l}: {np.sum(a != r)} px differ, max {np.max(np.abs(a - r))}"
                for l in range(nlev):
                    a, r = g.level(b, oc, l, _abi.DBG_DETH), o.level(b, oc, l, _abi.DBG_DETH)
                    assert np.array_equal(a.view(np.uint32), r.view(np.uint32)), \
                        f"{what}: det-H img {b} oct {oc} lvl {l}: {np.sum(a != r)} px differ, max {np.max(np.abs(a - r))}"
                for l in range(1, o.params.dog_level_num + 1):
                    a, r = g.level(b, oc, l, _abi.DBG_GOT), o.level(b, oc, l, _abi.DBG_GOT)
                    assert np.array_equal(a.view(np.uint32), r.view(np.uint32)), \
                        f"{what}: grad/theta img {b} oct {oc} lvl {l}: {np.sum(a != r)} values differ"
    for b in range(len(no)):
        gl, ol = g.rawlist(b), o.rawlist(b)
        assert len(gl) == len(ol), f"{what}: img {b} list length {len(gl)} != {len(ol)}"
        assert gl.tobytes() == ol.tobytes(), f"{what}: img {b} detection list differs"
    assert ng == no, f"{what}: feature counts {ng} != {no}"
    for b in range(len(no)):
        gk, gd = g.fetch(b)
        ok, od = o.fetch(b)
        assert_same_features(gk, gd, ok, od, f"{what} img {b}")
    return no
