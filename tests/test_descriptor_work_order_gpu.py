"""Work order of the descriptor launch: which wavefront takes which feature must not show in the results.

The three descriptor kernels share one feature order (first_feature in k_feature.hip: the list from its end backwards, in
blocks of HESS_DESC_XCD consecutive features per XCD) and one split of an image's features over several launches
(desc_image: part k of n, when one image is delivered by the copier thread).  For every descriptor_order and every block
size -- 0 is the plain order, 16 and 64 divide the grids used here -- the results are the oracle's: bitwise for the
sequential (1) and the pixel (2) order, within test_descriptor_order.TOL for the interleaved one (0), whose results must
also be the same bytes for all block sizes.  Delivery forms: one image (in-kernel host mirror), a batch of three (copier
thread), one image delivered by the copier thread's DMA copies (four launches over quarters of its features), and a 64 x 64
image with -topk 64: the feature storage, which bounds the grid whatever the image's size, then holds 256 features, the
grid is 64 workgroups -- below the 128 of one round of blocks -- and launch_descriptor turns the block order off itself."""
import numpy as np
import pytest

import fixtures
from hessgpu_amd import _abi
from oracle_lib import OracleSession
from test_descriptor_order import TOL

XCD_BLOCKS = ("0", "16", "64")
SMALL = dict(truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=64)


def _images():
    imgs = np.stack([fixtures.load_rgb(n)[..., 1] for n in ("640-3.jpg", "640-2.jpg", "640-1.jpg")])
    small = np.ascontiguousarray(imgs[1][200:264, 300:364])
    return imgs, small


@pytest.fixture(scope="module")
def oracle_results():
    """Per descriptor_order: the oracle's (keypoints, descriptors) of the three images and of the small one, computed once."""
    imgs, small = _images()
    out = {}
    for order in (0, 1, 2):
        o = OracleSession(threads=16, keep_levels=False, descriptor_order=order)
        n = o.run(imgs)
        big = [o.fetch(i) for i in range(len(imgs))]
        o.close()
        o = OracleSession(threads=4, keep_levels=False, descriptor_order=order, **SMALL)
        ns = o.run(small[None])
        out[order] = (n, big, ns, o.fetch(0))
        o.close()
    return out


def _check(g, order, want, first, tag, seen):
    for i, (ok, od) in enumerate(want):
        gk, gd = g.fetch(i)
        assert gk.tobytes() == ok.tobytes(), (tag, i)
        if order == 0:
            assert float(np.abs(gd - od).max()) <= TOL, (tag, i)
            seen.setdefault((first, i), gd.tobytes())
            assert gd.tobytes() == seen[(first, i)], (tag, i, "differs between HESS_DESC_XCD values")
        else:
            assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), (tag, i)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1, 2])
def test_results_do_not_depend_on_the_work_order(gpu_ctx_factory, monkeypatch, oracle_results, order):
    imgs, small = _images()
    n, big, ns, small_want = oracle_results[order]
    assert n[0] > 1000 and min(n) > 100 and ns[0] >= 1
    seen = {}  # interleaved order: the first block size's descriptor bytes, per (form, image)
    for xcd in XCD_BLOCKS:
        monkeypatch.setenv("HESS_DESC_XCD", xcd)
        # one image: descriptor_*_kernel<host mirror>; three: copier thread, the kernels without a mirror
        for form, batch in (("mirror", imgs[:1]), ("copier", imgs)):
            g = gpu_ctx_factory(dev_switches=True, descriptor_order=order)
            assert g.run(batch) == n[:len(batch)]
            _check(g, order, big[:len(batch)], form, (xcd, form), seen)
            g.close()
        # one image under DMA delivery: its features in several launches (DescParams::part, part_den)
        monkeypatch.setenv("HESS_DELIVERY", "dma")
        g = gpu_ctx_factory(dev_switches=True, descriptor_order=order)
        monkeypatch.delenv("HESS_DELIVERY")
        g.profile_enable()
        g.profile_reset()
        assert g.run(imgs[:1]) == n[:1]
        assert g.profile()["descriptor"]["launches"] > 1
        _check(g, order, big[:1], "parts", (xcd, "parts"), seen)
        g.close()
        # a grid below 128 workgroups
        g = gpu_ctx_factory(dev_switches=True, descriptor_order=order, **SMALL)
        assert g.run(small[None]) == ns
        _check(g, order, [small_want], "small", (xcd, "small"), seen)
        g.close()
