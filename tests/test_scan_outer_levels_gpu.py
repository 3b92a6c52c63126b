"""The streaming extrema scan (extrema_stream_kernel, dog <= 5) streams only the detection levels 1..dog; the outer levels
0 and dog+1 are read by key_eval, for the queued candidates of levels 1 and dog only.  The raw list, the keypoints and the
descriptors must stay those of the CPU oracle bit for bit, for both detectors, on inputs that reach the new branches:
no candidate at all (flat), candidates everywhere (noise), and blobs whose extrema lie on 32-column (128-byte line)
borders, scan strip edges (124 owned columns), the first and last rows of the 12- and 24-row scan segments and the first
and last interior rows and columns of the image (where the 1-D neighbour index wraps)."""
import numpy as np
import pytest

from hessgpu_amd import _abi
from oracle_lib import OracleSession
from test_dog_detector_gpu import _compare as _compare_dog
from test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

W, H = 700, 394  # neither a multiple of the strip pitch (124) nor of the segment lengths (12, 24)


def _run(gpu_ctx_factory, detector, imgs, what, **kw):
    if detector == "dog":
        g = gpu_ctx_factory(detector=_abi.DETECTOR_DOG, **kw)
        o = OracleSession(threads=8, detector=1, **kw)
        compare = _compare_dog
    else:
        g = gpu_ctx_factory(**kw)
        o = OracleSession(threads=8, **kw)
        compare = _compare_all
    try:
        return compare(g, o, imgs, f"{detector} {what} {kw}", stages=False)
    finally:
        o.close()


def _placed_blobs(k, w=W, h=H):
    """Bright and dark Gaussian blobs of several widths centred on line borders (multiples of 32), strip edges (multiples
    of 124), segment borders (multiples of 12) and the image's first and last rows and columns; image k shifts them by
    -1..+1 px so that the extrema fall on both sides of each border."""
    d = (-1, 0, 1)[k % 3]
    e = (0, 1, -1)[(k // 3) % 3]
    xs = sorted({c for c in list(range(32, w - 2, 32)) + list(range(124, w - 2, 124))} | {2, w - 3})
    ys = sorted(set(range(12, h - 2, 12)) | {2, h - 3})
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 128.0)
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            if (i + j) % 2:  # a checkerboard of the grid: blobs 24 px or more apart
                continue
            s = 1.0 + 0.45 * ((i + 2 * j + k) % 5)
            sign = 1.0 if (i // 2 + j + k) % 2 else -1.0
            cx, cy = min(max(x + d, 1), w - 2), min(max(y + e, 1), h - 2)
            img += sign * 100.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * s * s))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("detector", ["hessian", "dog"])
@pytest.mark.parametrize("batch", [1, 3])
def test_flat_image_has_no_detections(gpu_ctx_factory, detector, batch):
    imgs = np.full((batch, H, W), 97, np.uint8)
    n = _run(gpu_ctx_factory, detector, imgs, "flat")
    assert all(v == 0 for v in n), n


@pytest.mark.parametrize("detector", ["hessian", "dog"])
@pytest.mark.parametrize("dog", [1, 2, 3, 4, 5])
def test_noise_candidates_everywhere(gpu_ctx_factory, detector, dog):
    rng = np.random.RandomState(100 + dog)
    imgs = (rng.rand(2, H, W) * 255).astype(np.uint8)
    # (a low first threshold: nearly every local extremum of a level is queued)
    n = _run(gpu_ctx_factory, detector, imgs, "noise", dog_level_num=dog, dog_threshold=0.0005)
    assert min(n) > 40, n


@pytest.mark.parametrize("detector", ["hessian", "dog"])
@pytest.mark.parametrize("dog,batch", [(3, 1), (3, 3), (3, 8), (2, 3), (4, 3), (5, 3), (2, 8), (5, 1)])
def test_placed_blobs(gpu_ctx_factory, detector, dog, batch):
    imgs = np.stack([_placed_blobs(k) for k in range(batch)])
    n = _run(gpu_ctx_factory, detector, imgs, f"placed blobs x{batch}", dog_level_num=dog)
    assert min(n) > 20, n


@pytest.mark.parametrize("detector", ["hessian", "dog"])
def test_placed_blobs_first_octave_full_size_and_topk(gpu_ctx_factory, detector):
    # octave 0 at the image's own size (the grid's borders are the scan's borders there) and the top-K histogram path
    imgs = np.stack([_placed_blobs(k) for k in range(3)])
    _run(gpu_ctx_factory, detector, imgs, "placed blobs fo 0 topk", first_octave=0, truncate_method=_abi.TRUNC_TOPK,
         feature_count_threshold=300)
