"""Inputs for the detector tests and the one checker both callers use (a plain helper module, no tests in it).

check_against_model(session, case) runs a case on any Session -- the CPU oracle (tests/test_detector_model.py) or the
product context (tests/test_detector_model_gpu.py) -- and compares it stage by stage with np_restatement.DetectorModel,
every stage computed by the model FROM THE SESSION'S OWN PREVIOUS STAGE, so that errors do not accumulate and a failure
names the stage and the rule:

  geometry      octave sizes (decimation / up-sampling on input, -ads stepping, octave_num)                       exact
  gauss         level 0 from the pixels (conversion, decimation, up-sampling, first blur or its skip), level l from
                the session's level l - 1, level 0 of the next octave from the session's level `dog`               TOL_GAUSS
  det-H, grad, theta   from the session's Gaussian level                                                            TOL_*
  response      DoG mode, instead of det-H: D_l = G_l - G_(l-1) from the session's two Gaussian levels              exact
  detect        the raw list from the session's response planes: positions, order, type; list reduction and top-K  exact *
                offsets and response                                                                                2e-3, 1e-3
  orient        per raw item from the session's gradient planes: number of orientations, second truncation pass    exact *
                exported position / scale from the session's own offsets                                            one quantum
                orientation                                                                                         one quantum
  descriptor    a sample of <= 40, at the session's own quantised key                                               1e-4
  (*) except at items the model flags as uncertain (np_restatement.key_test_ex, orientations_ex): either answer passes.

The mode comes from session.params.detector.  In the difference-of-Gaussians mode an octave has the Gaussian levels
0 .. dog + 2 and the response planes 1 .. dog + 2 (the detector never reads response level 0, and neither does the
checker); list level l is scanned in the planes l, l + 1, l + 2 and described from Gaussian level l; where the two-peak
orientation branch ran the quantum is that of its 16-bit angles.

A case may carry `amp`, the amplitude of its float pixels (tests/float_range_cases.py; 1 otherwise): the absolute bounds
above are stated for luminance in [0, 1] and scale with it, and the response is compared as the half-precision number the
record packs, inf and subnormal steps included.

A case with batch_at = (n, i) runs as image i of a stack of n; the other images are seeded noise of the same size and
type (or the case's own `stack`), and image i is checked exactly as a single image would be.

small_cases() is a second dictionary, apart from cases(): planes below one tile of the kernels, with its own condition on
the statistics (check_small_statistics).

Images come from seeds; nothing here reads a file.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import fixtures
import np_restatement as R
from hessgpu_amd import _abi

# dense planes: the bounds of tests/test_oracle_vs_numpy.py
TOL_GAUSS = 2e-6
TOL_DETH = 1e-5          # x max(1, max |det-H|) (1: the square of the case's amplitude)
TOL_GRAD = 1e-6
TOL_THETA = 1e-5         # where the gradient is > 1e-6 (x the case's amplitude)
TOL_OFFSET = 2e-3
TOL_RESP = 1e-3          # relative; stated through the half the record packs (check_against_model)
QUANTUM = 2 * R.PI / 255.0
QUANTUM_16 = 2 * R.PI / 65535.0     # the two-peak branch of the difference-of-Gaussians mode
# Over one quantum (the floor of the code) an angle may differ by the binary32 error of what is floored.  The slack was set
# for the 8-bit angles and is kept for the 16-bit ones, a tenth of their quantum: the largest excess over one quantum that
# any case shows is 7e-8 rad, once the model takes the key position as the binary32 number it is (DetectorModel.key_geometry).
TOL_ANGLE = 1e-5
TOL_DESC = 1e-4
MAX_DESC = 40
MAX_UNCERTAIN_SHARE = 0.01

NOISE_KW = dict(dog_threshold=0.0005, edge_threshold=50.0)
DOG = dict(detector=_abi.DETECTOR_DOG)


def noise(w, h, seed=None):
    rng = np.random.RandomState(w * 131 + h if seed is None else seed)
    return (rng.rand(h, w) * 255).astype(np.uint8)


def blobs_noise(w=96, h=80, seed=5, amp=6.0):
    """fixtures.synthetic_blobs plus uniform noise of +-amp grey levels: blobs for the higher octaves, noise for many
    detections in the lower ones."""
    rng = np.random.RandomState(1000 + seed)
    img = fixtures.synthetic_blobs(w, h, seed).astype(np.float64) + (rng.rand(h, w) * 2 - 1) * amp
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


GRID_LAYERS = ((7, 1.9, 0.4), (15, 4.0, 0.5), (31, 8.0, 0.6))     # (period, sigma of the dots, gain)


def dot_grid(w=160, h=120, seed=7, layers=GRID_LAYERS):
    """Alternating bright / dark Gaussian dots on grids of three periods: a blob per dot and saddles between them, on
    several levels of several octaves.  The amplitudes come from a set of four, so that many detections share their
    half-precision response."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 0.5)
    for period, sigma, gain in layers:
        for cy in range(period // 2, h, period):
            for cx in range(period // 2, w, period):
                a = gain * (0.20 + 0.05 * rng.randint(0, 4)) * (1 if ((cx // period + cy // period) & 1) else -1)
                img += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))
    return np.clip(np.rint(img * 255), 0, 255).astype(np.uint8)


def colour(w=96, h=80, seed=3, bright=True):
    """u8 RGB with three different channels; bright: a third of the pixels near white (the 16-bit numerator wraps above
    2^31 / 65535 = 32768.5 grey levels of 65535, i.e. above half of full scale)."""
    chans = [blobs_noise(w, h, seed + i).astype(np.float64) for i in range(3)]
    img = np.stack(chans, axis=-1)
    if bright:
        img[:, w // 3: 2 * w // 3] = 128 + img[:, w // 3: 2 * w // 3] / 2
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _user_keys(w, h, seed=2):
    """Keys inside, on and beyond the border, scales inside every level's bin, clear of the bins' ends, and beyond the
    first and the last level."""
    rng = np.random.RandomState(seed)
    pts = []
    for x in (0.0, 1.4, w / 2.0, w - 1.4, float(w)):
        for y in (0.0, 1.6, h / 2.0, h - 0.7, float(h)):
            pts.append((x, y, 1.7 + 3.0 * rng.rand()))
    for s in (0.5, 1.2, 1.6, 2.0, 2.6, 3.2, 4.1, 5.0, 6.3, 8.2, 10.0, 13.0, 17.0, 40.0, 90.0):
        pts.append((w * (0.3 + 0.4 * rng.rand()), h * (0.3 + 0.4 * rng.rand()), s))
    keys = np.zeros(len(pts), dtype=_abi.KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["s"] = (np.array(v, dtype=np.float32) for v in zip(*pts))
    keys["o"] = ((keys["x"] * 0.37 + keys["y"] * 0.11 + keys["s"]) % 6.28).astype(np.float32)
    return keys


def _case(name, image, fmt=None, keys=None, have_orientation=1, min_features=1, batch_at=None, min_three_peaks=0, stack=None,
          **kw):
    return SimpleNamespace(name=name, image=image, fmt=fmt, keys=keys, have_orientation=have_orientation,
                           min_features=min_features, batch_at=batch_at, min_three_peaks=min_three_peaks, stack=stack, kw=kw)


def case_input(case):
    """-> (stack [n, H, W(, C)], index of the case's image in it).  batch_at = (n, i): the image at index i, seeded noise of
    the same shape and type elsewhere."""
    img = np.asarray(case.image)
    if case.batch_at is None:
        return img[None], 0
    n, at = case.batch_at
    if case.stack is not None:            # the whole stack is given: image `at` of it is the case's
        return case.stack, at
    top = 1.0 if img.dtype == np.float32 else float(np.iinfo(img.dtype).max)
    stack = [img if j == at else (np.random.RandomState(7919 + j).rand(*img.shape) * top).astype(img.dtype) for j in range(n)]
    return np.stack(stack), at


@functools.lru_cache(maxsize=None)
def cases():
    """-> {name: case}.  kw are hess_params overrides; the image is built on first use."""
    out = []
    for w, h in ((132, 25), (260, 49), (324, 223)):
        out.append(_case(f"noise {w}x{h}", noise(w, h), **NOISE_KW))
    b = blobs_noise()
    out.append(_case("first_octave -1", b, first_octave=-1))
    out.append(_case("first_octave -2", b, first_octave=-2))
    out.append(_case("first_octave -5 ads", b, first_octave=-5, auto_downscale=1, tex_max_dim=200))
    out.append(_case("first_octave 1", noise(324, 223), first_octave=1, **NOISE_KW))
    for dog in (1, 2, 4, 5, 6):
        out.append(_case(f"dog_level_num {dog}", b, dog_level_num=dog, dog_threshold=0.002))
    out.append(_case("sigman 1.56", b, sigman=1.56))                       # first blur of sigma 0.36: 3 taps, clamped to 5
    out.append(_case("factors", b, filter_width_factor=5.0, orient_window_factor=1.5, orient_gaussian_factor=1.2,
                     desc_window_factor=2.5))
    out.append(_case("subpixel 0", b, subpixel=0))
    out.append(_case("half_sift", b, half_sift=1))
    out.append(_case("max_orientation 1", b, max_orientation=1))
    out.append(_case("half_sift max_orientation 1", b, half_sift=1, max_orientation=1))
    out.append(_case("fixed_orientation", b, fixed_orientation=1))
    out.append(_case("lowe_origin", b, lowe_origin=1, dog_threshold=0.004, edge_threshold=5.0))
    out.append(_case("octave_num 2", b, octave_num=2))
    out.append(_case("octave_num 9", b, octave_num=9))
    out.append(_case("normalize 0", b, normalize=0))
    out.append(_case("dynamic_indexing", b, dynamic_indexing=1))
    g = dot_grid()
    gk = GRID_KW
    for name, method, thr in (("highest0", _abi.TRUNC_HIGHEST_0, GRID_THRESHOLD), ("highest1", _abi.TRUNC_HIGHEST_1, GRID_THRESHOLD),
                              ("lowest", _abi.TRUNC_LOWEST, GRID_THRESHOLD_LOWEST)):
        out.append(_case(f"truncate {name}", g, truncate_method=method, feature_count_threshold=thr, **gk))
    out.append(_case("top-K", g, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=GRID_TOPK, **gk))
    out.append(_case("top-K above the count", g, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=100000, **gk))
    c = colour()
    ck = COLOUR_KW
    alpha = np.full(c.shape[:2] + (1,), 255, np.uint8)
    out.append(_case("u8 rgb", c, **ck))
    out.append(_case("u8 lum", c[..., 1].copy(), **ck))
    out.append(_case("u16 rgb", c.astype(np.uint16) * 257, **ck))
    out.append(_case("u16 lum", c[..., 1].astype(np.uint16) * 257, **ck))
    out.append(_case("f32 lum", (c[..., 1] / 255.0).astype(np.float32), **ck))
    out.append(_case("f32 rgb", (c / 255.0).astype(np.float32), **ck))
    out.append(_case("f32 bgr", (c[..., ::-1] / 255.0).astype(np.float32), fmt=_abi.FMT_BGR, **ck))
    # float pixels are taken as they come: luminance in 0 .. 255 through the DEFAULT parameters (the product's default
    # descriptor order, PIXEL, silently becomes INTERLEAVED for float pixels: hess_schedule.hip, and the oracle alike)
    out.append(_case("f32 lum 0..255 defaults", c[..., 1].astype(np.float32), min_features=100))
    out.append(_case("f32 rgb 0..255 defaults", c.astype(np.float32), min_features=100))
    out.append(_case("u8 rgba", np.concatenate([c, alpha], axis=2), **ck))
    out.append(_case("u8 bgr", np.ascontiguousarray(c[..., ::-1]), fmt=_abi.FMT_BGR, **ck))
    out.append(_case("u8 bgra", np.concatenate([c[..., ::-1], alpha], axis=2), fmt=_abi.FMT_BGRA, **ck))
    keys = _user_keys(96, 80)
    for ho in (1, 0):
        out.append(_case(f"keypoint list orient={ho}", b, keys=keys, have_orientation=ho))
        out.append(_case(f"keypoint list orient={ho} first_octave -1 lowe", b, keys=keys, have_orientation=ho, first_octave=-1,
                         lowe_origin=1))
    out.append(_case("keypoint list half_sift", b, keys=keys, have_orientation=0, half_sift=1))
    out.append(_case("keypoint list max_orientation 1", b, keys=keys, have_orientation=0, max_orientation=1))
    out.append(_case("keypoint list fixed_orientation", b, keys=keys, have_orientation=0, fixed_orientation=1))
    out.append(_case("noise 260x49 batch 3", noise(260, 49), batch_at=(3, 1), **NOISE_KW))
    out.extend(_dog_cases(b, g, c, keys))
    return {c.name: c for c in out}


def _dog_cases(b, g, c, keys):
    """The difference-of-Gaussians mode (kw carries detector = 1).  White noise has few extrema in scale -- the finer
    difference is the stronger one nearly everywhere -- so the two small noise images come from seeds chosen for their
    number of detections (DOG_NOISE_SEEDS), and the thresholds of the Hessian cases, which count det-H, are not taken over:
    the defaults (0.02 / dog, 10) serve unless a case says otherwise.  b6: blobs_noise with another seed, for three cases
    in which the usual one has a flagged orientation among fewer than 100 candidates."""
    d = DOG
    b6 = blobs_noise(seed=6)
    out = []
    for w, h in ((132, 25), (260, 49), (324, 223)):
        out.append(_case(f"dog: noise {w}x{h}", noise(w, h, DOG_NOISE_SEEDS.get((w, h))), **NOISE_KW, **d))
    out.append(_case("dog: noise 260x49 batch 3", noise(260, 49, DOG_NOISE_SEEDS[260, 49]), batch_at=(3, 1), **NOISE_KW, **d))
    out.append(_case("dog: defaults", b, **d))
    out.append(_case("dog: first_octave -1", b6, first_octave=-1, **d))
    out.append(_case("dog: first_octave 1", noise(324, 223), first_octave=1, **NOISE_KW, **d))
    out.append(_case("dog: first_octave -2", b, first_octave=-2, **d))
    for dog in (1, 2, 5, 6):
        out.append(_case(f"dog: dog_level_num {dog}", b6 if dog == 1 else b, dog_level_num=dog, **d))
    out.append(_case("dog: subpixel 0", b, subpixel=0, **d))
    out.append(_case("dog: max_orientation 1", b, max_orientation=1, **d))
    # the dot grid: dots of three periods overlap into patches with several dominant directions
    out.append(_case("dog: max_orientation 4", g, max_orientation=4, min_three_peaks=5, **d))
    out.append(_case("dog: fixed_orientation", b, fixed_orientation=1, **d))
    out.append(_case("dog: half_sift", b, half_sift=1, **d))
    out.append(_case("dog: half_sift max_orientation 4", b, half_sift=1, max_orientation=4, **d))
    out.append(_case("dog: lowe_origin first_octave -1", b6, lowe_origin=1, first_octave=-1, **d))
    for name, method, thr in (("highest0", _abi.TRUNC_HIGHEST_0, DOG_GRID_THRESHOLD), ("highest1", _abi.TRUNC_HIGHEST_1, DOG_GRID_THRESHOLD),
                              ("lowest", _abi.TRUNC_LOWEST, DOG_GRID_THRESHOLD_LOWEST)):
        out.append(_case(f"dog: truncate {name}", g, truncate_method=method, feature_count_threshold=thr, **d))
    out.append(_case("dog: top-K", g, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=DOG_GRID_TOPK, **d))
    ck = DOG_COLOUR_KW
    out.append(_case("dog: u8 rgb", c, **ck, **d))
    out.append(_case("dog: u16 rgb", c.astype(np.uint16) * 257, **ck, **d))
    out.append(_case("dog: f32 lum", (c[..., 1] / 255.0).astype(np.float32), **ck, **d))
    out.append(_case("dog: keypoint list orient=1", b, keys=keys, have_orientation=1, **d))
    out.append(_case("dog: keypoint list orient=0", b, keys=keys, have_orientation=0, **d))
    out.append(_case("dog: keypoint list orient=0 first_octave -1 lowe", b, keys=keys, have_orientation=0, first_octave=-1,
                     lowe_origin=1, **d))
    return out


# ---- planes below one tile -------------------------------------------------------------------------------------------
# The kernels work on fixed blocks -- 64 x 32 Gaussian tiles with halos of up to 16 taps, 32 x 32 chain tiles, 128 x 4
# extrema tiles, 128-column scan strips in 24-row segments, 64-column row-mask words, a descriptor raster in 64-row bands
# -- and cases() has few partial ones.  Here every block is partial, and every index a clamped or a wrapped one.
SMALL_PLANES = {      # (w, h): what the size straddles
    (4, 1): "the smallest legal plane",
    (4, 2): "two rows, no interior row",
    (4, 3): "one interior row",
    (5, 5): "width truncated to 4",
    (7, 2): "width truncated to 4, no interior row",
    (8, 8): "below every halo",
    (12, 3): "narrower than a halo",
    (36, 5): "wider than a chain tile, lower than any tile",
    (68, 4): "one word past a 64-column tile, one extrema row group",
    (64, 1): "one row-mask word, one row",
    (300, 3): "three scan strips, one interior row",
    (4, 300): "one word wide, thirteen scan segments",
    (17, 23): "width truncated to 16, below one tile",
    (31, 31): "one short of a chain tile",
    (200, 16): "as many rows as the widest filter's radius",
}
SMALL_PYRAMIDS = {
    (32, 32): "second octave 16x16",
    (35, 64): "second octave 16x32, odd half",
    (64, 33): "second octave 32x16",
    (65, 33): "second octave 32x16, odd halves",
    (67, 35): "second octave 32x17, odd halves",
    (1000, 33): "thin second octave 500x16",
    (33, 700): "thin second octave 16x350",
    (128, 64): "three octaves",
}
SMALL_INPUT = ((4, 1), (12, 3), (36, 5), (65, 33))
SMALL_KEY_SIZES = ((4, 1), (4, 3), (7, 2), (12, 3), (36, 5), (64, 1), (17, 23), (4, 300), (300, 3))
SMALL_KEY_MODES = {"defaults": {}, "dog": DOG, "half_sift": dict(half_sift=1), "normalize 0": dict(normalize=0),
                   "first_octave -1": dict(first_octave=-1)}


def constant_stack(w, h, n=8):
    """Eight images of one size for the packed results: seeded noise, with constant images (no feature) at 0, 3, 4 and 7,
    so that empty images stand first, last and between non-empty ones."""
    stack = np.stack([noise(w, h, 4001 + j) for j in range(n)])
    for j, v in ((0, 0), (3, 255), (4, 17), (7, 128)):
        stack[j] = v
    return stack


@functools.lru_cache(maxsize=None)
def small_cases():
    """-> {name: case}: planes below one tile, the smallest pyramids, the input stages, batches and keypoint lists on
    them.  Apart from cases(): its parametrisations and statistics stay as they are.  min_features is what the oracle
    gives (SMALL_FEATURES; 0 where the plane has no interior, or nothing in it is found: those cases test the planes)."""
    out = []
    k = NOISE_KW

    def add(name, image, **kw):
        out.append(_case(name, image, min_features=SMALL_FEATURES[name], **kw))

    for (w, h), what in SMALL_PLANES.items():
        add(f"{w}x{h}: {what}", noise(w, h), **k)
        add(f"dog: {w}x{h}: {what}", noise(w, h), **k, **DOG)
    for w, h in ((4, 1), (8, 8), (12, 3), (4, 300), (200, 16)):           # 33 taps on fewer than 16 rows or columns
        add(f"{w}x{h} dog_level_num 1", noise(w, h), dog_level_num=1, **k)
    add("dog: 12x3 dog_level_num 1", noise(12, 3), dog_level_num=1, **k, **DOG)
    for w, h in ((12, 3), (68, 4), (31, 31), (200, 16)):                  # the LDS-tiled extrema scan
        add(f"{w}x{h} dog_level_num 6", noise(w, h), dog_level_num=6, **k)
    add("dog: 31x31 dog_level_num 6", noise(31, 31), dog_level_num=6, **k, **DOG)
    for (w, h), what in SMALL_PYRAMIDS.items():
        add(f"{w}x{h}: {what}", noise(w, h), **k)
        add(f"dog: {w}x{h}: {what}", noise(w, h), **k, **DOG)
    for fo in (-1, -2):                                                   # the up-sampling kernel
        for w, h in SMALL_INPUT + ((31, 31), (200, 16)):
            add(f"first_octave {fo} {w}x{h}", noise(w, h), first_octave=fo, **k)
    for w, h in ((8, 2), (8, 8), (12, 3), (300, 3)):                      # decimation down to 4 x 1
        add(f"first_octave 1 {w}x{h}", noise(w, h), first_octave=1, **k)
    for w, h in SMALL_INPUT:                                              # convert_kernel instead of the direct u8 path
        rgb = np.stack([noise(w, h, 5000 + 7 * i + w) for i in range(3)], axis=-1)
        add(f"u8 rgb {w}x{h}", rgb, **k)
        add(f"f32 lum {w}x{h}", (noise(w, h) / 255.0).astype(np.float32), **k)
    for w, h in SMALL_INPUT:
        add(f"batch 8 image 5 {w}x{h}", noise(w, h), batch_at=(8, 5), **k)
    cs = constant_stack(65, 33)                                           # feature-less images around and between the others
    add("batch 8 image 5 65x33 between constant images", cs[5], batch_at=(8, 5), stack=cs, **k)
    for sz in SMALL_KEY_SIZES:
        w, h = sz
        for mode, kw in SMALL_KEY_MODES.items():
            for ho in (1, 0):
                add(f"keypoint list {w}x{h} {mode} orient={ho}", noise(w, h), keys=_user_keys(w, h), have_orientation=ho, **kw)
    assert len({c.name for c in out}) == len(out) and {c.name for c in out} == set(SMALL_FEATURES)
    return {c.name: c for c in out}


def check_small_statistics(st, case):
    """A condition on check_against_model's statistics for a small case: it has the features the oracle finds; below 100
    candidates no detection and no orientation is flagged (a flagged item passes with either answer, and a case of ten
    candidates must not pass on one), above that at most MAX_UNCERTAIN_SHARE; no orientation of a keypoint list is
    flagged: the all-zero histogram has a rule (np_restatement.orientations_ex)."""
    assert st["features"] >= case.min_features, (st, case.min_features)
    if case.keys is not None:
        assert st["orient_uncertain"] == 0, st
        return
    flagged = st["uncertain"] + st["orient_uncertain"]
    if st["candidates"] < 100:
        assert flagged == 0, st
    else:
        assert flagged <= MAX_UNCERTAIN_SHARE * st["candidates"], st


# Features per small case, from the oracle (tests/test_small_images.py holds the oracle to the model on each).  0: the plane
# has no interior row, or nothing in it passes the tests; such a case is there for its planes.
SMALL_FEATURES = {
    "4x1: the smallest legal plane": 0, "dog: 4x1: the smallest legal plane": 0, "4x2: two rows, no interior row": 0,
    "dog: 4x2: two rows, no interior row": 0, "4x3: one interior row": 0, "dog: 4x3: one interior row": 0,
    "5x5: width truncated to 4": 0, "dog: 5x5: width truncated to 4": 0, "7x2: width truncated to 4, no interior row": 0,
    "dog: 7x2: width truncated to 4, no interior row": 0, "8x8: below every halo": 0, "dog: 8x8: below every halo": 0,
    "12x3: narrower than a halo": 0, "dog: 12x3: narrower than a halo": 0,
    "36x5: wider than a chain tile, lower than any tile": 0, "dog: 36x5: wider than a chain tile, lower than any tile": 0,
    "68x4: one word past a 64-column tile, one extrema row group": 0,
    "dog: 68x4: one word past a 64-column tile, one extrema row group": 0, "64x1: one row-mask word, one row": 0,
    "dog: 64x1: one row-mask word, one row": 0, "300x3: three scan strips, one interior row": 0,
    "dog: 300x3: three scan strips, one interior row": 0, "4x300: one word wide, thirteen scan segments": 0,
    "dog: 4x300: one word wide, thirteen scan segments": 0, "17x23: width truncated to 16, below one tile": 1,
    "dog: 17x23: width truncated to 16, below one tile": 0, "31x31: one short of a chain tile": 2,
    "dog: 31x31: one short of a chain tile": 0, "200x16: as many rows as the widest filter's radius": 9,
    "dog: 200x16: as many rows as the widest filter's radius": 0, "4x1 dog_level_num 1": 0, "8x8 dog_level_num 1": 0,
    "12x3 dog_level_num 1": 0, "4x300 dog_level_num 1": 0, "200x16 dog_level_num 1": 2, "dog: 12x3 dog_level_num 1": 0,
    "12x3 dog_level_num 6": 0, "68x4 dog_level_num 6": 1, "31x31 dog_level_num 6": 3, "200x16 dog_level_num 6": 14,
    "dog: 31x31 dog_level_num 6": 0, "32x32: second octave 16x16": 3, "dog: 32x32: second octave 16x16": 0,
    "35x64: second octave 16x32, odd half": 15, "dog: 35x64: second octave 16x32, odd half": 4,
    "64x33: second octave 32x16": 7, "dog: 64x33: second octave 32x16": 2, "65x33: second octave 32x16, odd halves": 6,
    "dog: 65x33: second octave 32x16, odd halves": 2, "67x35: second octave 32x17, odd halves": 20,
    "dog: 67x35: second octave 32x17, odd halves": 3, "1000x33: thin second octave 500x16": 126,
    "dog: 1000x33: thin second octave 500x16": 19, "33x700: thin second octave 16x350": 63,
    "dog: 33x700: thin second octave 16x350": 20, "128x64: three octaves": 33, "dog: 128x64: three octaves": 8,
    "first_octave -1 4x1": 0, "first_octave -1 12x3": 0, "first_octave -1 36x5": 1, "first_octave -1 65x33": 40,
    "first_octave -1 31x31": 15, "first_octave -1 200x16": 54, "first_octave -2 4x1": 0, "first_octave -2 12x3": 10,
    "first_octave -2 36x5": 60, "first_octave -2 65x33": 863, "first_octave -2 31x31": 361,
    "first_octave -2 200x16": 1375, "first_octave 1 8x2": 0, "first_octave 1 8x8": 0, "first_octave 1 12x3": 0,
    "first_octave 1 300x3": 0, "u8 rgb 4x1": 0, "f32 lum 4x1": 0, "u8 rgb 12x3": 0, "f32 lum 12x3": 0, "u8 rgb 36x5": 0,
    "f32 lum 36x5": 0, "u8 rgb 65x33": 7, "f32 lum 65x33": 6, "batch 8 image 5 4x1": 0, "batch 8 image 5 12x3": 0,
    "batch 8 image 5 36x5": 0, "batch 8 image 5 65x33": 6, "batch 8 image 5 65x33 between constant images": 6,
    "keypoint list 4x1 defaults orient=1": 40,
    "keypoint list 4x1 defaults orient=0": 40, "keypoint list 4x1 dog orient=1": 40, "keypoint list 4x1 dog orient=0": 40,
    "keypoint list 4x1 half_sift orient=1": 40, "keypoint list 4x1 half_sift orient=0": 40,
    "keypoint list 4x1 normalize 0 orient=1": 40, "keypoint list 4x1 normalize 0 orient=0": 40,
    "keypoint list 4x1 first_octave -1 orient=1": 40, "keypoint list 4x1 first_octave -1 orient=0": 40,
    "keypoint list 4x3 defaults orient=1": 40, "keypoint list 4x3 defaults orient=0": 40,
    "keypoint list 4x3 dog orient=1": 40, "keypoint list 4x3 dog orient=0": 40,
    "keypoint list 4x3 half_sift orient=1": 40, "keypoint list 4x3 half_sift orient=0": 40,
    "keypoint list 4x3 normalize 0 orient=1": 40, "keypoint list 4x3 normalize 0 orient=0": 40,
    "keypoint list 4x3 first_octave -1 orient=1": 40, "keypoint list 4x3 first_octave -1 orient=0": 40,
    "keypoint list 7x2 defaults orient=1": 40, "keypoint list 7x2 defaults orient=0": 40,
    "keypoint list 7x2 dog orient=1": 40, "keypoint list 7x2 dog orient=0": 40,
    "keypoint list 7x2 half_sift orient=1": 40, "keypoint list 7x2 half_sift orient=0": 40,
    "keypoint list 7x2 normalize 0 orient=1": 40, "keypoint list 7x2 normalize 0 orient=0": 40,
    "keypoint list 7x2 first_octave -1 orient=1": 40, "keypoint list 7x2 first_octave -1 orient=0": 40,
    "keypoint list 12x3 defaults orient=1": 40, "keypoint list 12x3 defaults orient=0": 40,
    "keypoint list 12x3 dog orient=1": 40, "keypoint list 12x3 dog orient=0": 40,
    "keypoint list 12x3 half_sift orient=1": 40, "keypoint list 12x3 half_sift orient=0": 40,
    "keypoint list 12x3 normalize 0 orient=1": 40, "keypoint list 12x3 normalize 0 orient=0": 40,
    "keypoint list 12x3 first_octave -1 orient=1": 40, "keypoint list 12x3 first_octave -1 orient=0": 40,
    "keypoint list 36x5 defaults orient=1": 40, "keypoint list 36x5 defaults orient=0": 40,
    "keypoint list 36x5 dog orient=1": 40, "keypoint list 36x5 dog orient=0": 40,
    "keypoint list 36x5 half_sift orient=1": 40, "keypoint list 36x5 half_sift orient=0": 40,
    "keypoint list 36x5 normalize 0 orient=1": 40, "keypoint list 36x5 normalize 0 orient=0": 40,
    "keypoint list 36x5 first_octave -1 orient=1": 40, "keypoint list 36x5 first_octave -1 orient=0": 40,
    "keypoint list 64x1 defaults orient=1": 40, "keypoint list 64x1 defaults orient=0": 40,
    "keypoint list 64x1 dog orient=1": 40, "keypoint list 64x1 dog orient=0": 40,
    "keypoint list 64x1 half_sift orient=1": 40, "keypoint list 64x1 half_sift orient=0": 40,
    "keypoint list 64x1 normalize 0 orient=1": 40, "keypoint list 64x1 normalize 0 orient=0": 40,
    "keypoint list 64x1 first_octave -1 orient=1": 40, "keypoint list 64x1 first_octave -1 orient=0": 40,
    "keypoint list 17x23 defaults orient=1": 40, "keypoint list 17x23 defaults orient=0": 40,
    "keypoint list 17x23 dog orient=1": 40, "keypoint list 17x23 dog orient=0": 40,
    "keypoint list 17x23 half_sift orient=1": 40, "keypoint list 17x23 half_sift orient=0": 40,
    "keypoint list 17x23 normalize 0 orient=1": 40, "keypoint list 17x23 normalize 0 orient=0": 40,
    "keypoint list 17x23 first_octave -1 orient=1": 40, "keypoint list 17x23 first_octave -1 orient=0": 40,
    "keypoint list 4x300 defaults orient=1": 40, "keypoint list 4x300 defaults orient=0": 40,
    "keypoint list 4x300 dog orient=1": 40, "keypoint list 4x300 dog orient=0": 40,
    "keypoint list 4x300 half_sift orient=1": 40, "keypoint list 4x300 half_sift orient=0": 40,
    "keypoint list 4x300 normalize 0 orient=1": 40, "keypoint list 4x300 normalize 0 orient=0": 40,
    "keypoint list 4x300 first_octave -1 orient=1": 40, "keypoint list 4x300 first_octave -1 orient=0": 40,
    "keypoint list 300x3 defaults orient=1": 40, "keypoint list 300x3 defaults orient=0": 40,
    "keypoint list 300x3 dog orient=1": 40, "keypoint list 300x3 dog orient=0": 40,
    "keypoint list 300x3 half_sift orient=1": 40, "keypoint list 300x3 half_sift orient=0": 40,
    "keypoint list 300x3 normalize 0 orient=1": 40, "keypoint list 300x3 normalize 0 orient=0": 40,
    "keypoint list 300x3 first_octave -1 orient=1": 40, "keypoint list 300x3 first_octave -1 orient=0": 40,
}


# The dot grid has [345, 219, 34, 1, 50, 10, 2, 7] detections and [381, 282, 43, 1, 59, 14, 3, 22] features per level
# (tests/test_detector_model.py::test_grid_thresholds_fall_inside_a_level asserts it).  120 lies inside level 1 counted from
# the top (104 detections above it, 323 with it): the first pass keeps level 1, the second, on the 424 features, drops it
# (424 - 282 = 142 > 120).  400 lies inside level 1 counted from the bottom.  192: the detections ranked 191, 192 and 193 by
# abs(half(response)) are equal, so the top-K cut separates equals.
#
# 'truncate highest0' and 'truncate highest1' give the same features here, and at every threshold: method 1 stops generating
# lists, walking downwards, once the levels above hold more than the threshold (PyramidCU.cpp:1314-1319), and method 0's
# LimitFeatureCount drops a level, walking upwards, while the levels above it hold more than the threshold
# (SiftPyramid.cpp:224-277) -- one condition, stated twice.  They differ in the work done, not in the result, so no
# case can tell a product that mixed the two up; the pair of cases pins that both reach the common result.
GRID_KW = dict(dog_threshold=0.0004, edge_threshold=60.0)
# The mean of three channels, and the bright band at half contrast, leave little above the default thresholds.
COLOUR_KW = dict(dog_threshold=0.0015, edge_threshold=20.0)
GRID_THRESHOLD = 120
GRID_THRESHOLD_LOWEST = 400
GRID_TOPK = 192
# The same grid in the difference-of-Gaussians mode, at the default thresholds: [173, 68, 1, 2, 21, 0, 0, 0] detections and
# [196, 89, 2, 3, 26, 0, 0, 0] features per level (test_dog_grid_thresholds_fall_inside_a_level).  27: the levels above level
# 1 hold 24 detections, so the first pass keeps level 1 (92 with it); above it are 31 features, so the second pass drops it.
# 200 lies inside level 1 counted from the bottom (173, 241 with it).  124: the detections ranked 123, 124 and 125 by
# abs(half(response)) are equal.
DOG_GRID_THRESHOLD = 27
DOG_GRID_THRESHOLD_LOWEST = 200
DOG_GRID_TOPK = 124
DOG_COLOUR_KW = dict(dog_threshold=0.003, edge_threshold=10.0)
# noise(w, h, seed) with at least 8 detections in the difference-of-Gaussians mode at NOISE_KW; of the seeds 0 .. 64399 one
# gives 8 on 132 x 25 (the median is 1), 394 is the best of 0 .. 399 on 260 x 49 (14; the median is 6)
DOG_NOISE_SEEDS = {(132, 25): 21600, (260, 49): 394}


def _circ(a, b):
    d = abs(a - b) % (2 * R.PI)
    return min(d, 2 * R.PI - d)


def _half(packed):
    return float(np.array([int(packed) >> 16], dtype=np.uint16).view(np.float16)[0])


class Mismatch(AssertionError):
    """A stage of the session does not follow the model: .stage names it."""

    def __init__(self, stage, msg):
        super().__init__(f"[{stage}] {msg}")
        self.stage = stage


def _need(cond, stage, msg):
    if not cond:
        raise Mismatch(stage, msg() if callable(msg) else msg)


def check_against_model(session, case, model=None, dense=True, log=None):
    """Run `case` on `session` and compare every stage with the model (default: the right rules for session.params).
    -> statistics: candidates, uncertain (detection), detections, features, orient_uncertain, descriptors checked and the
    largest deviation per stage.  Raises Mismatch."""
    m = model or R.DetectorModel(session.params)
    img = np.asarray(case.image)
    # The amplitude of a float case's pixels (float_range_cases sets case.amp; 1 otherwise): every ABSOLUTE gate of the
    # checker is stated for luminance in [0, 1] and scales with it -- the planes and the gradient by amp, det-H and its
    # response by amp^2, an unnormalised descriptor by amp.  The reference's own absolute constants (the 1e-10 pivots) do not.
    amp = float(getattr(case, "amp", 1.0))
    tol_desc = TOL_DESC if m.normalize else TOL_DESC * amp
    h, w = img.shape[:2]
    st = dict(candidates=0, uncertain=0, orient_uncertain=0, gauss=0.0, deth=0.0, grad=0.0, theta=0.0, desc=0.0,
              angle=0.0, three_peaks=0)
    is_dog = int(session.params.detector) == _abi.DETECTOR_DOG
    _need(m.is_dog == is_dog, "geometry", "the model is not in the session's mode")
    session.keep_levels(True)
    stack, bi = case_input(case)
    session.run(stack, fmt=case.fmt)
    ds, omin, geo, scales = m.plan(w, h)
    _need(session.geometry() == geo, "geometry", lambda: f"{session.geometry()} != {geo}")
    dog, nlev = m.dog, m.nlev
    # the response planes the scans read (a wrong-rule model may ask for level 0; the right DoG rules never do)
    first_d = min(min(m.scan_planes(l)) for l in range(1, dog + 1)) if is_dog else 0

    # ---- dense planes
    G = [[session.level(bi, oc, l, _abi.DBG_GAUSS) for l in range(nlev)] for oc in range(len(geo))]
    D = [[session.level(bi, oc, l, _abi.DBG_DETH) if l >= first_d else None for l in range(nlev)] for oc in range(len(geo))]
    GOT = [[session.level(bi, oc, l, _abi.DBG_GOT).astype(np.float64) if 1 <= l <= dog else None for l in range(nlev)]
           for oc in range(len(geo))]
    if dense:
        base, taps0 = m.base_plane(img, case.fmt)
        # binary32 rounds relative to the magnitude: float pixels are taken as they come (0 .. 255, say), and the absolute
        # bounds of the planes, stated for luminance in [0, 1], grow with the largest pixel (1 for every 8- and 16-bit case)
        # and shrink with a case's stated amplitude below 1 (float_range_cases; 1 for every other case)
        mag = max(amp, float(np.abs(base).max()))
        for oc, (wa, hh) in enumerate(geo):
            for l in range(nlev):
                a = G[oc][l].astype(np.float64)
                if l == 0 and oc == 0:
                    want = base if taps0 is None else R.gaussian(base, taps0)
                elif l == 0:
                    want = R.downsample(G[oc - 1][m.level_ds].astype(np.float64), wa, hh)
                else:
                    want = R.gaussian(G[oc][l - 1].astype(np.float64), m.level_taps(l))
                _need(a.shape == want.shape, "gauss", lambda: f"octave {oc} level {l}: shape {a.shape} != {want.shape}")
                d = float(np.abs(a - want).max())
                st["gauss"] = max(st["gauss"], d)
                _need(d < TOL_GAUSS * mag, "gauss", lambda: f"octave {oc} level {l}: max |d| {d:.3g}")
                # (gradient and angle are the same lines in both kernels: ProgramCU.cu:567-591 and :612-621)
                deth, grad, theta = m.planes(a, l)
                if is_dog:
                    if l >= 1:       # exact: a correctly rounded binary32 subtraction of these two planes has one answer
                        want = m.response_plane(G[oc][l], G[oc][l - 1])
                        bad = int((D[oc][l] != want).sum())
                        _need(bad == 0, "response", lambda: f"octave {oc} level {l}: {bad} pixels are not G_l - G_(l-1)")
                else:
                    d = float(np.abs(D[oc][l] - deth).max()) / max(amp * amp, float(np.abs(deth).max()))
                    st["deth"] = max(st["deth"], d)
                    _need(d < TOL_DETH, "det-H", lambda: f"octave {oc} level {l}: {d:.3g} of the plane's maximum")
                if 1 <= l <= dog:
                    got = GOT[oc][l]
                    d = float(np.abs(got[..., 0] - grad).max())
                    st["grad"] = max(st["grad"], d)
                    _need(d < TOL_GRAD * mag, "gradient", lambda: f"octave {oc} level {l}: {d:.3g}")
                    dang = np.abs(np.angle(np.exp(1j * (got[..., 1] - theta))))
                    sel = grad > 1e-6 * mag
                    d = float(dang[sel].max()) if sel.any() else 0.0
                    st["theta"] = max(st["theta"], d)
                    _need(d < TOL_THETA, "theta", lambda: f"octave {oc} level {l}: {d:.3g}")

    if case.keys is not None:
        _check_keypoint_list(session, case, m, GOT, scales, st, tol_desc)
        return st

    # ---- detection from the session's response planes
    raw = session.rawlist(bi)
    found, unsure = [], []
    for oc in range(len(geo)):
        for l in range(1, dog + 1):
            pc, pp, pn = m.scan_planes(l)
            f, u, n = m.scan(D[oc][pc], D[oc][pp], D[oc][pn], G[oc][l])
            found.append(f)
            unsure.append(u)
            st["candidates"] += n
            st["uncertain"] += len(u)
    reducing = m.fct > 0
    full_counts = [len(f) for f in found]
    kept = m.reduce_first(full_counts)
    expect = [sorted(f) if k else [] for f, k in zip(found, kept)]
    if m.method == R.TRUNC_TOPK and reducing:
        flat = [(li, pos) for li, lst in enumerate(expect) for pos in lst]
        resp = [found[li][pos][0] for li, pos in flat]
        keep = m.topk(resp)
        if len(keep) < len(flat):
            key = sorted((abs(m.packed_half(r)) for r in resp), reverse=True)
            cut_in, cut_out = key[m.fct - 1], key[m.fct]
            st["topk_tie_at_cut"] = int(cut_in == cut_out)
            # a response at a rounding boundary of binary16 next to the cut would make the cut depend on float32 rounding
            for r in resp:
                lo, hi = abs(m.packed_half(abs(r) * (1 - 32 * R.U))), abs(m.packed_half(abs(r) * (1 + 32 * R.U)))
                _need(lo == hi or hi < cut_out or lo > cut_in, "detect", f"response {r!r} decides the top-K cut by rounding")
        expect = [[] for _ in expect]
        for i in keep:
            expect[flat[i][0]].append(flat[i][1])
    if reducing:
        _need(not any(unsure), "detect", lambda: f"uncertain detections in a case that reduces the list: {unsure}")
    for li in range(len(expect)):
        sel = raw[raw["level_index"] == li]
        got = [(int(k["row"]), int(k["col"])) for k in sel]
        bad = (set(got) ^ set(expect[li])) - unsure[li]
        _need(not bad, "detect", lambda: f"level {li}: {len(got)} detections, model {len(expect[li])}; differ at (row, col) "
                                         f"{sorted(bad)[:8]}")
        _need(got == sorted(got), "detect", f"level {li}: the list is not in row-major order")
        for k in sel:
            pos = (int(k["row"]), int(k["col"]))
            if pos not in found[li]:
                continue
            resp, typ, dx, dy, dsc = found[li][pos]
            pk = int(k["packed"])
            _need(pk & 4 and (pk & 3 == typ or pos in unsure[li]), "detect", f"level {li} {pos}: type {pk & 3}, model {typ}")
            # The packed response is half(r') of the binary32 r'; the model has r' in float64.  Every binary32 value within
            # TOL_RESP / 2 of the model's must pack to a half between the halves of the interval's ends -- inf above 65504,
            # steps of 2^-24 below 2^-14, 0 below 2^-25.  On normal halves that is |half - r'| <= (TOL_RESP / 2 + 2^-11)
            # |r'| < TOL_RESP |r'|, inside the bound this line had before, whose absolute term stood for the subnormal step.
            lo, hi = sorted((m.packed_half(resp * (1 - TOL_RESP / 2)), m.packed_half(resp * (1 + TOL_RESP / 2))))
            _need(lo <= _half(pk) <= hi, "detect", f"level {li} {pos}: response {_half(pk)} model half({resp}) = {m.packed_half(resp)}")
            _need(max(abs(k["dx"] - dx), abs(k["dy"] - dy), abs(k["ds"] - dsc)) < TOL_OFFSET, "detect",
                  f"level {li} {pos}: offsets {(k['dx'], k['dy'], k['ds'])} model {(dx, dy, dsc)}")
    _need(len(raw) == sum(len(raw[raw["level_index"] == li]) for li in range(len(expect))), "detect", "level index out of range")
    st["detections"] = len(raw)

    # ---- orientation per raw item, from the session's gradient planes
    keys, desc = session.fetch(bi)
    groups = []                                   # runs of equal (level, x, y, s): the orientations of one location
    for i, k in enumerate(keys):
        ident = (int(k["level"]), float(k["x"]), float(k["y"]), float(k["s"]))
        if groups and groups[-1][0] == ident:
            groups[-1][1].append(i)
        else:
            groups.append((ident, [i]))
    items = []
    for rk in raw:
        li = int(rk["level_index"])
        oc, l = li // dog, li % dog + 1
        x, y, s = m.key_geometry(l, int(rk["row"]), int(rk["col"]), float(rk["dx"]), float(rk["dy"]), float(rk["ds"]))
        info = {}
        angles, unc = m.rotations(GOT[oc][l][..., 0], GOT[oc][l][..., 1], x, y, s, info=info)
        items.append((li, oc, l, x, y, s, angles, unc, rk))
        st["orient_uncertain"] += int(unc)
        st["three_peaks"] += int(info.get("peaks", 0) >= 3)
    multi = [0] * len(expect)
    for it in items:
        multi[it[0]] += len(it[6])
    kept2 = m.reduce_second(multi) if reducing else multi
    if reducing and m.method != R.TRUNC_TOPK:
        _need(st["orient_uncertain"] == 0, "orient", "an uncertain orientation count in a case that truncates on the counts")
    items = [it for it in items if kept2[it[0]] > 0 and (it[6] or it[7])]
    _need(len(groups) == len(items), "orient", lambda: f"{len(groups)} locations among the features, model {len(items)} "
                                                       f"(features per level {np.bincount(keys['level'], minlength=len(multi)).tolist()}, model {kept2})")
    off = 0.0 if m.lowe_origin else 0.5
    # the quantum of the session's mode, whatever the model believes: 16-bit angles where the two-peak branch ran
    quantum = QUANTUM_16 if is_dog and not m.single and not m.fixed_orientation else QUANTUM
    todo = []
    for (ident, idx), (li, oc, l, x, y, s, angles, unc, rk) in zip(groups, items):
        sc = scales[oc]
        ex, ey, es = m.export(x, y, s, sc)
        k0 = keys[idx[0]]
        _need(ident[0] == li, "orient", f"feature {idx[0]}: level {ident[0]}, raw list {li}")
        _need(abs(k0["x"] - ex) <= sc / 1024 * 1.01 + 1e-6 * abs(ex) and abs(k0["y"] - ey) <= sc / 1024 * 1.01 + 1e-6 * abs(ey),
              "export", f"feature {idx[0]} level {li}: position {(k0['x'], k0['y'])}, model {(ex, ey)}")
        _need(abs(k0["s"] - es) <= sc / 256 * 1.01, "export", f"feature {idx[0]}: scale {k0['s']}, model {es}")
        _need(int(k0["type"]) == int(rk["packed"]) & 3 and float(k0["response"]) == _half(rk["packed"]), "export",
              f"feature {idx[0]}: type / response differ from the raw list")
        _need(len(idx) == len(angles) or unc, "orient", f"location {(li, int(rk['row']), int(rk['col']))}: {len(idx)} orientations, "
                                                        f"model {len(angles)}")
        if len(idx) == len(angles):
            for j, a in zip(idx, angles):
                d = _circ(float(keys[j]["o"]), m.mirrored(a))
                if not unc:
                    st["angle"] = max(st["angle"], d - quantum)
                _need(d <= quantum + TOL_ANGLE or unc, "orient", f"feature {j} level {li}: orientation {keys[j]['o']}, model {m.mirrored(a)}")
        for j in idx:
            todo.append((j, oc, l, sc))
    st["features"] = len(keys)

    # ---- descriptors: a sample, at the session's own key
    if desc.size:
        clipped = [t for t in todo if _clipped(keys[t[0]], t[3], m.dwf, geo[t[1]], off)]
        pick = {t[0]: t for t in clipped[:: max(1, len(clipped) // 10)][:10]}
        for t in todo[:: max(1, len(todo) // (MAX_DESC - len(pick)))]:
            if len(pick) < MAX_DESC:
                pick.setdefault(t[0], t)
        for j, oc, l, sc in pick.values():
            k = keys[j]
            ang = (2 * R.PI - float(k["o"])) % (2 * R.PI)
            d = m.descriptor(GOT[oc][l][..., 0], GOT[oc][l][..., 1], (float(k["x"]) - off) / sc + 0.5, (float(k["y"]) - off) / sc + 0.5,
                             float(k["s"]) / sc, ang)
            dev = float(np.abs(d - desc[j]).max())
            st["desc"] = max(st["desc"], dev)
            _need(dev < tol_desc, "descriptor", f"feature {j} level {int(k['level'])}: max |d| {dev:.3g}")
        st["descriptors"] = len(pick)
        st["clipped"] = len([j for j in pick if any(j == t[0] for t in clipped)])
    return st


def check_statistics(st, case):
    """What both callers ask of check_against_model's statistics: the case is not empty, and the items at which either
    answer passed -- detection and orientation decisions together -- are at most 1 % of the candidates that pass the exact
    neighbour comparisons.  A keypoint list has no candidates: no orientation may be flagged there."""
    assert st["features"] >= case.min_features, "the case is empty: it would prove nothing"
    if case.keys is not None:
        assert st["orient_uncertain"] == 0, st
        return
    assert st["detections"] >= 8, st
    assert st["uncertain"] + st["orient_uncertain"] <= MAX_UNCERTAIN_SHARE * st["candidates"], st
    assert st["descriptors"] >= min(30, st["features"]) and st["clipped"] >= 5, st
    # the two-strongest rule is exercised only where three or more peaks qualify
    assert st["three_peaks"] >= case.min_three_peaks, st


def _clipped(k, sc, dwf, geo, off):
    """The descriptor's footprint (half-diagonal 2 sqrt(2) x window) leaves the octave's plane."""
    x, y, r = (float(k["x"]) - off) / sc + 0.5, (float(k["y"]) - off) / sc + 0.5, 2 * math.sqrt(2) * dwf * float(k["s"]) / sc
    return x - r < 1.5 or y - r < 1.5 or x + r > geo[0] - 1.5 or y + r > geo[1] - 1.5


def _check_keypoint_list(session, case, m, GOT, scales, st, tol_desc=TOL_DESC):
    """RunSIFT(num, keys, flag) on the current image: level binning, fixed-point position and scale, the strongest
    orientation only or the caller's own, descriptors -- all of it shows in the descriptor (which level's planes, where, at
    which angle) and, without given orientations, in the returned angle."""
    keys = case.keys
    n = session.run_keypoints(keys, case.have_orientation)
    _need(n == len(keys), "keylist", f"{n} features for {len(keys)} keys")
    out, desc = session.fetch(0)          # (a keypoint list runs on one image: no case has both keys and batch_at)
    # -m 1 and -ofix download the list again after the orientation pass (SiftPyramid.cpp:165-172): position and scale come
    # back through the fixed-point record, with the level; otherwise the caller's keys are returned as they came and only
    # the descriptor shows the orientation that was found
    downloaded = not case.have_orientation and (m.single or m.fixed_orientation)
    worst = 0.0
    for i, k in enumerate(keys):
        hits = m.bin_key(k["s"], scales)
        # a defect of the case, not of the session: no Mismatch, so that no wrong-rule test can be satisfied by it
        assert len(hits) == 1, f"key {i} (scale {k['s']}) is on {len(hits)} levels in the model: choose another scale"
        oc, l = hits[0] // m.dog, hits[0] % m.dog + 1
        sc = scales[oc]
        fx, fy, fs = m.user_key(float(k["x"]), float(k["y"]), float(k["s"]), sc)
        grad, theta = GOT[oc][l][..., 0], GOT[oc][l][..., 1]
        unc = False
        if case.have_orientation:
            ang = math.fmod(2 * R.PI - float(k["o"]), 2 * R.PI)
        else:
            (ang,), unc = m.rotations(grad, theta, fx, fy, fs, user=True)
            st["orient_uncertain"] += int(unc)
        if downloaded:
            ex, ey, es = m.export(fx, fy, fs, sc)
            _need(int(out[i]["level"]) == hits[0], "keylist", f"key {i} (scale {k['s']}): level {out[i]['level']}, model {hits[0]}")
            _need(max(abs(out[i]["x"] - ex), abs(out[i]["y"] - ey)) <= 1e-6 * (1 + abs(ex) + abs(ey)) and abs(out[i]["s"] - es) <= 1e-6 * es,
                  "keylist", f"key {i}: {(out[i]['x'], out[i]['y'], out[i]['s'])}, model {(ex, ey, es)}")
            d = _circ(float(out[i]["o"]), m.mirrored(ang))
            if math.isnan(ang):           # the all-zero histogram: NaN on both sides
                d = 0.0 if math.isnan(float(out[i]["o"])) else math.inf
            _need(d <= QUANTUM + TOL_ANGLE or unc, "keylist", f"key {i} (level {hits[0]}): orientation {out[i]['o']}, model {m.mirrored(ang)}")
            ang = (2 * R.PI - float(out[i]["o"])) % (2 * R.PI)
        else:
            _need(out[i].tobytes() == k.tobytes(), "keylist", f"key {i}: the caller's key changed")
        if unc:
            continue                      # (two votes within rounding of each other: no strongest orientation)
        if fs == 0:
            continue                      # a scale below 1 / 512 of a pixel: the window is empty
        # (nothing under the window: every component 1 / sqrt(dim), np_restatement.descriptor_ex; a NaN on either side
        # fails the comparison)
        d = m.descriptor(grad, theta, fx, fy, fs, ang)
        st["empty_windows"] = st.get("empty_windows", 0) + int(float(np.ptp(d)) == 0.0)
        dev = float(np.abs(d - desc[i]).max())
        worst = max(worst, dev)
        _need(dev < tol_desc, "keylist", f"key {i} (level {hits[0]}, scale {k['s']}): descriptor max |d| {dev:.3g}")
    st["desc"] = worst
    st["features"] = st["descriptors"] = len(keys)
