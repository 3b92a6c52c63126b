"""Keypoint lists for whole batches (hess_set_keypoints_batch / hess_run_keypoints_batch / hess_key_list_order): the seeded
cases and a binary32 restatement of the level rule (a plain helper module, no tests in it).

The rule (PyramidCU::GenerateFeatureListTex, PyramidCU.cpp:566-603) in the order the reference evaluates it: for every
octave, for every level 1..dog,
    level_sigma = GetLevelSigma(level) * octave_sigma;  sigma_min = level_sigma / h;  sigma_max = level_sigma * h
with h = powf(2.0f, 0.5f / dog), all binary32, and key k is listed at the level when
    (s >= sigma_min && s < sigma_max) || (s < sigma_min, first level of all) || (s > sigma_max, last level of all)
-- s the key's scale, or min(s, o) / 12.0f for rectangles.  The list of an image is ordered by level index, then by input
index.  powf is the C library's (ctypes), so the table holds the numbers the host code of both the product and the oracle
forms; the comparisons are numpy float32 comparisons.

Cases, all on fixtures.synthetic_blobs(160, 120, i) (three octaves of three levels):
  A  four images with 0, 1, 67 and 333 keys (empty; one key; more than a wavefront; more than a 256-thread workgroup),
     scales log-uniform in 0.3 .. 80: every level index and both catch-alls
  B  one image, 200 keys of one scale, some of them exact repeats: the compaction's 64-key seams inside a single level
  C  two images: the float32 neighbours (0, +-1, +-2 ulp) of every level's sigma_max (image 0) and sigma_min (image 1,
     which also has a key whose scale is NaN): keys that are listed twice, or nowhere
  D  A as rectangles (rect_keys): min(width, height) / 12 takes A's scales
"""
import ctypes
import ctypes.util
import functools
import math

import numpy as np

import fixtures
from hessgpu_amd import _abi
from hessgpu_amd.session import rect_keys

WIDTH, HEIGHT = 160, 120
COUNTS_A = (0, 1, 67, 333)
F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(a, b):
    return F(_libm.powf(float(F(a)), float(F(b))))


@functools.lru_cache(maxsize=None)
def image(index):
    img = fixtures.synthetic_blobs(WIDTH, HEIGHT, index)
    img.setflags(write=False)
    return img


def images(n):
    return np.stack([image(i) for i in range(n)])


def octaves(width=WIDTH, height=HEIGHT):
    """PyramidCU.cpp:238-245 for the default octave_num."""
    return max(1, int(math.floor(math.log(min(width & ~3, height)) / math.log(2.0))) - 3)


def level_table(sigma0=1.6, dog=3, noct=None):
    """-> float32 arrays (sigma_min, sigma_max, octave_sigma) per level index octave * dog + (level - 1), first octave at the
    input's size, the Hessian detector's GetLevelSigma(level) = sigma0 * powf(2, level / dog) (SiftGPU.cpp:1422-1425)."""
    noct = octaves() if noct is None else noct
    half = powf(2.0, F(0.5) / F(dog))
    lo, hi, osig = [], [], []
    octave_sigma = F(1.0)
    for _ in range(noct):
        for level in range(1, dog + 1):
            level_sigma = F(F(sigma0) * powf(2.0, F(level) / F(dog))) * octave_sigma
            lo.append(F(level_sigma / half))
            hi.append(F(level_sigma * half))
            osig.append(octave_sigma)
        octave_sigma = F(octave_sigma * F(2.0))
    return np.array(lo, F), np.array(hi, F), np.array(osig, F)


def binned_scale(keys, flag):
    """The scale the rule looks at: s, or min(s, o) / 12.0f for rectangles (PyramidCU.cpp:598-599), binary32."""
    s = keys["s"].astype(F)
    if flag == _abi.KEYS_RECTANGLES:
        s = (np.where(keys["s"] < keys["o"], keys["s"], keys["o"]).astype(F) / F(12.0)).astype(F)
    return s


def membership(keys, flag, table=None):
    """-> bool [nlev, num]: key k is listed at level index l."""
    lo, hi, _ = table or level_table()
    s = binned_scale(keys, flag)[None, :]
    lo, hi = lo[:, None], hi[:, None]
    nlev = len(lo)
    first = (np.arange(nlev) == 0)[:, None]
    last = (np.arange(nlev) == nlev - 1)[:, None]
    with np.errstate(invalid="ignore"):
        return ((s >= lo) & (s < hi)) | ((s < lo) & first) | ((s > hi) & last)


def list_order(keys, flag, table=None):
    """-> int32 [list length]: list position -> input index, level index ascending, then input index ascending."""
    m = membership(keys, flag, table)
    return np.concatenate([np.flatnonzero(row) for row in m]).astype(np.int32) if m.size else np.zeros(0, np.int32)


def _keys(n):
    return np.zeros(n, dtype=_abi.KEYPOINT_DTYPE)


def _spread(rng, n, lo=0.3, hi=80.0):
    k = _keys(n)
    k["x"] = rng.uniform(2.0, WIDTH - 2.0, n).astype(F)
    k["y"] = rng.uniform(2.0, HEIGHT - 2.0, n).astype(F)
    k["s"] = np.exp(rng.uniform(math.log(lo), math.log(hi), n)).astype(F)
    k["o"] = rng.uniform(0.0, 2.0 * math.pi, n).astype(F)
    return k


@functools.lru_cache(maxsize=None)
def case_a():
    """-> tuple of four key arrays (COUNTS_A)."""
    rng = np.random.default_rng(20240)
    return tuple(_spread(rng, n) for n in COUNTS_A)


@functools.lru_cache(maxsize=None)
def case_b():
    """-> (keys,): 200 keys of scale 2.6 (level index 1), every fifth one an exact repeat of the key before it."""
    rng = np.random.default_rng(20241)
    k = _spread(rng, 200)
    k["s"] = F(2.6)
    k[4::5] = k[3::5]
    return (k,)


@functools.lru_cache(maxsize=None)
def case_c():
    """-> (keys of image 0, keys of image 1): the neighbours of every sigma_max, of every sigma_min (+ a NaN scale)."""
    rng = np.random.default_rng(20242)
    lo, hi, _ = level_table()
    out = []
    for bounds in (hi, lo):
        scales = []
        for v in bounds:
            below1 = np.nextafter(v, F(0.0))
            above1 = np.nextafter(v, F(np.inf))
            scales += [np.nextafter(below1, F(0.0)), below1, v, above1, np.nextafter(above1, F(np.inf))]
        k = _spread(rng, len(scales))
        k["s"] = np.array(scales, F)
        out.append(k)
    nan = _spread(rng, 1)
    nan["s"] = F(np.nan)
    out[1] = np.concatenate([out[1][:7], nan, out[1][7:]])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_d():
    """-> tuple of four rectangle key arrays: A's positions as corners, min(width, height) = 12 x A's scale."""
    rng = np.random.default_rng(20243)
    out = []
    for a in case_a():
        n = len(a)
        side = (a["s"].astype(F) * F(12.0)).astype(F)
        longer = (side * rng.uniform(1.0, 1.5, n).astype(F)).astype(F)
        tall = rng.uniform(size=n) < 0.5
        w, h = np.where(tall, side, longer), np.where(tall, longer, side)
        out.append(rect_keys(np.stack([a["x"] - 1.0, a["y"] - 1.0, w, h], axis=1) if n else np.zeros((0, 4), F)))
    return tuple(out)


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d}
