"""Rectangle descriptors (keys_have_orientation == -1, HESS_KEYS_RECTANGLES): an independent float64 model, the cases and
the one checker both callers use (a plain helper module, no tests in it).

The CPU oracle does not restate this mode, so the yardstick is the model below, written from the reference's lines
(SiftPyramid.cpp:345-354, PyramidCU.cpp:522, 591-666, ProgramCU.cu:1806-1948, 2105-2143) and from nothing of the kernel:

  level      np_restatement.DetectorModel.bin_key of min(s, o) / 12.0f                        (PyramidCU.cpp:598-599)
  record     corner and width through DetectorModel.user_key (14.10 and 8.8 fixed point, masked: a width of 256 level
             pixels wraps, a negative corner wraps to the far side of 16384 and the window is empty); the height is the
             binary32 quotient o / scale, not quantised                                         (PyramidCU.cpp:616-657)
  descriptor rect_descriptor_ex: 4 x 4 cells of sptx x spty = W/4 x H/4 from the corner, bilinear weight per axis, no
             Gaussian, no rotation, bins from -theta, its own normalisation                    (ProgramCU.cu:1849-1947)

check_rectangles(session, case) runs a case on any session that answers run / run_keypoints / set_keypoints / fetch /
geometry / level -- a product context (tests/test_rect_gpu.py) or ModelSession below, which answers from the model and
can be told to follow a WRONG rule (tests/test_rect_model.py shows that the checker notices each of them).  Every
rectangle's descriptor is computed from THE SESSION'S OWN gradient plane of the level the model bins it to and compared
with TOL_DESC; no rectangle is skipped: the rule is continuous in everything but the sample whose bin coordinate is 8.0.

Images come from seeds (detector_cases); nothing here reads a file.
"""
import math
from types import SimpleNamespace

import numpy as np

import detector_cases as dc
import np_restatement as R
from hessgpu_amd import _abi
from hessgpu_amd.session import rect_keys

RECT = _abi.KEYS_RECTANGLES
TOL_DESC = dc.TOL_DESC
MAX_CELL = 2048          # level pixels of a cell's box in every case: a binary32 sum of that many non-negative terms is
                         # within 2048 * 2^-24 = 1.2e-4 RELATIVE of the exact one in the worst association and ~ 1e-6 in
                         # any tree or pairwise one -- well inside TOL_DESC on a unit-norm descriptor
LENGTHS = (1, 2, 65, 300)

# the wrong rules ModelSession can follow (tests/test_rect_model.py: check_rectangles raises for each)
WRONG_RULES = {
    "corner taken as centre": "centre",
    "width and height swapped": "swapped",
    "level from s instead of min(s, o) / 12": "level_from_s",
    "height quantised to 8.8 like the width": "height_q8",
    "a Gaussian weight added": "gaussian",
    "the oriented descriptor at (x, y, s, o)": "oriented",
}


# ---- the model ----------------------------------------------------------------------------------------------------------
def _normalized(d):
    """NormalizeDescriptor_Kernel, ProgramCU.cu:1972-2054, restated here: unit length, min(0.2, .) by a min that returns
    the operand which is not NaN, unit length again.  The empty window (all zeros): 0 * rsqrt(0) = NaN, min(0.2, NaN) = 0.2,
    then 0.2 / sqrt(dim 0.04) = 1 / sqrt(dim) in every component."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.fmin(0.2, d * (1.0 / np.sqrt((d * d).sum())))
        return d / np.sqrt((d * d).sum())


def rect_descriptor_ex(grad, theta, X, Y, W, H, half=False, dynamic_indexing=False, normalize=True, gaussian=False,
                       info=None):
    """ComputeDescriptorRECT_Kernel, ProgramCU.cu:1806-1948, in float64.  (X, Y): the corner, W x H: the size, all in
    level pixels (pixel centres at integer + 0.5).  The binary32 value is asked for at one place only: a sample whose bin
    coordinate -theta 4/pi + 8 is 8.0 AS A binary32 NUMBER (:1889-1892) falls into no bin (:1905-1916), or into des[8]
    with dynamic_indexing (:1899-1903).  W == 0 or H == 0: nx or ny is infinite or NaN, `(nxn < 1.0f) && (nyn < 1.0f)`
    (:1882) is false for every sample: the empty window.  gaussian: the WRONG rule that keeps the oriented kernel's
    exp(-((nx + ix - 1.5)^2 + (ny + iy - 1.5)^2) / 8).  info: a dict that receives max_cell, the largest cell box."""
    h, w = grad.shape
    sptx, spty = W * 0.25, H * 0.25
    out = []
    biggest = 0
    for cell in range(16):
        ix, iy = cell & 3, cell >> 2
        cx, cy = sptx * (ix + 0.5) + X, spty * (iy + 0.5) + Y
        des = np.zeros(9)
        xmin, ymin = max(1.5, math.floor(cx - sptx) + 0.5), max(1.5, math.floor(cy - spty) + 0.5)
        xmax, ymax = min(w - 1.5, math.floor(cx + sptx) + 0.5), min(h - 1.5, math.floor(cy + spty) + 0.5)
        if sptx != 0 and spty != 0 and xmax >= xmin and ymax >= ymin:
            xs, ys = np.arange(xmin, xmax + 0.25), np.arange(ymin, ymax + 0.25)
            biggest = max(biggest, len(xs) * len(ys))
            nx, ny = ((xs - cx) / sptx)[None, :], ((ys - cy) / spty)[:, None]
            g = grad[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)]
            t = theta[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)]
            ok = (np.abs(nx) < 1) & (np.abs(ny) < 1)
            wgt = (1 - np.abs(nx)) * (1 - np.abs(ny)) * g
            if gaussian:
                wgt = wgt * np.exp(-0.125 * ((nx + ix - 1.5) ** 2 + (ny + iy - 1.5) ** 2))
            th = -t * 4.0 / R.PI
            th = np.where(th < 0, th + 8.0, th)
            t32 = (-t.astype(np.float32)) * np.float32(4.0 / R.PI)
            t32 = np.where(t32 < 0, t32 + np.float32(8.0), t32)
            th = np.where(t32 == np.float32(8.0), 8.0, th)
            fo = np.floor(th)
            ok = ok & (fo >= 0) & ((fo <= 8) if dynamic_indexing else (fo < 8))
            fo_i = fo.astype(int)[ok]
            np.add.at(des, fo_i, ((fo + 1 - th) * wgt)[ok])
            hi = fo_i + 1
            np.add.at(des, hi[hi <= 8], ((th - fo) * wgt)[ok][hi <= 8])
        des[0] += des[8]                                                              # :1920
        out.extend([des[k] + des[k + 4] for k in range(4)] if half else des[:8])      # :1923-1943
    if info is not None:
        info["max_cell"] = max(info.get("max_cell", 0), biggest)
    d = np.array(out)
    return _normalized(d) if normalize else d


def rect_sigma(k):
    """The scale that is binned, PyramidCU.cpp:598-599: min(s, o) / 12.0f, a binary32 quotient."""
    return float(np.float32(min(np.float32(k["s"]), np.float32(k["o"]))) / np.float32(12.0))


def rect_record(m, k, scale, wrong=None):
    """-> (X, Y, W, H) in level pixels as the record holds them (PyramidCU.cpp:616-657): corner and width through the fixed
    point of every caller key, the height o / scale as the binary32 number it is."""
    X, Y, W = m.user_key(float(k["x"]), float(k["y"]), float(k["s"]), scale)
    H = float(np.float32(k["o"]) / np.float32(scale))
    if wrong == "swapped":
        W, H = (R.fixed(float(k["o"]) / scale, 8) & 0xFFFF) / 256.0, float(np.float32(k["s"]) / np.float32(scale))
    if wrong == "height_q8":
        H = (R.fixed(H, 8) & 0xFFFF) / 256.0
    if wrong == "centre":
        X, Y = X - W / 2, Y - H / 2
    return X, Y, W, H


def model_descriptor(m, got, scales, k, wrong=None, info=None, strict=True):
    """-> (level index, descriptor) of one rectangle.  got(octave, level) -> the float64 (gradient, theta) plane [h, w, 2].
    strict: the key must fall on exactly one level in the model (a defect of the case otherwise, not of the session)."""
    if wrong == "oriented":          # what the code did before the mode existed: s a scale, o an angle
        hits = m.bin_key(float(k["s"]), scales)
        oc, l = hits[0] // m.dog, hits[0] % m.dog + 1
        plane = got(oc, l)
        fx, fy, fs = m.user_key(float(k["x"]), float(k["y"]), float(k["s"]), scales[oc])
        ang = math.fmod(2 * R.PI - float(k["o"]), 2 * R.PI)
        if fs == 0:
            d = np.zeros(64 if m.half else 128)
            return hits[0], _normalized(d) if m.normalize else d
        return hits[0], m.descriptor(plane[..., 0], plane[..., 1], fx, fy, fs, ang)
    hits = m.bin_key(float(k["s"]) if wrong == "level_from_s" else rect_sigma(k), scales)
    if strict:
        assert len(hits) == 1, f"rectangle {tuple(k)[:4]} is on {len(hits)} levels in the model: choose another size"
    oc, l = hits[0] // m.dog, hits[0] % m.dog + 1
    plane = got(oc, l)
    X, Y, W, H = rect_record(m, k, scales[oc], wrong)
    return hits[0], rect_descriptor_ex(plane[..., 0], plane[..., 1], X, Y, W, H, m.half, m.di, m.normalize,
                                       gaussian=wrong == "gaussian", info=info)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def rectangles(m, w, h, n, seed=11):
    """-> KEYPOINT_DTYPE array of n rectangles for a w x h image under the model's parameters: the named shapes first (at
    most 27 of them; lists shorter than that take the first n), seeded ones inside the bins after them."""
    _, _, geo, scales = m.plan(w, h)
    rng = np.random.RandomState(seed)
    last = len(scales) - 1

    def side(oc, l, f=1.0):
        """the smaller side whose twelfth is f x the sigma of level l of octave oc: inside that level's bin for 0.9 < f <
        1.1 (the bin reaches 2^(+-1/(2 dog)) = +-12 % at dog = 3)"""
        return 12.0 * m.level_sigma(l) * scales[oc] * f

    a1, a2, a3 = side(0, 1), side(0, 2), side(0, m.dog)
    out = []
    # a square in every level's bin of every octave, one below the first level, one above the last
    for oc in range(len(scales)):
        for l in range(1, m.dog + 1):
            a = side(oc, l, 0.95 + 0.1 * rng.rand())
            out.append((rng.uniform(0.5, max(1.0, w - a)), rng.uniform(0.5, max(1.0, h - a)), a, a))
    out.append((w * 0.3, h * 0.4, a1 * 0.5, a1 * 0.5))
    out.append((w * 0.1, h * 0.1, side(last, m.dog, 2.0), side(last, m.dog, 2.0)))
    # 5 : 1 and 1 : 5
    out.append((w * 0.05, h * 0.3, 5 * a2, a2))
    out.append((w * 0.4, h * 0.02, a2, 5 * a2))
    # boxes (1.25 W) wider than 64 and than 128 level pixels of octave 0, W < 256: the seams of the 64-column bands
    out.append((3.0 * scales[0], h * 0.2, 60.0 * scales[0], a3))
    out.append((4.5 * scales[0], h * 0.45, 110.0 * scales[0], a3))
    # over the left, the top, the right and the bottom border (a negative corner would wrap: the corners stay inside)
    out.append((0.3 * scales[0], h * 0.4, a2, a2 * 1.3))
    out.append((w * 0.4, 0.2 * scales[0], a2 * 1.2, a2))
    out.append((w - a2 * 0.5, h * 0.3, a2, a2))
    # ... the bottom one 260 level pixels tall: a height that does not fit 8.8 fixed point and is not meant to
    out.append((w * 0.3, h * 0.5, a1, 260.0 * scales[0]))
    # wholly outside; a negative corner (wraps); narrower than 1/512 level pixel; height 0; W >= 256 level pixels (wraps)
    out.append((w + 50.0, h + 40.0, a2, a2))
    out.append((-7.0, h * 0.2, a2, a2))
    out.append((w * 0.5, h * 0.5, scales[0] / 1024.0, a2))
    out.append((w * 0.5, h * 0.5, a2, 0.0))
    out.append((2.0 * scales[0], h * 0.3, 300.0 * scales[0], a3))
    assert len(out) <= 27 + 3 * max(0, len(scales) - 4)
    # seeded rectangles inside the bins, aspect up to 2.5 either way
    while len(out) < n:
        oc, l = rng.randint(0, len(scales)), rng.randint(1, m.dog + 1)
        a, asp = side(oc, l, 0.93 + 0.14 * rng.rand()), 1.0 + 1.5 * rng.rand()
        s, o = (a * asp, a) if rng.rand() < 0.5 else (a, a * asp)
        out.append((rng.uniform(0.0, w * 0.8), rng.uniform(0.0, h * 0.8), s, o))
    return rect_keys(np.array(out[:n], dtype=np.float64))


def _images():
    return {"blobs": dc.blobs_noise(), "grid": dc.dot_grid(),
            # float luminance is taken as it is: values up to 255, not 1
            "blobs float": dc.blobs_noise().astype(np.float32)}


def cases(params=None, image_of_length=None):
    """-> [case] for one parameter set (a dict of hess_params overrides): the lists of LENGTHS, 1 / 2 / 65 on blobs_noise
    96 x 80 and 300 on dot_grid 160 x 120 (wide enough for a box of more than 128 level pixels).  image_of_length: another
    assignment, e.g. {65: "blobs float"}."""
    m = R.DetectorModel(dict(params or {}))
    imgs = _images()
    which = {1: "blobs", 2: "blobs", 65: "blobs", 300: "grid"}
    which.update(image_of_length or {})
    out = []
    for n in LENGTHS:
        img = imgs[which[n]]
        h, w = img.shape[:2]
        out.append(SimpleNamespace(name=f"{which[n]} x {n}", image=img, fmt=None, keys=rectangles(m, w, h, n)))
    return out


# ---- the checker --------------------------------------------------------------------------------------------------------
def run_case(session, case, entry="run_keypoints"):
    """The case through one of the two entries -> number of features reported.  run_keypoints: the image, then the list on
    the current image (pyramid reused); set_keypoints: the list for the next image, then the image (pyramid built)."""
    stack = np.asarray(case.image)[None]
    if entry == "set_keypoints":
        session.set_keypoints(case.keys, RECT)
        return session.run(stack, fmt=case.fmt)[0]
    session.run(stack, fmt=case.fmt)
    return session.run_keypoints(case.keys, RECT)


def check_rectangles(session, case, entry="run_keypoints"):
    """Run `case` on `session` with flag -1 and compare every rectangle with the model.  -> statistics: rectangles, worst
    (largest deviation relative to the bound's scale), empty windows, levels hit, largest cell.  Raises dc.Mismatch."""
    m = R.DetectorModel(session.params)
    img = np.asarray(case.image)
    h, w = img.shape[:2]
    keys = case.keys
    n = run_case(session, case, entry)
    dc._need(n == len(keys), "rect", f"{n} features for {len(keys)} rectangles")
    out, desc = session.fetch(0)
    dc._need(out.tobytes() == keys.tobytes(), "rect", "the caller's keys changed")
    _, _, geo, scales = m.plan(w, h)
    dc._need(session.geometry() == geo, "geometry", lambda: f"{session.geometry()} != {geo}")
    dim = 64 if m.half else 128
    dc._need(desc.shape == (len(keys), dim) and desc.dtype == np.float32, "rect", f"descriptors {desc.shape} {desc.dtype}")
    planes = {}

    def got(oc, l):
        if (oc, l) not in planes:
            planes[oc, l] = session.level(0, oc, l, _abi.DBG_GOT).astype(np.float64)
        return planes[oc, l]

    st = dict(rectangles=len(keys), worst=0.0, empty=0, levels=set(), max_cell=0)
    for i, k in enumerate(keys):
        level, d = model_descriptor(m, got, scales, k, info=st)
        st["levels"].add(level)
        st["empty"] += int(float(np.ptp(d)) == 0.0)
        tol = TOL_DESC * (1.0 if m.normalize else max(1.0, float(np.sqrt((d * d).sum()))))
        dev = float(np.abs(d - desc[i]).max())        # (a NaN on either side fails the comparison)
        st["worst"] = max(st["worst"], dev / tol * TOL_DESC) if dev == dev else math.inf
        dc._need(dev < tol, "rect", f"rectangle {i} {tuple(float(v) for v in tuple(k)[:4])} (level {level}): "
                                    f"descriptor max |d| {dev:.3g}, bound {tol:.3g}")
    assert st["max_cell"] <= MAX_CELL, f"a cell of {st['max_cell']} level pixels: the case is outside the bound's reasoning"
    return st


# ---- a session that answers from the model ------------------------------------------------------------------------------
class ModelSession:
    """run / set_keypoints / run_keypoints / fetch / geometry / level answered by the model itself: the pyramid by
    np_restatement (Gaussian levels, gradient planes, stored as binary32 like a context's), the descriptors by
    model_descriptor -- under the right rules, or under one of WRONG_RULES' values."""

    def __init__(self, wrong=None, **params):
        assert wrong is None or wrong in WRONG_RULES.values(), wrong
        self.params = dict(params)
        self.wrong = wrong
        self._pending = None
        self._result = None

    def run(self, stack, fmt=None):
        img = np.asarray(stack)[0]
        m = self._m = R.DetectorModel(self.params)
        _, _, self._geo, self._scales = m.plan(img.shape[1], img.shape[0])
        base, taps0 = m.base_plane(img, fmt)
        g = base if taps0 is None else R.gaussian(base, taps0)
        self._got = {}
        for oc, (wa, hh) in enumerate(self._geo):
            if oc:
                g = R.downsample(below, wa, hh)
            for l in range(1, m.dog + 1):
                g = R.gaussian(g, m.level_taps(l))
                _, grad, theta = m.planes(g, l)
                self._got[oc, l] = np.stack([grad, theta], axis=-1).astype(np.float32)
                if l == m.level_ds:
                    below = g
        self._result = None
        if self._pending is not None:
            keys, self._pending = self._pending, None
            return [self.run_keypoints(keys, RECT)]
        return [0]

    def set_keypoints(self, keys, have_orientation=True):
        assert have_orientation == RECT
        self._pending = np.array(keys, dtype=_abi.KEYPOINT_DTYPE)

    def run_keypoints(self, keys, have_orientation=True):
        assert have_orientation == RECT
        keys = np.array(keys, dtype=_abi.KEYPOINT_DTYPE)
        got = lambda oc, l: self._got[oc, l].astype(np.float64)
        desc = [model_descriptor(self._m, got, self._scales, k, self.wrong, strict=False)[1] for k in keys]
        self._result = keys, np.array(desc, dtype=np.float32)
        return len(keys)

    def fetch(self, img=0):
        return self._result

    def geometry(self):
        return list(self._geo)

    def level(self, img, octave, level, what):
        assert what == _abi.DBG_GOT
        return self._got[octave, level].copy()
