"""Float pixels of any range: inputs for tests/test_float_range.py (the CPU oracle) and tests/test_float_range_gpu.py (the
HIP path).  A plain helper module, no tests in it; the images come from detector_cases, whose `_case` and checker are used.

Float pixels (HESS_PIX_F32, the SiftGPU class's GL_FLOAT) are taken as they are: no scale, no clamp.  Callers hand in
luminance in 0 .. 255, in 0 .. 65535 and zero-mean.  Such an image goes through convert_kernel (never gauss_first_kernel) and
the INTERLEAVED descriptor_kernel (never the pixel raster), and its range reaches places that 8- and 16-bit pixels cannot:

  homogeneity   Every stage is homogeneous in the pixels: for A a power of two (no rounding differs) the Gaussian planes and
                the gradient of A B are A times those of B, det-H A^2 times (the DoG response A times), theta, the offsets,
                the keypoints and the normalised descriptors are the same BITS, provided the threshold is scaled alike.  That
                needs no oracle and no tolerance (pairs()).
  the half      The list record packs the response as binary16.  It is inf from about A = 2^12 on (every top-K key
                0x7c00), a subnormal half at 2^-8 and 0 from 2^-11 down (every key 0): the top-K cut is then decided by the
                tie rule alone, first come first kept (list_cases()).
  the pivots    The sub-pixel solve guards its pivots with an ABSOLUTE 1e-10 (np_restatement.key_test_ex).  From A = 2^-14
                down no candidate has such a pivot: "no solution", offsets 0, none of the tests on the refined values, and
                more detections than the solved branch gives.  2^-12 and 2^-13, where pivots lie AT the guard, are avoided.

Every case has the prefix `float:`, its threshold (dog_threshold of the [0, 1] image times A^2, times A with detector = 1,
as binary32 products) and, in `why`, the property it is there for.  `amp` is the amplitude the checker's absolute gates take
(detector_cases.check_against_model), `exp` its binary logarithm where it is a power of two.
"""
import functools

import numpy as np

import detector_cases as dc
import list_cases as L
from hessgpu_amd import _abi

T_DEFAULT = np.float32(0.02) / np.float32(3)       # ParseSiftParam's dog_threshold at dog_level_num 3
SOLVED, UNSOLVED = "solved", "no solution"
EXPONENTS = (8, 10, 16, -8, -11, -14, -20)
# what becomes of half(r') at each power of two, for responses of ordinary contrast (0.007 .. 0.03 on [0, 1])
HALF = {0: "normal", 8: "normal", 10: "normal", 16: "inf", -8: "subnormal", -11: "zero", -14: "zero", -20: "zero"}


def unit(img):
    """u8 -> float32 in [0, 1], the image every other float case is a multiple of."""
    return (np.asarray(img) / 255.0).astype(np.float32)


def times(b, a):
    return (b * np.float32(a)).astype(np.float32)


def threshold(t0, a, dog=False):
    a = np.float32(a)
    return float(np.float32(t0) * a) if dog else float(np.float32(t0) * a * a)


def _tag(e):
    return f"2^{e}"


def _add(out, name, image, amp, why, t0=T_DEFAULT, exp=None, base=None, **kw):
    isdog = kw.get("detector") == _abi.DETECTOR_DOG
    case_kw = {k: kw.pop(k) for k in ("fmt", "keys", "have_orientation", "batch_at", "stack", "min_features") if k in kw}
    c = dc._case("float: " + name, image, dog_threshold=threshold(t0, amp, isdog), **case_kw, **kw)
    c.amp, c.why, c.exp = float(amp), why, exp
    c.side = UNSOLVED if amp <= 2.0 ** -14 else SOLVED
    c.base = None if base is None else "float: " + base      # the case it is an exact multiple of (pairs())
    out.append(c)
    return c


# hess_params overrides of the variants, on blobs_noise at 2^8 and 2^-14
VARIANTS = {
    "dog": dc.DOG,
    "first_octave -1": dict(first_octave=-1),
    "first_octave 1": dict(first_octave=1),
    "subpixel 0": dict(subpixel=0),
    "normalize 0": dict(normalize=0),
    "half_sift": dict(half_sift=1),
    "dynamic_indexing": dict(dynamic_indexing=1),
}
VARIANT_EXPONENTS = (8, -14)
# first_octave 1 decimates to a quarter of the pixels: the larger blobs image, and a threshold that leaves 50 candidates
DECIMATED = dict(w=160, h=120, t0=np.float32(0.002))
# the DoG mode has few extrema on the blobs at its default threshold (detector_cases._dog_cases): a lower one
DOG_T0 = np.float32(0.002)


@functools.lru_cache(maxsize=None)
def cases():
    """-> {name: case}, pixel cases and keypoint lists; every one runs through detector_cases.check_against_model."""
    out = []
    b = unit(dc.blobs_noise())
    n = unit(dc.noise(260, 49))
    c = unit(dc.colour(96, 80))
    nk = dict(t0=dc.NOISE_KW["dog_threshold"], edge_threshold=dc.NOISE_KW["edge_threshold"])
    ck = dict(t0=dc.COLOUR_KW["dog_threshold"], edge_threshold=dc.COLOUR_KW["edge_threshold"])

    # ---- the unit images: what the multiples are compared with
    _add(out, "blobs 1", b, 1.0, "the unit image", exp=0)
    _add(out, "noise 260x49 1", n, 1.0, "the unit image", exp=0, **nk)
    _add(out, "rgb 1", c, 1.0, "the unit image", exp=0, **ck)
    _add(out, "bgr 1", np.ascontiguousarray(c[..., ::-1]), 1.0, "the unit image", exp=0, fmt=_abi.FMT_BGR, **ck)

    # ---- powers of two: exact multiples
    why = {8: "0 .. 256: homogeneity, normal halves", 10: "the largest halves short of inf", 16: "0 .. 65536: every half inf",
           -8: "subnormal halves", -11: "still solved, every half 0", -14: "every pivot below 1e-10: no solution",
           -20: "no solution, det-H near 1e-15"}
    for e in EXPONENTS:
        base = "blobs 2^-14" if e == -20 else "blobs 1"
        _add(out, f"blobs {_tag(e)}", times(b, 2.0 ** e), 2.0 ** e, why[e], exp=e, base=base)
    for e in (8, 16, -14):
        _add(out, f"noise 260x49 {_tag(e)}", times(n, 2.0 ** e), 2.0 ** e, why[e] + "; two octaves of a wide plane", exp=e,
             base="noise 260x49 1" if e != -14 else None, **nk)
    for e in (8, -14):
        _add(out, f"rgb {_tag(e)}", times(c, 2.0 ** e), 2.0 ** e, why[e] + "; the float luminance sum", exp=e,
             base="rgb 1" if e == 8 else None, **ck)
    _add(out, "bgr 2^16", times(np.ascontiguousarray(c[..., ::-1]), 2.0 ** 16), 2.0 ** 16, why[16] + "; the float luminance sum, BGR",
         exp=16, base="bgr 1", fmt=_abi.FMT_BGR, **ck)

    # ---- the caller's ranges: not exact multiples, the model alone judges them
    for a in (255.0, 65535.0):
        _add(out, f"blobs {a:g}", times(b, a), a, f"0 .. {a:g} as callers have it")
    _add(out, "noise 260x49 65535", times(n, 65535.0), 65535.0, "0 .. 65535, every half inf", **nk)
    _add(out, "rgb 255", times(c, 255.0), 255.0, "0 .. 255 RGB", **ck)
    _add(out, "bgr 65535", times(np.ascontiguousarray(c[..., ::-1]), 65535.0), 65535.0, "0 .. 65535 BGR", fmt=_abi.FMT_BGR, **ck)
    _add(out, "blobs - 0.5", (b - np.float32(0.5)).astype(np.float32), 1.0, "zero-mean: negative luminance")
    # det-H is even in the sign of the plane: the same detections and responses; dark and bright change places, and every
    # gradient turns by pi
    _add(out, "blobs negated", -b, 1.0, "the negative image: types mirrored, orientations turned by pi")

    # ---- the variants, on both sides of the pivot guard
    keys = dc._user_keys(96, 80)
    for e in VARIANT_EXPONENTS:
        a, img = 2.0 ** e, times(b, 2.0 ** e)
        for name, kw in VARIANTS.items():
            kw = dict(kw)
            image, t0 = img, T_DEFAULT
            if name == "dog":
                t0 = DOG_T0
            if name == "first_octave 1":
                image = times(unit(dc.blobs_noise(DECIMATED["w"], DECIMATED["h"])), a)
                t0 = DECIMATED["t0"]
            _add(out, f"blobs {_tag(e)} {name}", image, a, f"{name} at {_tag(e)}", t0=t0, exp=e, **kw)
        for ho in (1, 0):
            _add(out, f"blobs {_tag(e)} keypoint list orient={ho}", img, a, f"a caller's keypoints at {_tag(e)}", exp=e, keys=keys,
                 have_orientation=ho)

    # ---- one batch, one threshold: the unit image, 2^16 and 2^-14 times it
    stack = np.stack([b, times(b, 2.0 ** 16), times(b, 2.0 ** -14)])
    for i, (a, what) in enumerate(((1.0, "the unit image"), (2.0 ** 16, "every extremum passes, every half inf"))):
        _add(out, f"batch of three, image {i}", stack[i], a, f"in a batch under the unit threshold: {what}", t0=T_DEFAULT / np.float32(a * a),
             batch_at=(3, i), stack=stack)
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


BATCH_THRESHOLD = float(T_DEFAULT)
# features per image of the batch under BATCH_THRESHOLD, from the oracle (tests/test_float_range.py asserts them): at 2^16
# every extremum that passes the edge test is kept, at 2^-14 no response reaches the threshold
BATCH_FEATURES = [80, 138, 0]


def batch_stack():
    return cases()["float: batch of three, image 0"].stack


# ---- homogeneity -----------------------------------------------------------------------------------------------------------
def _unit_of(c, k):
    """The case c with its pixels and its threshold divided by 2^k (by the same binary32 products): made on the spot."""
    kw = dict(c.kw)
    isdog = kw.get("detector") == _abi.DETECTOR_DOG
    kw["dog_threshold"] = float(np.float32(kw["dog_threshold"]) * np.float32(2.0 ** (-k if isdog else -2 * k)))
    u = dc._case(f"{c.name} / 2^{k}", times(c.image, 2.0 ** -k), fmt=c.fmt, keys=c.keys, have_orientation=c.have_orientation, **kw)
    u.amp, u.exp = c.amp * 2.0 ** -k, c.exp - k
    return u


def pairs():
    """-> {name: (case A b, case b, k, the lists agree)}: A = 2^k.  Every dense stage of the first is an exact multiple of the
    second's.  Where both lie on one side of the pivot guard the lists, the keypoints and the descriptors are the same bits
    too; at 2^-11 most pivots are above 1e-10 and a few below, so only the planes are claimed there, and 2^-14 and 2^-20,
    beyond the guard, are held against each other.  The variants at 2^8 are held against the unit image with the same
    parameters."""
    out = {}
    for name, c in cases().items():
        if getattr(c, "base", None) is not None:
            b = cases()[c.base]
            out[name] = (c, b, c.exp - b.exp, c.exp != -11 and c.side == b.side)
    for v in list(VARIANTS) + ["keypoint list orient=1", "keypoint list orient=0"]:
        c = cases()[f"float: blobs 2^8 {v}"]
        out[c.name] = (c, _unit_of(c, 8), 8, True)
        c = cases()[f"float: blobs 2^-14 {v}"]                    # beyond the guard: against 2^-20 with the same parameters
        out[c.name] = (c, _unit_of(c, 6), 6, True)
    return out


def half_regime(case):
    """What half(r') is for every response of the case (HALF; the DoG response grows with A, not with A^2)."""
    if case.kw.get("detector") == _abi.DETECTOR_DOG:
        return {0: "normal", 8: "normal", -14: "subnormal", -20: "tiny"}[case.exp]
    return HALF[case.exp]


def snapshot(session, case):
    """Run the case with every level kept -> its planes, raw list, keypoints and descriptors."""
    session.keep_levels(True)
    stack, bi = dc.case_input(case)
    session.run(stack, fmt=case.fmt)
    geo = session.geometry()
    dog = int(session.params.dog_level_num) or 3
    isdog = int(session.params.detector) == _abi.DETECTOR_DOG
    nlev = dog + 2 + int(isdog)
    s = dict(geometry=geo, isdog=isdog, normalize=bool(session.params.normalize))
    s["gauss"] = [session.level(bi, oc, l, _abi.DBG_GAUSS) for oc in range(len(geo)) for l in range(nlev)]
    s["resp"] = [session.level(bi, oc, l, _abi.DBG_DETH) for oc in range(len(geo)) for l in range(int(isdog), nlev)]
    got = [session.level(bi, oc, l, _abi.DBG_GOT) for oc in range(len(geo)) for l in range(1, dog + 1)]
    s["grad"], s["theta"] = [g[..., 0].copy() for g in got], [g[..., 1].copy() for g in got]
    s["raw"] = session.rawlist(bi) if case.keys is None else None
    if case.keys is not None:
        session.run_keypoints(case.keys, case.have_orientation)
        bi = 0
    s["keys"], s["desc"] = session.fetch(bi)
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _normal_half(v):
    v = np.abs(v.astype(np.float64))
    return (v >= 2.0 ** -14) & (v <= 65504.0)


def check_homogeneous(a, b, k, lists=True, half_a="normal", half_b="normal"):
    """a, b: snapshots of A b and b, A = 2^k.  No tolerance: a multiplication by a power of two is exact in binary32 (no value
    here is subnormal or overflows), so every bit of `a` follows from `b`.  half_a, half_b: what the response halves of either
    side are (HALF); the one relation that is not exact is a subnormal half, bounded by half its step."""
    A = np.float32(2.0 ** k)
    R = A if a["isdog"] else A * A
    assert a["geometry"] == b["geometry"]
    for what, f in (("gauss", A), ("resp", R), ("grad", A), ("theta", np.float32(1.0))):
        assert len(a[what]) == len(b[what])
        for i, (pa, pb) in enumerate(zip(a[what], b[what])):
            bad = int((_bits(pa) != _bits(pb * f)).sum())
            assert bad == 0, f"{what} plane {i}: {bad} values are not {float(f)!r} times the other image's"
    if not lists:
        return
    if a["raw"] is not None:
        ra, rb = a["raw"], b["raw"]
        assert len(ra) == len(rb) > 0, (len(ra), len(rb))
        for f in ("level_index", "row", "col", "dx", "dy", "ds"):
            assert ra[f].tobytes() == rb[f].tobytes(), f"raw list: {f} differs"
        assert np.array_equal(ra["packed"] & 0xffff, rb["packed"] & 0xffff), "raw list: type bits differ"
    ka, kb = a["keys"], b["keys"]
    assert len(ka) == len(kb) > 0, (len(ka), len(kb))
    for f in ("x", "y", "s", "o", "level", "type"):
        assert ka[f].tobytes() == kb[f].tobytes(), f"keypoints: {f} differs"
    if a["raw"] is not None:
        va, vb = ka["response"], kb["response"]
        both = _normal_half(va) & _normal_half(vb)
        assert np.array_equal(va[both], vb[both] * R), "response: a normal half is not the multiple of the other side's"
        for v, regime in ((va, half_a), (vb, half_b)):
            if regime == "normal":
                assert _normal_half(v).all(), "a response is no normal half"
            elif regime == "inf":
                assert np.isinf(v).all(), "a response is finite where every half overflows"
            elif regime == "zero":
                assert not v.any(), "a response is not 0 where every half underflows"
            else:                                              # subnormal; tiny: subnormal or 0
                assert (np.abs(v) < 2.0 ** -14).all() and (v.any() or regime == "tiny"), "the responses are not subnormal halves"
        if half_a == "subnormal" and half_b == "normal":
            # half(r' A^2) against half(r') A^2: half a subnormal step, and the rounding of the normal half carried along
            err = np.abs(va.astype(np.float64) - vb.astype(np.float64) * float(R))
            assert (err <= 2.0 ** -25 + 2.0 ** -11 * np.abs(va)).all(), float(err.max())
    da, db = a["desc"], b["desc"]
    assert da.shape == db.shape and da.size
    f = np.float32(1.0) if a["normalize"] else A
    bad = int((_bits(da) != _bits(db * f)).sum())
    assert bad == 0, f"descriptors: {bad} components are not {float(f)!r} times the other image's"


# ---- lists: every top-K key equal ----------------------------------------------------------------------------------------
GRID_T0 = dc.GRID_KW["dog_threshold"]


def _grid(e):
    return lambda: times(unit(dc.dot_grid()), 2.0 ** e)[None]


def _half_the_list(model, raw, counts):
    return dict(truncate_method=L.T["topk"], feature_count_threshold=len(raw) // 2)


def list_cases():
    """-> {name: list_cases.Case} on the dot grid (805 features on [0, 1]): top-K at half the list where every key is 0x7c00
    (2^16) and where every key is 0 (2^-11); one level-truncation rule at a threshold inside a level (detector_cases.
    GRID_THRESHOLD: the first pass keeps level 1, the second drops it)."""
    out = {}
    for e, key in ((16, 0x7c00), (-11, 0)):
        base = dict(dog_threshold=threshold(GRID_T0, 2.0 ** e), edge_threshold=dc.GRID_KW["edge_threshold"])
        name = f"float: grid {_tag(e)} top-K half the list"
        out[name] = L._case(name, "topk", _grid(e), base=base, trunc=_half_the_list, key=key)
    e = 16
    base = dict(dog_threshold=threshold(GRID_T0, 2.0 ** e), edge_threshold=dc.GRID_KW["edge_threshold"])
    name = "float: grid 2^16 truncate highest1 inside a level"
    out[name] = L._case(name, "rows", _grid(e), base=base,
                        trunc=dict(truncate_method=_abi.TRUNC_HIGHEST_1, feature_count_threshold=dc.GRID_THRESHOLD), inside=True)
    return out


def check_list_reach(st, case, run):
    """The list case reaches what it is there for, asserted from the session's own untruncated list.  run: as for
    list_cases.check_case."""
    full = run(dict(case.base))
    key = L.topk_key(full.raw)
    want = 0x7c00 if "2^16" in case.name else 0
    assert len(key) > 500 and (key == want).all(), f"keys {sorted(set(key.tolist()))[:4]} ..., expected {want:#x} everywhere"
    if "key" in case.reach:
        K = st["trunc"]["feature_count_threshold"]
        assert K == len(key) // 2 and st["kept"] == K
        t = st["topk"]
        assert (t["sure"], t["ties"], t["need"], t["last_kept_tie"]) == (0, len(key), K, K - 1), t
        sel = run(dict(case.base, **st["trunc"]))
        assert sel.raw.tobytes() == full.raw[:K].tobytes(), "the kept rows are not the first K of the list"
    if case.reach.get("inside"):
        c, t = st["level_counts"], st["trunc"]["feature_count_threshold"]
        assert sum(c[2:]) < t < sum(c[1:]), (c, t)                          # the first pass stops inside level 1 and keeps it ...
        assert 0 < st["features"] < st["first_pass_features"], st          # ... the second, on the features, drops a level


def check_statistics(st, case):
    """detector_cases.check_statistics, and the conditions of these cases: nothing flagged, no small case."""
    dc.check_statistics(st, case)
    assert st["uncertain"] == 0 and st["orient_uncertain"] == 0, st
    if case.keys is None:
        assert st["candidates"] >= 50 and st["detections"] >= 8, st


# Wrong rule -> (case that catches it, stage)
CATCHES = {
    "float pixels clamped to [0, 1]": ("float: blobs 2^8", "gauss"),
    "float pixels above 1 divided by 255": ("float: blobs 255", "gauss"),
    "pivot test relative to the matrix": ("float: blobs 2^-14", "detect"),
    "half response saturates to 65504": ("float: blobs 2^16", "detect"),
    "threshold applied to the unscaled response": ("float: blobs 255", "detect"),
}
