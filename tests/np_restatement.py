"""Independent NumPy / pure-Python restatement of the reference's Hessian + SIFT path.

Written from the textual description in SURVEY.md section 8(a) and the reference source, NOT from
oracle/hess_oracle.c: vectorised float64 arithmetic for the dense stages, plain Python loops for
the per-keypoint stages (small cases only).  It shares no code with the oracle or the product;
tests/test_oracle_vs_numpy.py uses it to cross-check the oracle within tolerances (the oracle
itself is bit-exact only against the HIP path).  Reference lines are cited per function.
"""
import math

import numpy as np

PI = 3.14159265358979323846


# ---- schedule: SiftGPU.cpp:482-563,1422-1425 ----------------------------------------------------
def schedule(dog=3, sigma0=1.6, sigman=0.5, first_octave_ds=0):
    k = 2.0 ** (1.0 / dog)
    dsigma0 = sigma0 * math.sqrt(k * k - 1.0)
    inter = [dsigma0 * k ** i for i in range(dog + 1)]          # blur taking level i to i+1
    level_sigma = [sigma0 * 2.0 ** (l / dog) for l in range(dog + 2)]
    sb = sigman / 2.0 ** first_octave_ds
    init = math.sqrt(sigma0 * sigma0 - sb * sb)
    return init, inter, level_sigma


# ---- ProgramCU::CreateFilterKernel, ProgramCU.cu:423-453 ------------------------------------------
def filter_taps(sigma, factor=4.0, clamp33=True):
    """clamp33: the truncation to KERNEL_MAX_WIDTH = 33 (ProgramCU.cu:428-433), a switch for DetectorModel."""
    sz = int(math.ceil(factor * sigma - 0.5))
    width = max(2 * sz + 1, 5)
    if clamp33:
        width = min(width, 33)
    sz = width // 2
    i = np.arange(-sz, sz + 1, dtype=np.float64)
    k = np.exp(-0.5 * i * i / (sigma * sigma))
    return k / k.sum()


# ---- input conversion, GLTexImage.cpp:802-862 ------------------------------------------------------
def luminance(img):
    a = np.asarray(img)
    if a.ndim == 2:
        if a.dtype == np.uint8:
            return a.astype(np.float64) / 255.0
        if a.dtype == np.uint16:
            return a.astype(np.float64) / 65535.0
        return a.astype(np.float64)
    r, g, b = (a[..., i].astype(np.float64) for i in range(3))
    if a.dtype == np.uint8:
        return (19595.0 * r + 38470.0 * g + 7471.0 * b) / (65535.0 * 255.0)
    if a.dtype == np.uint16:
        return (19595.0 * r + 38470.0 * g + 7471.0 * b) / (65535.0 * 65535.0)
    return 0.299 * r + 0.587 * g + 0.114 * b


# ---- FilterH / FilterV with replicated borders, ProgramCU.cu:117-231 -------------------------------
def gaussian(img, taps):
    r = len(taps) // 2
    p = np.pad(img, ((0, 0), (r, r)), mode="edge")
    h = sum(taps[i] * p[:, i:i + img.shape[1]] for i in range(len(taps)))
    p = np.pad(h, ((r, r), (0, 0)), mode="edge")
    return sum(taps[i] * p[i:i + img.shape[0], :] for i in range(len(taps)))


# ---- DownsampleKernel, ProgramCU.cu:312-326 + 4-aligned widths, PyramidCU.cpp:274-309 --------------
def downsample(src, dst_w_aligned, dst_h):
    sw = src.shape[1]
    cols = np.minimum(np.arange(dst_w_aligned) * 2, sw - 1)
    return src[np.arange(dst_h) * 2][:, cols]


def octave_geometry(w, h, octave_num=-1):
    w &= ~3
    nmax = max(1, int(math.floor(math.log(min(w, h)) / math.log(2.0))) - 3)
    n = octave_num if 1 <= octave_num < nmax else nmax
    out = []
    for _ in range(n):
        out.append((((w + 3) // 4) * 4, h))
        w >>= 1
        h >>= 1
    return out


def build_pyramid(lum, dog=3, octave_num=-1):
    init, inter, _ = schedule(dog)
    geo = octave_geometry(lum.shape[1], lum.shape[0], octave_num)
    lum = lum[:, :geo[0][0]]
    pyr = []
    for o, (wa, h) in enumerate(geo):
        if o == 0:
            levels = [gaussian(lum, filter_taps(init))]
        else:
            levels = [downsample(pyr[o - 1][dog], wa, h)]
        for l in range(1, dog + 2):
            levels.append(gaussian(levels[-1], filter_taps(inter[l - 1])))
        pyr.append(levels)
    return pyr


# ---- ComputeHessian_Kernel, ProgramCU.cu:523-595: 1-D index neighbours, zero outside the plane -----
def hessian_planes(g, sigma, clamp=False):
    """The neighbour of pixel i at (dy, dx) is index i + dy w + dx of the FLAT plane: at a row's end that is the next
    row's first pixel, before and past the plane a fetch returns 0.  On a plane of one row every vertical neighbour is 0,
    on one of four columns half the horizontal ones are a row end.  clamp: the WRONG rule (replicated borders, as the
    filters have them)."""
    h, w = g.shape
    flat = np.concatenate([np.zeros(w + 1), g.ravel(), np.zeros(w + 1)])
    base = w + 1
    n = h * w
    edge = np.pad(g, 1, mode="edge") if clamp else None

    def nb(dy, dx):
        if clamp:
            return edge[1 + dy: 1 + dy + h, 1 + dx: 1 + dx + w]
        off = dy * w + dx
        return flat[base + off: base + off + n].reshape(h, w)

    v11, v12, v13 = nb(-1, -1), nb(-1, 0), nb(-1, 1)
    v21, v22, v23 = nb(0, -1), nb(0, 0), nb(0, 1)
    v31, v32, v33 = nb(1, -1), nb(1, 0), nb(1, 1)
    lxx = v21 - 2.0 * v22 + v23
    lyy = v12 - 2.0 * v22 + v32
    lxy = (v13 - v11 + v31 - v33) * 0.25
    deth = (lxx * lyy - lxy * lxy) * sigma ** 4
    dx, dy = v23 - v21, v32 - v12
    grad = 0.5 * np.sqrt(dx * dx + dy * dy)
    theta = np.where(grad == 0.0, 0.0, np.arctan2(dy, dx))
    return deth, grad, theta


# ---- ComputeKEY_Kernel, ProgramCU.cu:702-882 (pure Python, one pixel) -----------------------------
def key_test(C, P, N, G, row, col, T, edge=10.0, subpixel=True):
    """-> None or (response, type, dx, dy, ds).  C/P/N: det-H of the level / previous / next.  The rule itself is stated
    once, in key_test_ex below, which also says how close each gate came to its threshold."""
    return key_test_ex(C, P, N, G, row, col, T, edge, subpixel)[0]


# ---- ComputeOrientation_Kernel, ProgramCU.cu:1221-1605 (multi-orientation branch) -----------------
def orientations(grad, theta, x, y, s, half=False, gaussian_factor=1.5, window_factor=2.0):
    """-> list of up to 4 rotations in bin units (rot in [0,36)), strongest first.  Stated once, in orientations_ex."""
    return orientations_ex(grad, theta, x, y, s, half, gaussian_factor, window_factor)[0]


# ---- ComputeDescriptor_Kernel + NormalizeDescriptor_Kernel, ProgramCU.cu:1650-2054 -----------------
def descriptor(grad, theta, x, y, s, angle, half=False, window_factor=3.0):
    """Stated once, in descriptor_ex."""
    return descriptor_ex(grad, theta, x, y, s, angle, half, window_factor)


# =====================================================================================================================
# DetectorModel: every option of the Hessian detector and of the difference-of-Gaussians detector, end to end on a small
# image, in float64.
#
# Written from the reference source (lines cited per rule) and SURVEY.md section 8.  A rule marked PROJECT is the
# project's own: the reference does not state it (or cannot reach it).  Keyword switches of DetectorModel state
# plausible WRONG rules with the same code (WRONG_RULES); tests/test_detector_model.py shows that each one is caught.
#
# The difference-of-Gaussians mode (detector = 1) is the reference compiled WITHOUT GPU_HESSIAN, stated from the #else /
# #ifndef lines alone.  Its rules, each once, where the Hessian rule is stated, behind a switch:
#   schedule    DetectorModel.__init__, level_sigma, initial_sigma       SiftGPU.cpp:466-556
#   planes      response_plane, scan_planes                               ProgramCU.cu:598-637, PyramidCU.cpp:1593-1605, 1654-1670
#   key test    key_test_ex(dog=True)                                     ProgramCU.cu:680-699, 853-854
#   orientation orientations_ex(two_peaks=True), rotations                ProgramCU.cu:1493-1548, PyramidCU.cpp:763-767, 800-820
# Shared code that the build without GPU_HESSIAN reaches through other lines, or not at all -- the product keeps the
# records of the GPU_HESSIAN / GPU_SIFT_MODIFIED builds in both modes, so these are PROJECT in DoG mode:
#   * the list record: that build stores x, y and the scale as floats (ProgramCU.cu:1417-1419, 1557-1559), not as 14.10 /
#     8.8 fixed point with the half-precision response and the type (:1574-1596, the GPU_SIFT_MODIFIED form kept here);
#     export() and user_key() therefore round as in the Hessian mode;
#   * keypoint lists: binned by the same half-step rule on GetLevelSigma(level + _level_min + 1), levels counted from 0
#     (PyramidCU.cpp:575, 583, 607-610) -- the same sigmas and the same catch-alls in this numbering; the record is the
#     float one (:668-692);
#   * top-K exists only with GPU_HESSIAN or GPU_SIFT_MODIFIED (config.h:81-85, PyramidCU.cpp:1879-1989); the level
#     truncation passes (SiftPyramid.cpp:224-277, PyramidCU.cpp:1283-1345) and the descriptor (ProgramCU.cu:1650-2054)
#     are the same lines in every build.
# =====================================================================================================================
U = 2.0 ** -24                      # unit round-off of binary32
TEN_DEG = 5.7295779513082320876798154814105
TRUNC_HIGHEST_0, TRUNC_HIGHEST_1, TRUNC_LOWEST, TRUNC_TOPK = 0, 1, 2, 3   # GlobalUtil.h TRUNCATE_METHOD_*
FMT_LUM, FMT_RGB, FMT_RGBA, FMT_BGR, FMT_BGRA = 1, 3, 4, 5, 6

WRONG_RULES = {
    "top-K ties go to the higher index": dict(topk_tie_high=True),
    "top-K keyed on the float response": dict(topk_float_key=True),
    "second truncation pass omitted": dict(no_second_pass=True),
    "up-sample row end clamps": dict(upsample_clamp=True),
    "first blur not skipped": dict(no_skip=True),
    "33-tap clamp omitted": dict(no_clamp33=True),
    "half fold refreshes the 37th slot": dict(fold_refresh=True),
    "single peak takes the last maximum": dict(single_last=True),
    "subpixel=0 keeps the 0.8 factor": dict(keep08=True),
    "16-bit RGB does not wrap": dict(no_wrap=True),
    "level binning rounds at whole steps": dict(whole_step=True),
    "lowe_origin offset before the octave scale": dict(lowe_before_scale=True),
    # the difference-of-Gaussians mode (detector = 1)
    "DoG extrema keep the Hessian sign tests": dict(dog_sign_tests=True),
    "DoG list level sought one plane lower": dict(dog_plane_lower=True),
    "DoG type from L_xx": dict(dog_type_lxx=True),
    "DoG angles are 8-bit": dict(dog_angle8=True),
    "DoG keeps up to four peaks": dict(dog_four_peaks=True),
    "DoG next octave from the level above": dict(dog_ds_above=True),
    "DoG level sigma one level off": dict(dog_sigma_off=True),
    # planes below one tile (detector_cases.small_cases)
    "empty window gives NaN": dict(empty_nan=True),
    "det-H neighbours clamp at the row ends": dict(deth_clamp=True),
    # float pixels of any range (float_range_cases.cases)
    "float pixels clamped to [0, 1]": dict(float_clamp=True),
    "float pixels above 1 divided by 255": dict(float_div255=True),
    "pivot test relative to the matrix": dict(pivot_relative=True),
    "half response saturates to 65504": dict(half_saturates=True),
    "threshold applied to the unscaled response": dict(threshold_unscaled=True),
}


def f2h(v, saturate=False):
    """binary32 -> binary16 -> float, round to nearest even (__float2half_rn / half2float, GlobalUtil.cpp:588-621): a value
    of 65520 or more becomes inf, one below 2^-14 is rounded to a multiple of 2^-24, one of 2^-25 or less to 0.
    saturate: the WRONG rule, the largest finite half instead of inf."""
    with np.errstate(over="ignore"):
        h = float(np.float32(v).astype(np.float16))
    if saturate and math.isinf(h):
        return math.copysign(65504.0, h)
    return h


def fixed(v, bits):
    """FLOAT_TO_FIXED_POINT, config.h:73-74: (int)(v * 2^bits + 0.5), evaluated in double."""
    return int(v * (1 << bits) + 0.5)


# ---- input conversion with decimation, GLTexImage.cpp:802-916 (DownSamplePixelDataI2F / F) ------------------------
def input_plane(img, fmt=None, ds=0, no_wrap=False, float_clamp=False, float_div255=False):
    """-> float64 [H >> ds, (W >> ds) & ~3]: every 2^ds-th pixel of every 2^ds-th row (ws = width/ds - skip with skip the
    columns TruncateWidthCU drops, :998-1016).  Integer types: the numerator 19595 R + 38470 G + 7471 B is an `int`
    expression (:842), so it wraps modulo 2^32 for bright 16-bit pixels.  Float pixels are taken as they are (:866-912:
    `*po++ = *p`, no scale, no clamp), whatever their range and sign.  float_clamp, float_div255: the WRONG rules -- a clamp
    to [0, 1], and a division by 255 of an image that has a value above 1 (the guess that such an image holds byte values)."""
    a = np.asarray(img)
    if a.dtype == np.float32 and float_clamp:
        a = np.clip(a, 0.0, 1.0)
    if a.dtype == np.float32 and float_div255 and a.size and float(a.max()) > 1.0:
        a = a / np.float32(255.0)
    step = 1 << ds
    h, w = a.shape[0] >> ds, (a.shape[1] >> ds) & ~3
    a = a[:h * step:step, :w * step:step]
    if a.ndim == 2:
        if a.dtype == np.uint8:
            return a.astype(np.float64) / 255.0
        if a.dtype == np.uint16:
            return a.astype(np.float64) / 65535.0
        return a.astype(np.float64)
    c = (2, 1, 0) if fmt in (FMT_BGR, FMT_BGRA) else (0, 1, 2)
    if a.dtype in (np.uint8, np.uint16):
        r, g, b = (a[..., i].astype(np.int64) for i in c)
        num = 19595 * r + 38470 * g + 7471 * b
        if not no_wrap:
            num = (num + (1 << 31)) % (1 << 32) - (1 << 31)      # two's-complement int32
        return num.astype(np.float64) / (65535.0 * (255.0 if a.dtype == np.uint8 else 65535.0))
    r, g, b = (a[..., i].astype(np.float64) for i in c)
    return float(np.float32(0.299)) * r + float(np.float32(0.587)) * g + float(np.float32(0.114)) * b   # :894,906


# ---- UpsampleKernel, ProgramCU.cu:233-285: bilinear by 2^k, the source fetched by 1-D index -----------------------
def upsample(src, k, clamp=False):
    """Source pixel (row, col) yields 2^k output pixels of every output row dst_row >> k == row.  Its right and lower
    neighbours are index + 1 and index + width of the FLAT plane: at the end of a row that is the next row's first
    pixel, past the plane a texture fetch returns 0.  clamp: the WRONG rule (replicated border)."""
    h, w = src.shape
    S = 1 << k
    if clamp:
        p = np.pad(src, ((0, 1), (0, 1)), mode="edge")
        v11, v12, v21, v22 = p[:h, :w], p[:h, 1:], p[1:, :w], p[1:, 1:]
    else:
        flat = np.concatenate([src.ravel(), np.zeros(w + 2)])
        idx = np.arange(h * w).reshape(h, w)
        v11, v12, v21, v22 = flat[idx], flat[idx + 1], flat[idx + w], flat[idx + w + 1]
    out = np.zeros((h * S, w * S))
    for helper in range(S):
        w1 = helper / S
        v1 = v21 * w1 + (1.0 - w1) * v11 if helper else v11
        v2 = v22 * w1 + (1.0 - w1) * v12 if helper else v12
        for i in range(S):
            out[helper::S, i::S] = v1 * (1.0 - i / S) + v2 * (i / S) if i else v1
    return out


# ---- ComputeKEY_Kernel with rounding margins ------------------------------------------------------------------------
def key_test_ex(C, P, N, G, row, col, T, edge=10.0, subpixel=True, keep08=False, dog=False, dog_sign_tests=False,
                dog_type_lxx=False, pivot_relative=False):
    """ComputeKEY_Kernel, ProgramCU.cu:702-882 (pure Python, one pixel) -> (result, uncertain); result is None or
    (response, type, dx, dy, ds).  uncertain: a gate value lies within 8 x a first-order bound of the
    binary32 evaluation's error of its threshold, so the float32 implementation may decide either way (the comparisons
    of r with its neighbours are exact on float32 planes and never flagged).
    dog: the kernel as compiled without GPU_HESSIAN.  READ_CMP_DOG_DATA (:680-699) has no sign conditions -- a maximum may
    be negative and a minimum positive -- and the type is BRIGHT where `response > nmax` and DARK otherwise (:853-854),
    with the response AFTER the sub-pixel step and nmax as the neighbour tests left it: the largest of all 26 neighbours
    at a maximum, of the left and right neighbour only at a minimum (the else branch never touches nmax).  There is no
    saddle type.  dog_sign_tests, dog_type_lxx: the WRONG rules that keep the Hessian lines.
    THE PIVOT GUARDS of the sub-pixel solve are ABSOLUTE: maxa >= 1e-10 and the two abs(..) >= 1e-10 (:790, 808, 813), on
    second differences of the response, which scale with the square of the pixels' amplitude (with the amplitude in the
    DoG build).  Below an amplitude of about 2^-13 no candidate has a pivot of 1e-10: "no solution", offsets 0, the
    response that of the pixel, and none of the tests on the refined values.  pivot_relative: the WRONG rule, the guards
    taken relative to the largest entry of the system."""
    signs = not dog or dog_sign_tests
    T = float(T)
    thr0 = (0.8 if (subpixel or keep08) else 1.0) * T
    edge_t = (edge + 1.0) ** 2 / edge
    r = float(C[row, col])
    unc = abs(abs(r) - thr0) <= 8 * U * thr0
    if abs(r) <= thr0:
        return None, unc
    left, right = float(C[row, col - 1]), float(C[row, col + 1])
    nmax, nmin = max(left, right), min(left, right)
    if nmin <= r <= nmax:
        return None, False
    state = [nmax, nmin]

    def triple(plane, rr):
        vals = [float(plane[rr, col - 1]), float(plane[rr, col]), float(plane[rr, col + 1])]
        if r > state[0]:
            state[0] = max([state[0]] + vals)
            return not (r < state[0] or (signs and r < 0))
        state[1] = min([state[1]] + vals)
        return not (r > state[1] or (signs and r > 0))

    if not triple(C, row - 1) or not triple(C, row + 1):
        return None, False
    up, dn = float(C[row - 1, col]), float(C[row + 1, col])
    c4 = [float(C[row + 1, col + 1]), float(C[row - 1, col - 1]), float(C[row + 1, col - 1]), float(C[row - 1, col + 1])]
    fxx, exx = left + right - 2 * r, 3 * U * (abs(left) + abs(right) + 2 * abs(r))
    fyy, eyy = up + dn - 2 * r, 3 * U * (abs(up) + abs(dn) + 2 * abs(r))
    fxy, exy = 0.25 * (c4[0] + c4[1] - c4[2] - c4[3]), U * sum(abs(v) for v in c4)
    det = fxx * fyy - fxy * fxy
    edet = abs(fyy) * exx + abs(fxx) * eyy + 2 * abs(fxy) * exy + 2 * U * (abs(fxx * fyy) + fxy * fxy)
    tr = fxx + fyy
    g = tr * tr - edge_t * det
    eg = 2 * abs(tr) * (exx + eyy + U * abs(tr)) + U * tr * tr + edge_t * edet + 2 * U * edge_t * abs(det)
    unc = unc or abs(det) <= 8 * edet or abs(g) <= 8 * eg
    if det <= 0 or g > 0:
        return None, unc
    for plane in (P, N):
        for rr in (row - 1, row, row + 1):
            if not triple(plane, rr):
                return None, False
    dx = dy = ds = 0.0
    resp = r
    eresp = 0.0
    if subpixel:
        pc, nc = float(P[row, col]), float(N[row, col])
        fx, fy, fs = 0.5 * (right - left), 0.5 * (dn - up), 0.5 * (nc - pc)
        fss = nc + pc - 2 * r
        fxs = 0.25 * (float(N[row, col + 1]) + float(P[row, col - 1]) - float(N[row, col - 1]) - float(P[row, col + 1]))
        fys = 0.25 * (float(N[row + 1, col]) + float(P[row - 1, col]) - float(N[row - 1, col]) - float(P[row + 1, col]))
        rows = [[fxx, fxy, fxs, -fx], [fxy, fyy, fys, -fy], [fxs, fys, fss, -fs]]
        rows = [rw if rw[0] > 0 else [-v for v in rw] for rw in rows]
        maxa = max(rw[0] for rw in rows)
        solved = False
        piv = [maxa]
        guard = 1e-10 * max(abs(v) for rw in rows for v in rw[:3]) if pivot_relative else 1e-10
        if maxa >= guard:
            if maxa == rows[1][0]:
                rows[0], rows[1] = rows[1], rows[0]
            elif maxa == rows[2][0]:
                rows[0], rows[2] = rows[2], rows[0]
            a0 = [rows[0][0]] + [v / rows[0][0] for v in rows[0][1:]]
            a1 = [rows[1][0]] + [rows[1][j] - rows[1][0] * a0[j] for j in (1, 2, 3)]
            a2 = [rows[2][0]] + [rows[2][j] - rows[2][0] * a0[j] for j in (1, 2, 3)]
            if abs(a2[1]) > abs(a1[1]):
                a1, a2 = a2, a1
            piv.append(abs(a1[1]))
            if abs(a1[1]) >= guard:
                a1 = a1[:2] + [a1[2] / a1[1], a1[3] / a1[1]]
                a2 = a2[:2] + [a2[2] - a2[1] * a1[2], a2[3] - a2[1] * a1[3]]
                piv.append(abs(a2[2]))
                if abs(a2[2]) >= guard:
                    solved = True
                    ds = a2[3] / a2[2]
                    dy = a1[3] - ds * a1[2]
                    dx = a0[3] - ds * a0[2] - dy * a0[1]
                    resp = r + 0.5 * (dx * fx + dy * fy + ds * fs)
        unc = unc or any(abs(p - 1e-10) <= 1e-11 for p in piv)       # a pivot at its guard
        if solved:
            A = np.array([[fxx, fxy, fxs], [fxy, fyy, fys], [fxs, fys, fss]])
            # the solution of a 3 x 3 system in binary32: relative error <= c u cond(A), c = 8 covers the elimination
            eoff = 8 * U * float(np.linalg.cond(A)) * max(abs(dx), abs(dy), abs(ds))
            eresp = 2 * U * (abs(r) + abs(dx * fx) + abs(dy * fy) + abs(ds * fs)) + 0.5 * eoff * (abs(fx) + abs(fy) + abs(fs))
            unc = unc or any(abs(abs(v) - 1.0) <= 8 * eoff for v in (dx, dy, ds)) or abs(abs(resp) - T) <= 8 * eresp
            if not (abs(resp) > T and abs(ds) < 1 and abs(dx) < 1 and abs(dy) < 1):
                return None, unc
    if dog and not dog_type_lxx:
        unc = unc or (eresp > 0 and abs(resp - state[0]) <= 8 * eresp)
        typ = 1 if resp > state[0] else 0
    elif resp < 0 and not dog:
        typ = 2
    else:
        gl, gc, gr = float(G[row, col - 1]), float(G[row, col]), float(G[row, col + 1])
        lxx = gl - 2 * gc + gr
        unc = unc or abs(lxx) <= 8 * 3 * U * (abs(gl) + 2 * abs(gc) + abs(gr))
        typ = 0 if lxx > 0 else 1
    return (resp, typ, dx, dy, ds), unc


def scan_level(C, P, N, G, T, edge=10.0, subpixel=True, keep08=False, **dog):
    """All interior pixels of one level (ProgramCU.cu:702-882) -> ({(row, col): result}, {(row, col)} uncertain, number
    of candidates).  The exact part is vectorised: |r| against a threshold loosened by its margin and r against its 26
    neighbours with non-strict comparisons (a superset of the triple rule, with or without the sign conditions);
    key_test_ex sees the survivors only.  dog: key_test_ex's keywords of the difference-of-Gaussians build."""
    C, P, N = (np.asarray(a, dtype=np.float32) for a in (C, P, N))
    h, w = C.shape
    thr0 = (0.8 if (subpixel or keep08) else 1.0) * float(T)
    c = C[1:h - 1, 1:w - 1]
    ge = np.ones(c.shape, bool)
    le = np.ones(c.shape, bool)
    for pl in (C, P, N):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if pl is C and dy == 1 and dx == 1:
                    continue
                nb = pl[dy:dy + h - 2, dx:dx + w - 2]
                ge &= c >= nb
                le &= c <= nb
    cand = (np.abs(c) > thr0 * (1 - 16 * U)) & (ge | le)
    found, unsure = {}, set()
    for row, col in np.argwhere(cand) + 1:
        res, unc = key_test_ex(C, P, N, G, int(row), int(col), T, edge, subpixel, keep08, **dog)
        if unc:
            unsure.add((int(row), int(col)))
        if res is not None:
            found[(int(row), int(col))] = res
    return found, unsure, int(cand.sum())


# ---- ComputeOrientation_Kernel, both branches, with rounding margins ------------------------------------------------
def orientations_ex(grad, theta, x, y, s, half=False, gaussian_factor=1.5, window_factor=2.0, single=False,
                    fold_refresh=False, single_last=False, two_peaks=False, info=None):
    """-> (rotations in bin units, uncertain).  multi (ProgramCU.cu:1430-1489): every strict local maximum above 0.8 x the
    largest vote, the 4 strongest, strongest first, equal weights in bin order.  single (:1398-1420, -m 1 and keypoint
    lists): the FIRST strict maximum (`vote[i] > max_vote`), no 0.8 rule; its right neighbour is vote[index + 1], whose
    slot 36 holds the UNFOLDED vote[0] under -half (:1381-1392).  uncertain: a comparison that decides the set or the
    order of the peaks lies within 8 x (error bound of the two votes).
    two_peaks (the build without GPU_HESSIAN, :1493-1548): the same qualifying peaks, visited in bin order and kept in two
    slots that start at weight 0: a peak above slot 1 goes into slot 0 if it is above slot 0 (whose holder moves to slot
    1), else into slot 1; both comparisons are strict, so of equal peaks the one met first stays ahead and a third equal
    one is dropped.  That leaves the two strongest, stronger first.  info: a dict that receives `peaks`, the number of
    qualifying peaks."""
    h, w = grad.shape
    gs = s * gaussian_factor
    win = abs(s) * gaussian_factor * window_factor
    factor = -0.5 / (gs * gs)
    xmin, ymin = max(1.5, math.floor(x - win) + 0.5), max(1.5, math.floor(y - win) + 0.5)
    xmax, ymax = min(w - 1.5, math.floor(x + win) + 0.5), min(h - 1.5, math.floor(y + win) + 0.5)
    vote = np.zeros(37)
    err = np.zeros(37)
    if xmax >= xmin and ymax >= ymin:
        xs = np.arange(xmin, xmax + 0.25)
        ys = np.arange(ymin, ymax + 0.25)
        d2 = (xs[None, :] - x) ** 2 + (ys[:, None] - y) ** 2
        g = grad[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)]
        t = theta[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)] * TEN_DEG
        inside = d2 < win * win + 0.5
        b = np.floor(t).astype(int)
        wgt = np.where(inside, g * np.exp(d2 * factor), 0.0)
        near = inside & (np.abs(t - np.rint(t)) <= 4 * U * np.abs(t) + 1e-12)     # the bin itself may differ
        # |win^2 + 0.5 - d2| tiny: membership may differ
        edge = np.abs(d2 - (win * win + 0.5)) <= 8 * U * (d2 + win * win)
        np.add.at(vote, b % 36, wgt)
        cnt = np.bincount((b % 36)[inside], minlength=37)[:37]
        err[:36] = U * (cnt[:36] + 6) * vote[:36]                                 # n additions, exp, product
        for m in (near, edge):
            if m.any():
                wg = g * np.exp(d2 * factor)
                np.add.at(err, (b % 36)[m], wg[m])
                np.add.at(err, ((b - 1) % 36)[m], wg[m])
                np.add.at(err, ((b + 1) % 36)[m], wg[m])
    for _ in range(6):
        old, olde = vote[:36].copy(), err[:36].copy()
        vote[:36] = (np.roll(old, 1) + old + np.roll(old, -1)) / 3.0
        err[:36] = (np.roll(olde, 1) + olde + np.roll(olde, -1)) / 3.0 + 4 * U * vote[:36]
    vote[36], err[36] = vote[0], err[0]
    if half:
        vote[:18] += vote[18:36]
        err[:18] += err[18:36] + U * vote[:18]
        vote[18:36] = 0.0
        err[18:36] = 0.0
        if fold_refresh:
            vote[36], err[36] = vote[0], err[0]
    v = vote
    mx = float(v[:36].max())
    unc = False
    if single and not v[:36].any():
        # THE ALL-ZERO HISTOGRAM (no sample under the window -- every key on a plane of one or two rows -- or no gradient
        # there): exactly zero in binary32 too, so nothing is uncertain.  :1400-1415: no vote[i] > 0, index_max = 0,
        # max_vote = pre = next = 0 and off = 0.5f * FDIV(0, 0); __fdividef is x * rcp(y) = 0 * inf, NaN like the IEEE
        # quotient: key.w is NaN.  The multi-peak branches below need no line of their own: the threshold 0.8 * 0 admits
        # no vote[i] > 0, so orientationsCount = 0 and the packed 8-bit angles are 0 (:1448, 1474-1489), in the build
        # without GPU_HESSIAN ocount = 0 and both 16-bit codes are 65535, 'none' (:1500-1548): no feature either way.
        return [float("nan")], False
    if single:
        imax = 0
        for i in range(1, 36):
            if (v[i] >= v[imax]) if single_last else (v[i] > v[imax]):
                imax = i
        unc = any(i != imax and abs(v[i] - mx) <= 8 * (err[i] + err[imax]) for i in range(36))
        pre, nxt = v[35 if imax == 0 else imax - 1], v[imax + 1]
        den = 2 * mx - nxt - pre
        off = 0.5 * (nxt - pre) / den if den != 0 else 0.0
        return [imax + 0.5 + off], bool(unc) or den == 0
    peaks = []
    imx = int(v[:36].argmax())
    for i in range(36):
        pre, nxt = v[i - 1] if i else v[35], v[i + 1]
        m = 8 * (err[i] + max(err[i - 1] if i else err[35], err[i + 1], err[imx]))
        is_peak = v[i] > 0.8 * mx and v[i] > pre and v[i] > nxt
        if v[i] > 0.8 * mx - m and v[i] > pre - m and v[i] > nxt - m:             # a peak within the margin
            if abs(v[i] - 0.8 * mx) <= m or abs(v[i] - pre) <= m or abs(v[i] - nxt) <= m:
                unc = True
        if is_peak:
            di = 0.5 * (nxt - pre) / (2 * v[i] - nxt - pre)
            peaks.append((v[i], i + di + 0.5, err[i]))
    if info is not None:
        info["peaks"] = len(peaks)
    if two_peaks:
        kept = [peaks[i] for i in two_slots([p[0] for p in peaks])]
    else:
        kept = sorted(peaks, key=lambda p: -p[0])[:4]
    ranked = sorted(peaks, key=lambda p: -p[0])
    for a, b_ in zip(ranked, ranked[1:]):                                           # the order, and who is last
        if abs(a[0] - b_[0]) <= 8 * (a[2] + b_[2]):
            unc = True
    return [p[1] for p in kept], bool(unc)


def two_slots(weights):
    """ProgramCU.cu:1500-1532, 1538-1541: the weights of the qualifying peaks in bin order -> indices of the kept ones,
    slot 0 first.  max_vot = {0, 0}; a weight above slot 1 goes into slot 0 if it is above slot 0, whose holder moves to
    slot 1, else into slot 1, and is counted; slot 0 is read if anything was counted, slot 1 if more than one was."""
    slot, ocount = [(0.0, None), (0.0, None)], 0
    for i, w in enumerate(weights):
        if w > slot[1][0]:
            slot = [(w, i), slot[0]] if w > slot[0][0] else [slot[0], (w, i)]
            ocount += 1
    return [sl[1] for sl in slot[:min(ocount, 2)]]


def descriptor_ex(grad, theta, x, y, s, angle, half=False, window_factor=3.0, dynamic_indexing=False, normalize=True,
                  empty_nan=False):
    """ComputeDescriptor_Kernel + NormalizeDescriptor_Kernel, ProgramCU.cu:1650-2054, with -di and normalize=0.  A sample whose bin coordinate is 8.0 AS A binary32 NUMBER
    (th < 0 by less than half an ulp of 8, so th + 8 rounds up) falls into no bin, or into des[8] with -di
    (ProgramCU.cu:1745-1776): the one place where the float64 model has to ask for the float32 value.
    THE EMPTY WINDOW.  A key whose 16 boxes hold no sample (any key on a plane of one or two rows: ymin = 1.5 > ymax =
    h - 1.5; a key far outside the plane) has des = 0 everywhere.  The normalisation then forms min(0.2f, 0 * rsqrt(0))
    = min(0.2f, NaN) (:1989-1995, the -half kernel :2034-2044, the build without GPU_HESSIAN :2077-2090), and CUDA's min
    on floats returns the operand that is not NaN: every component becomes 0.2, and after the second pass 0.2 /
    sqrt(dim 0.04) = 1 / sqrt(dim).  Not NaN, not zero.  With normalize=0 the zeros are returned as they are.
    empty_nan: the WRONG rule (a min that propagates NaN, as np.minimum and a comparison-and-select do).
    A NaN ANGLE (the single-peak orientation of an all-zero histogram, orientations_ex) makes nx and ny NaN for every
    sample, `(nxn < 1.0f) && (nyn < 1.0f)` (:1735) false, and the window empty whatever the boxes are (max / min in
    :1713-1716 drop the NaN operand as well: the boxes are the whole plane)."""
    h, w = grad.shape
    if math.isnan(angle):
        d = np.zeros(64 if half else 128)
        return _normalized(d, empty_nan) if normalize else d
    spt = abs(s * window_factor)
    sn, cs = math.sin(angle), math.cos(angle)
    anglef = angle - 2 * PI if angle > PI else angle
    out = []
    for cell in range(16):
        ix, iy = cell & 3, cell >> 2
        ox, oy = ix - 1.5, iy - 1.5
        px = cs * spt * ox - sn * spt * oy + x
        py = cs * spt * oy + sn * spt * ox + y
        bsz = abs(cs * spt) + abs(sn * spt)
        xmin, ymin = max(1.5, math.floor(px - bsz) + 0.5), max(1.5, math.floor(py - bsz) + 0.5)
        xmax, ymax = min(w - 1.5, math.floor(px + bsz) + 0.5), min(h - 1.5, math.floor(py + bsz) + 0.5)
        des = np.zeros(9)
        if xmax >= xmin and ymax >= ymin:
            xs, ys = np.arange(xmin, xmax + 0.25), np.arange(ymin, ymax + 0.25)
            dx, dy = (xs - px)[None, :], (ys - py)[:, None]
            nx, ny = (cs * dx + sn * dy) / spt, (cs * dy - sn * dx) / spt
            g = grad[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)]
            t = theta[int(ymin):int(ymin) + len(ys), int(xmin):int(xmin) + len(xs)]
            ok = (np.abs(nx) < 1) & (np.abs(ny) < 1)
            wgt = np.exp(-0.125 * ((nx + ox) ** 2 + (ny + oy) ** 2)) * (1 - np.abs(nx)) * (1 - np.abs(ny)) * g
            th = (anglef - t) * 4.0 / PI
            th = np.where(th < 0, th + 8.0, th)
            th = np.where(th.astype(np.float32) >= np.float32(8.0), 8.0, th)
            fo = np.floor(th)
            ok &= (fo >= 0) & ((fo <= 8) if dynamic_indexing else (fo < 8))
            fo_i = fo.astype(int)[ok]
            np.add.at(des, fo_i, ((fo + 1 - th) * wgt)[ok])
            hi = fo_i + 1
            np.add.at(des, hi[hi <= 8], ((th - fo) * wgt)[ok][hi <= 8])
        des[0] += des[8]
        out.extend([des[k] + des[k + 4] for k in range(4)] if half else des[:8])
    d = np.array(out)
    return _normalized(d, empty_nan) if normalize else d


def _normalized(d, empty_nan=False):
    """NormalizeDescriptor_Kernel, ProgramCU.cu:1972-2054: unit length, the clamp to 0.2 by a min that keeps the operand
    which is not NaN (np.fmin), unit length again."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (np.minimum if empty_nan else np.fmin)(0.2, d * (1.0 / np.sqrt((d * d).sum())))
        return d / np.sqrt((d * d).sum())


class DetectorModel:
    """One parameter set -> every rule of the path as a method.  `params` is anything with the fields of hess_params
    (a Session's .params, or a dict); a field that is 0 takes the default ParseSiftParam gives it (SiftGPU.cpp:491-563)."""

    def __init__(self, params=None, **wrong):
        if params is None or isinstance(params, dict):
            table = params or {}
            get = table.get
        else:
            get = lambda k, d: getattr(params, k)
        self.wrong = dict(topk_tie_high=False, topk_float_key=False, no_second_pass=False, upsample_clamp=False,
                          no_skip=False, no_clamp33=False, fold_refresh=False, single_last=False, keep08=False,
                          no_wrap=False, whole_step=False, lowe_before_scale=False, dog_sign_tests=False,
                          dog_plane_lower=False, dog_type_lxx=False, dog_angle8=False, dog_four_peaks=False,
                          dog_ds_above=False, dog_sigma_off=False, empty_nan=False, deth_clamp=False,
                          float_clamp=False, float_div255=False, pivot_relative=False, half_saturates=False,
                          threshold_unscaled=False)
        assert set(wrong) <= set(self.wrong), wrong
        self.wrong.update(wrong)
        self.detector = int(get("detector", 0))
        assert self.detector in (0, 1), "the model states the Hessian (0) and the difference-of-Gaussians (1) detector"
        self.is_dog = self.detector == 1
        self.dog = int(get("dog_level_num", 3)) or 3
        # PROJECT: sigma0 is the sigma of this numbering's level 0 in both modes.  The build without GPU_HESSIAN counts its
        # levels from _level_min = -1 (SiftGPU.cpp:471) and its _sigma0 belongs to ITS level 0, this numbering's level 1:
        # the default there is 1.6 * 2^(1/dog) (:503), i.e. 1.6 for the level below, as here.
        self.sigma0 = float(get("sigma0", 1.6)) or float(np.float32(1.6))
        self.sigman = float(get("sigman", 0.5)) or 0.5
        self.T = float(get("dog_threshold", 0.0)) or float(np.float32(0.02) / np.float32(self.dog))
        self.edge = float(get("edge_threshold", 10.0)) or 10.0
        self.fwf = float(get("filter_width_factor", 4.0))
        self.owf = float(get("orient_window_factor", 2.0))
        self.ogf = float(get("orient_gaussian_factor", 1.5))
        self.dwf = float(get("desc_window_factor", 3.0))
        self.first_octave = int(get("first_octave", 0))
        self.octave_num = int(get("octave_num", -1))
        self.subpixel = bool(get("subpixel", 1))
        self.max_orientation = int(get("max_orientation", 2))
        self.fixed_orientation = bool(get("fixed_orientation", 0))
        self.lowe_origin = bool(get("lowe_origin", 0))
        self.half = bool(get("half_sift", 0))
        self.normalize = bool(get("normalize", 1))
        self.method = int(get("truncate_method", 0))
        self.fct = int(get("feature_count_threshold", -1))
        self.maxd = int(get("tex_max_dim", 3200))
        self.ads = bool(get("auto_downscale", 0))
        self.di = bool(get("dynamic_indexing", 0))
        k = 2.0 ** (1.0 / self.dog)
        self.sigma_step = k
        if self.is_dog:
            # SiftGPU.cpp:471, 496-497, 509: levels _level_min = -1 .. _level_max = dog + 1, dog + 3 of them: the build's
            # level j - 1 is level j here, 0 .. dog + 2.  :531, 547-555: dsigma0 = _sigma0 sqrt(1 - 1/k^2) and the blur
            # that takes the build's level i - 1 to i is dsigma0 k^i for i = 0 .. dog + 1, dog + 2 steps; with _sigma0 =
            # sigma0 k the first of them is sigma0 sqrt(k^2 - 1), the Hessian build's, and the list is one step longer.
            s0 = self.sigma0 * k
            dsigma0 = s0 * math.sqrt(1.0 - 1.0 / (k * k))
            self.top = self.dog + 2
            # :511-513: _level_ds = _level_min + dog = dog - 1 there, level dog here, is decimated into the next octave
            # (PyramidCU.cpp:1533).  dog_ds_above: the WRONG rule (one level up).
            self.level_ds = self.dog + (1 if self.wrong["dog_ds_above"] else 0)
        else:
            dsigma0 = self.sigma0 * math.sqrt(k * k - 1.0)
            self.top = self.dog + 1
            self.level_ds = self.dog
        self.nlev = self.top + 1
        self.inter = [dsigma0 * k ** i for i in range(self.top)]                     # SiftGPU.cpp:547-556
        self.single = self.max_orientation == 1                                     # ProgramCU.cu:1398
        # the two-slot branch of the build without GPU_HESSIAN runs for every max_orientation > 1 (:1398, 1491-1549)
        self.two_peaks = self.is_dog and not self.single and not self.fixed_orientation

    # -- schedule ---------------------------------------------------------------------------------------------------
    def level_sigma(self, l):
        """GetLevelSigma, SiftGPU.cpp:1422-1425.  DoG: the build's level l - 1 with _sigma0 = sigma0 2^(1/dog):
        sigma0 2^(1/dog) 2^((l - 1)/dog), the same number."""
        return self.sigma0 * 2.0 ** (l / self.dog)

    def orient_sigma(self, l):
        """The sigma handed to ComputeOrientation for list level l (PyramidCU.cpp:1825-1848).  DoG: the loop counts
        level = 0 .. dog - 1 for list levels 1 .. dog and asks GetLevelSigma(level + _level_min + 1) = GetLevelSigma(l - 1) of
        the build's numbering, level l here.  dog_sigma_off: the WRONG rule that forgets _sigma0's factor 2^(1/dog)."""
        return self.level_sigma(l - 1 if self.is_dog and self.wrong["dog_sigma_off"] else l)

    def initial_sigma(self, octave_min):
        """GetInitialSmoothSigma, SiftGPU.cpp:482-489: 0 = no blur when sa <= sb + 0.001.  PROJECT: 'no blur' leaves
        the plane as it is; the reference would build a 5-tap table from sigma = 0, which is NaN (ProgramCU.cu:440-445).
        DoG: sa = _sigma0 2^(_level_min / dog) = sigma0 2^(1/dog) 2^(-1/dog), the sigma of level 0 here as well."""
        sa, sb = self.sigma0, self.sigman / 2.0 ** octave_min
        if sa > sb + 0.001:
            return math.sqrt(sa * sa - sb * sb)
        return math.sqrt(abs(sa * sa - sb * sb)) if self.wrong["no_skip"] else 0.0

    def taps(self, sigma):
        return filter_taps(sigma, self.fwf, clamp33=not self.wrong["no_clamp33"])

    def level_taps(self, l, octave_min=0):
        """Taps of the blur that produces level l (l = 0: the first blur; None when it is skipped)."""
        if l == 0:
            s = self.initial_sigma(octave_min)
            return self.taps(s) if s > 0 else None
        return self.taps(self.inter[l - 1])

    # -- geometry: GLTexImage.cpp:933-982 (ds on input), PyramidCU.cpp:113-176 (InitPyramid), :232-310 -----------------
    def plan(self, w, h):
        """-> (ds, octave_min, [(aligned width, height)], [scale of every octave]).  ds: log2 of the decimation on input;
        octave_min < 0: log2 of the up-sampling.  A pyramid that would still begin below the input's resolution after the
        -ads stepping (octave_min > 0 with ds == 0) does not occur for inputs that fit tex_max_dim and is not modelled."""
        fo, ds = self.first_octave, 0
        ws, hs = w, h
        if fo > 0:                                                                   # _PreProcessOnCPU = 1, GlobalUtil.cpp:79
            ds, ws, hs = fo, w >> fo, h >> fo
        while ws > self.maxd or hs > self.maxd:
            if not self.ads:
                raise ValueError("too big without auto_downscale")
            ds, ws, hs = ds + 1, ws >> 1, hs >> 1
        if ds == 0:
            w &= ~3
            fo = max(-3, fo)                                                         # "can't upsample by more than 8", :132
            wp, hp = (w << -fo, h << -fo) if fo < 0 else (w, h)
            omin = fo
        else:
            omin, wp, hp = 0, (w >> ds) & ~3, h >> ds
        while wp > self.maxd or hp > self.maxd:                                      # :154-166, whatever the sign of omin
            if not self.ads:
                raise ValueError("too big without auto_downscale")
            omin, wp, hp = omin + 1, wp >> 1, hp >> 1
        assert not (omin > 0 and ds == 0)
        nmax = max(1, int(math.floor(math.log(min(wp, hp)) / math.log(2.0))) - 3)    # :238-245
        # PROJECT: an octave_num beyond the automatic count is capped to it (the reference would allocate empty octaves)
        n = self.octave_num if 1 <= self.octave_num < nmax else nmax
        geo, scales = [], []
        sc = 2.0 ** (omin + ds)
        for _ in range(n):
            geo.append((((wp + 3) // 4) * 4, hp))
            scales.append(sc)
            wp, hp, sc = wp >> 1, hp >> 1, sc * 2
        return ds, omin, geo, scales

    def base_plane(self, img, fmt=None):
        """-> (level 0 of the first octave BEFORE the first blur, taps of the first blur or None)."""
        a = np.asarray(img)
        ds, omin, _, _ = self.plan(a.shape[1], a.shape[0])
        lum = input_plane(a, fmt, ds, no_wrap=self.wrong["no_wrap"], float_clamp=self.wrong["float_clamp"],
                          float_div255=self.wrong["float_div255"])
        if omin < 0:
            lum = upsample(lum, -omin, clamp=self.wrong["upsample_clamp"])           # PyramidCU.cpp:1523-1524
        return lum, self.level_taps(0, omin + ds)

    # -- detection --------------------------------------------------------------------------------------------------
    @staticmethod
    def response_plane(g, g_below):
        """ComputeDOG_Kernel, ProgramCU.cu:598-637: D_l = G_l - G_(l-1), one binary32 subtraction per pixel (texC is the
        level, texP the one below it: `(gus - 1)->BindTexture(texP)`, :646-647).  PyramidCU.cpp:1593-1605 runs it for the
        build's levels 0 .. dog + 1, levels 1 .. dog + 2 here; level 0 has no level below it and no plane."""
        return np.asarray(g, dtype=np.float32) - np.asarray(g_below, dtype=np.float32)

    def scan_planes(self, l):
        """-> (centre, previous, next): the response planes list level l (1 .. dog) is sought in.  Hessian: det-H of levels
        l, l - 1, l + 1 (PyramidCU.cpp:1631-1646).  DoG: :1654-1668 starts `dog` and `key` at base + 2 for the first list
        level, so list level l has its centre in D_(l+1), between D_l and D_(l+2) -- while orientation and descriptor read
        the gradient of Gaussian level l (`got = base + 1`, :1825).  dog_plane_lower: the WRONG rule, centre D_l."""
        c = l + 1 if self.is_dog and not self.wrong["dog_plane_lower"] else l
        return c, c - 1, c + 1

    def scan(self, C, P, N, G):
        """The threshold is compared with the response as it is: a caller whose pixels have the amplitude A scales it by
        A^2 (by A in the DoG mode).  threshold_unscaled: the WRONG rule of a detector that brought 0 .. 255 responses to
        [0, 1] first, |r| / 255^2 (/ 255) against T -- stated here as T times that factor."""
        T = np.float32(self.T)
        if self.wrong["threshold_unscaled"]:
            T = np.float32(T * np.float32(255.0 if self.is_dog else 255.0 * 255.0))
        return scan_level(C, P, N, G, T, self.edge, self.subpixel, keep08=self.wrong["keep08"],
                          dog=self.is_dog, dog_sign_tests=self.wrong["dog_sign_tests"],
                          dog_type_lxx=self.wrong["dog_type_lxx"], pivot_relative=self.wrong["pivot_relative"])

    def packed_half(self, r):
        """The response as the list record packs it: binary16 of the binary32 r', inf beyond 65504 + half a step, subnormal
        steps of 2^-24 below 2^-14 (ProgramCU.cu:1574-1596, GlobalUtil.cpp:588-621).  half_saturates: the WRONG rule."""
        return f2h(r, saturate=self.wrong["half_saturates"])

    def reduce_first(self, counts):
        """Per-level counts (octave-major, ascending) -> counts kept after list generation and the first LimitFeatureCount.
        PyramidCU.cpp:1283-1345: -tc2 walks octaves and levels downwards, -tc2 and -tc3 stop generating lists once the
        running total EXCEEDS the threshold; SiftPyramid.cpp:224-277: -tc3 keeps levels from the bottom while the total is
        below the threshold, the others drop levels from the bottom while the rest still exceeds it."""
        c = list(counts)
        if self.fct <= 0 or self.method == TRUNC_TOPK:
            return c
        if self.method in (TRUNC_HIGHEST_1, TRUNC_LOWEST):
            order = range(len(c) - 1, -1, -1) if self.method == TRUNC_HIGHEST_1 else range(len(c))
            total = 0
            for i in order:
                if total > self.fct:
                    c[i] = 0
                total += c[i]
        return self.limit(c)

    def limit(self, c):
        c = list(c)
        if self.fct <= 0 or self.method == TRUNC_TOPK:
            return c
        if self.method == TRUNC_LOWEST:
            i = new = 0
            while new < self.fct and i < len(c):
                new += c[i]
                i += 1
            return c[:i] + [0] * (len(c) - i)
        total, i = sum(c), 0
        while total - c[i] > self.fct:
            total -= c[i]
            c[i] = 0
            i += 1
        return c

    def reduce_second(self, multi_counts):
        """After the multi-orientation reshape the counts are those of the FEATURES and LimitFeatureCount(1) runs again
        on them (SiftPyramid.cpp:140-147); not with -m 1, -ofix (no reshape) or top-K (:213-214)."""
        if self.wrong["no_second_pass"] or self.single or self.fixed_orientation:
            return list(multi_counts)
        return self.limit(multi_counts)

    def topk(self, responses):
        """responses of the whole list in list order -> sorted indices kept (PyramidCU.cpp:1881-1987): the K largest
        abs(half(r')); skipped when the list is shorter than K.  PROJECT: equal keys go to the lower list index (the
        reference's bitonic sort leaves their order to the network)."""
        n, K = len(responses), self.fct
        if self.method != TRUNC_TOPK or K <= 0 or n < K:
            return list(range(n))
        key = [abs(float(r)) if self.wrong["topk_float_key"] else abs(self.packed_half(r)) for r in responses]
        order = sorted(range(n), key=lambda i: (-key[i], -i if self.wrong["topk_tie_high"] else i))
        return sorted(order[:K])

    # -- orientation and export ---------------------------------------------------------------------------------------
    def key_geometry(self, l, row, col, dx, dy, ds):
        """ProgramCU.cu:1281-1298: position and scale of a detection in its octave.  key.x = ikey.x + 0.5f + offset.y is a
        binary32 sum, and the model has to take it as one: at x = 500 it is a multiple of 2^-15, and moving the centre of
        the orientation window by that much tilts a flat histogram peak by more than a 16-bit angle step (the votes change
        by 1e-5 of their size, one-sidedly, and the peak interpolation divides by 2 v - next - pre, a small share of v)."""
        s = self.orient_sigma(l)
        if self.subpixel:
            return float(np.float32(col + 0.5) + np.float32(dx)), float(np.float32(row + 0.5) + np.float32(dy)), s * self.sigma_step ** ds
        return col + 0.5, row + 0.5, s

    def rotations(self, grad, theta, x, y, s, user=False, info=None):
        """-> (angles handed to the descriptor in radians, un-mirrored; uncertain).  -ofix: 0 (num_orientation = 0, :1312).
        DoG with max_orientation > 1 (ProgramCU.cu:1534-1551, PyramidCU.cpp:766, 798-820): the two slots become 16-bit
        codes floor(fr * 65535), 65535 standing for 'none'; the first is expanded to a feature if it is not 'none', the
        second if, besides, it is neither 'none' nor equal to the first; the angle is code * 2 pi / 65535.  max_orientation
        1, -ofix and keypoint lists take the branches above it, which no build changes.  dog_angle8 and dog_four_peaks: the
        WRONG rules that keep the GPU_HESSIAN lines (:1430-1489)."""
        if self.fixed_orientation:
            return [0.0], False
        single = self.single or user
        two = self.two_peaks and not single and not self.wrong["dog_four_peaks"]
        rots, unc = orientations_ex(grad, theta, x, y, s, self.half, self.ogf, self.owf, single=single,
                                    fold_refresh=self.wrong["fold_refresh"], single_last=self.wrong["single_last"],
                                    two_peaks=two, info=info)
        if single:
            return [rots[0] / TEN_DEG], unc                                           # :1415
        steps = 65535.0 if self.is_dog and not self.wrong["dog_angle8"] else 255.0
        codes = []
        for rot in rots:
            fr = rot / 36.0
            if fr < 0:
                fr += 1.0
            codes.append(math.floor(fr * steps))                                      # :1481-1486 / :1538-1548
        if self.is_dog and not self.wrong["dog_angle8"]:
            if codes and codes[0] == 65535:
                codes = []
            codes = codes[:1] + [c for c in codes[1:] if c != 65535 and c != codes[0]]
        return [c * 2 * PI / steps for c in codes], unc                               # PyramidCU.cpp:764-766

    def export(self, xf, yf, sf, scale):
        """PyramidCU.cpp:1097-1122: fixed-point record -> host keypoint."""
        fx, fy, fs = fixed(xf, 10) / 1024.0, fixed(yf, 10) / 1024.0, (fixed(sf, 8) & 0xFFFF) / 256.0
        off = 0.0 if self.lowe_origin else 0.5
        if self.lowe_origin and self.wrong["lowe_before_scale"]:
            return scale * (fx - 1.0) + 0.5, scale * (fy - 1.0) + 0.5, scale * fs
        return scale * (fx - 0.5) + off, scale * (fy - 0.5) + off, scale * fs

    @staticmethod
    def mirrored(angle):
        return math.fmod(2 * PI - angle, 2 * PI)                                      # PyramidCU.cpp:1134

    def descriptor(self, grad, theta, x, y, s, angle):
        return descriptor_ex(grad, theta, x, y, s, angle, self.half, self.dwf, self.di, self.normalize,
                             empty_nan=self.wrong["empty_nan"])

    def planes(self, g, l):
        """-> (det-H, gradient, theta) of Gaussian level l (ComputeHessian_Kernel, ProgramCU.cu:523-595).  deth_clamp: the
        WRONG rule, replicated borders instead of the 1-D index."""
        return hessian_planes(g, self.level_sigma(l), clamp=self.wrong["deth_clamp"])

    # -- keypoint lists, PyramidCU.cpp:555-718 ------------------------------------------------------------------------
    def bin_key(self, s, scales):
        """-> index of the level (octave * dog + level - 1) a caller's keypoint of scale s is put on, as a list (one entry, or two where the
        catch-alls overlap a bin; the caller asks for exactly one): half a level
        step either side of the level's sigma, the first and the last level catching everything beyond."""
        step = 2.0 ** ((1.0 if self.wrong["whole_step"] else 0.5) / self.dog)
        s = float(s)
        hits = []
        for o, sc in enumerate(scales):
            for l in range(1, self.dog + 1):
                ls = float(np.float32(self.level_sigma(l) * sc))
                lo, hi = (ls, ls * step) if self.wrong["whole_step"] else (ls / step, ls * step)
                if lo <= s < hi or (s < lo and o == 0 and l == 1) or (s > hi and o == len(scales) - 1 and l == self.dog):
                    hits.append(o * self.dog + l - 1)
        return hits

    def user_key(self, x, y, s, scale):
        """-> fixed-point position and scale in the octave (PyramidCU.cpp:616-657)."""
        off = 0.0 if self.lowe_origin else 0.5
        fx, fy, fs = (x - off) / scale + 0.5, (y - off) / scale + 0.5, s / scale
        return (fixed(fx, 10) & 0xFFFFFF) / 1024.0, (fixed(fy, 10) & 0xFFFFFF) / 1024.0, (fixed(fs, 8) & 0xFFFF) / 256.0
