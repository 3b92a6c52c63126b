"""Input layouts on the GPU: row pitch, image stride and base offset on every input path of the product.

The product gets the pixels in one of the layouts of tests/input_layouts.py, every byte that is not a pixel poisoned; the
reference is always the CPU oracle on the PACKED copy of the same pixels, and everything is compared bit for bit (geometry,
raw detection list, keypoints, descriptors; for the kernels that read u8 pixels directly also every Gaussian, det-H and
gradient/theta plane of every octave).  tests/test_input_layouts.py shows, with the oracle, that every one of these cases
tells a reading that ignores pitch, image_stride or the offset, or takes padding for pixels, from the right one.

Which kernel read the pixels is asserted from the profile counters: "input" launches == 0 means gauss_first_kernel or
gauss_kernel<R, true, false> read the u8 pixels themselves (hess_schedule.hip, direct_u8), > 0 means convert_kernel did.
Contexts and references are shared between the tests of this file: a context that runs one layout after another is itself
part of what is tested (no stale layout in the pending run or the staging area).
"""
import numpy as np
import pytest

import detector_cases
import input_layouts as L
from hessgpu_amd import _abi
from hessgpu_amd.session import HessError
from oracle_lib import OracleSession
from parity_compare import compare_results

pytestmark = pytest.mark.gpu

NOISE_KW, COLOUR_KW = detector_cases.NOISE_KW, detector_cases.COLOUR_KW
FUSION_OFF = (dict(filter_width_factor=5.0), dict(dog_level_num=1))   # gauss_first_available / level_ds != 1 (hess_schedule.hip)
OPTIONS = {"default": {}, "first_octave 1": dict(first_octave=1), "first_octave -1": dict(first_octave=-1),
           "auto_downscale": dict(auto_downscale=1, tex_max_dim=64)}


def _key(kw):
    return tuple(sorted(kw.items()))


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    """One product context per set of parameters for the whole file, with the launch counters on."""
    made = {}

    def get(**kw):
        if _key(kw) not in made:
            made[_key(kw)] = gpu_ctx_factory(**kw)
            made[_key(kw)].profile_enable(True)
        return made[_key(kw)]

    return get


_refs = {}


def _reference(name, pixels, fmt, kw):
    """-> (oracle session that has run the packed pixels, its counts): computed once per (pixels, parameters), then only read."""
    key = (name, _key(kw))
    if key not in _refs:
        o = OracleSession(threads=4, keep_levels=True, **kw)      # (detector: the oracle's switch has the product's values)
        _refs[key] = (o, o.run(np.ascontiguousarray(pixels), fmt=fmt))
    return _refs[key]


def _bytes(g, batch):
    out = []
    for b in range(batch):
        k, d = g.fetch(b)
        out += [g.rawlist(b).tobytes(), k.tobytes(), d.tobytes()]
    return out


def _hand_over(g, lay, how):
    """Give the layout's buffer to the product through one entry point; -> feature counts."""
    if how == "run":                                   # pageable NumPy memory
        return g.run(L.view(lay), fmt=lay.fmt)
    import torch

    if how in ("run pinned", "submit pinned"):         # a strided view of a pinned torch tensor
        t = torch.from_numpy(lay.buf).pin_memory()
        v = L.view(lay, t.numpy())
        assert v.ctypes.data == t.data_ptr() + lay.offset
        if how == "run pinned":
            return g.run(v, fmt=lay.fmt)
        g.submit_host(v, fmt=lay.fmt)
        g.wait()                                       # (t stays alive until here)
    elif how == "submit pinned ptr":                   # the raw-pointer form (u8 luminance)
        t = torch.from_numpy(lay.buf).pin_memory()
        g.submit_host(ptr=t.data_ptr() + lay.offset, batch=lay.batch, height=lay.height, width=lay.width, pitch=lay.pitch,
                      image_stride=lay.image_stride)
        g.wait()
    else:                                              # a slice of a device tensor
        d = torch.from_numpy(lay.buf).to("cuda:0")
        torch.cuda.synchronize()
        args = (d.data_ptr() + lay.offset, lay.batch, lay.height, lay.width, lay.channels, lay.pix, lay.fmt)
        if how == "run_device":
            g.run_device(*args, pitch=lay.pitch, image_stride=lay.image_stride)
        else:
            assert how == "submit_device", how
            g.submit_device(*args, pitch=lay.pitch, image_stride=lay.image_stride)
            g.wait()
        del d
    return [g.count(b) for b in range(lay.batch)]


def _check(g, kw, pname, packed, lay, direct, stages=False, how="run", fmt=None, floor=1):
    """Run `lay` on `g` and compare with the oracle on the packed pixels; -> (profile of the run, result bytes)."""
    what = f"{pname} {lay.name} batch {lay.batch} poison {lay.poison:#x} via {how} {kw}"
    o, no = _reference(pname + (" x same" if lay.name == "same_image" else ""), L.reference_pixels(packed, lay.name), fmt, kw)
    assert min(no) >= floor, f"{what}: {no} features: the case would prove little"
    g.keep_levels(stages)
    g.profile_reset()
    ng = _hand_over(g, lay, how)
    prof = g.profile()
    print(what, "counts", ng, "launches: input", prof["input"]["launches"], "gauss_octave0", prof["gauss_octave0"]["launches"])
    compare_results(g, o, ng, no, what, stages)
    if direct is not None:
        assert (prof["input"]["launches"] == 0) == direct, f"{what}: convert_kernel launches {prof['input']['launches']}, direct u8 expected: {direct}"
    return prof, _bytes(g, lay.batch)


def _check_layout(g, kw, pname, packed, lname, direct, fmt=None, floor=1, **more):
    """The layout with poison 0xA5; `pad` again with 0x5A: the same bytes."""
    prof, res = _check(g, kw, pname, packed, L.build(packed, lname, 0xA5, fmt), direct, fmt=fmt, floor=floor, **more)
    if lname == "pad":
        _, res2 = _check(g, kw, pname, packed, L.build(packed, lname, 0x5A, fmt), direct, fmt=fmt, floor=floor, **more)
        assert res == res2, f"{pname} {lname}: the padding's bytes reach the results"
    return prof, res


# ---- gauss_first_kernel: u8 luminance, default parameters -------------------------------------------------------------

FIRST_CASES = [(w, h, lname) for (w, h) in L.NOISE_SIZES[:2] for lname in ("pad4", "pad", "side_by_side", "same_image", "roi_corner")]
FIRST_CASES.append((324, 73, "pad"))


@pytest.mark.parametrize("batch", [1, 2, 5])     # level-chain schedule; latency batch; level, pair and multi launches, copier delivery
@pytest.mark.parametrize("w,h,lname", FIRST_CASES)
def test_first_tile_kernel_reads_the_layout(ctx, w, h, lname, batch):
    g = ctx(**NOISE_KW)
    px = L.noise_batch(w, h, batch)
    _, res = _check_layout(g, NOISE_KW, f"noise {w}x{h}x{batch}", px, lname, direct=True, stages=True, floor=L.MIN_FEATURES_NOISE)
    if lname == "same_image":
        per = len(res) // batch
        for b in range(1, batch):
            assert res[b * per:(b + 1) * per] == res[:per], f"image {b} of the same image {batch} times differs from image 0"


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("off", FUSION_OFF, ids=lambda d: " ".join(f"{k}={v}" for k, v in d.items()))
def test_level0_kernel_reads_the_layout_when_the_first_tile_fusion_is_off(ctx, off, batch):
    """gauss_kernel<R, true, false>: tap radii the fused first tile is not instantiated for, or a schedule whose level 1
    is the down-sampling level.  That the fusion is off is asserted two ways.  Level 0 of octave 0 is in HBM without
    hess_debug_keep_levels (fused, it exists in LDS only and the dump is refused).  And with the other taps every level of
    octave 0 is a launch of its own, dog + 2 = 5 of them: one more than the default's launches in a batch of five; in a
    single image two more, because there the default also lets octave 0's top level ride with the other octaves' top levels,
    which needs the default tap counts as well."""
    kw = dict(NOISE_KW, **off)
    for (w, h) in L.NOISE_SIZES[:2]:
        px = L.noise_batch(w, h, batch)
        pname = f"noise {w}x{h}x{batch}"
        prof, _ = _check_layout(ctx(**kw), kw, pname, px, "pad", direct=True, stages=True)
        dflt, _ = _check(ctx(**NOISE_KW), NOISE_KW, pname, px, L.build(px, "pad"), direct=True, stages=True)
        n, n0 = prof["gauss_octave0"]["launches"], dflt["gauss_octave0"]["launches"]
        if "filter_width_factor" in off:
            assert n == 5 and n > n0, f"octave-0 launches {n}, default {n0}: the first-tile fusion is not off"
            if batch == 5:
                assert n == n0 + 1, f"octave-0 launches {n}, default {n0}"
        for g, k, fused in ((ctx(**kw), kw, False), (ctx(**NOISE_KW), NOISE_KW, True)):
            _check(g, k, pname, px, L.build(px, "pad"), direct=True, stages=False)
            if fused:
                with pytest.raises(HessError):
                    g.level(0, 0, 0, _abi.DBG_GAUSS)
            else:
                got, want = g.level(0, 0, 0, _abi.DBG_GAUSS), _reference(pname, px, None, k)[0].level(0, 0, 0, _abi.DBG_GAUSS)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("batch", [1, 5])
def test_dog_detector_stores_level_0_from_the_layout(ctx, batch):
    """detector=1: store0 in launch_gauss_first (level 0 is D_1's input)."""
    kw = dict(NOISE_KW, detector=_abi.DETECTOR_DOG)
    for (w, h) in L.NOISE_SIZES[:2]:
        _check_layout(ctx(**kw), kw, f"noise {w}x{h}x{batch}", L.noise_batch(w, h, batch), "pad", direct=True, stages=True)


# ---- fallback by alignment ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", L.NOISE_SIZES[:2])
@pytest.mark.parametrize("lname", ["odd_pitch", "odd_stride", "side_by_side_odd", "odd_base"])
def test_unaligned_u8_goes_through_convert_kernel(ctx, lname, w, h):
    """pitch, image_stride or device address no multiple of 4: not the uchar4 loads.  (side_by_side_odd at width 260 has an
    image stride of 260 bytes: aligned, read directly.)"""
    g = ctx(**NOISE_KW)
    px = L.noise_batch(w, h, 2)
    direct = lname == "side_by_side_odd" and w % 4 == 0
    hows = ("run_device", "submit_device") if lname == "odd_base" else ("run", "run_device")
    for how in hows:
        _check_layout(g, NOISE_KW, f"noise {w}x{h}x2", px, lname, direct=direct, stages=True, how=how, floor=L.MIN_FEATURES_NOISE)


# ---- convert_kernel with a layout ---------------------------------------------------------------------------------------

def test_u8_rgb_with_a_pitch_of_3w_plus_5(ctx):
    px, _ = L.colour_batch("u8 rgb", 2)
    h, w = px.shape[1:3]
    for poison in (0xA5, 0x5A):
        lay = L.custom(px, 0, 3 * w + 5, (3 * w + 5) * h, poison, tail=5, name="pitch 3w+5")
        _check(ctx(**COLOUR_KW), COLOUR_KW, "u8 rgb", px, lay, direct=False, stages=True, floor=L.MIN_FEATURES_COLOUR)


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("kind", [k for k in L.COLOUR_KINDS if k != "u8 rgb"])
def test_convert_kernel_reads_the_layout(ctx, kind, opt):
    """Every wide or multi-channel type; read step 2 (first_octave=1, and auto_downscale with tex_max_dim below the width)
    and up-sampling after the conversion (first_octave=-1)."""
    kw = dict(COLOUR_KW, **OPTIONS[opt])
    px, fmt = L.colour_batch(kind, 2)
    for lname in ("pad", "roi_corner"):
        _check_layout(ctx(**kw), kw, kind, px, lname, direct=False, fmt=fmt, stages=True,
                      floor=L.MIN_FEATURES_COLOUR if opt == "default" else 20)


# ---- every entry point --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lname", ["pad", "roi_corner"])
@pytest.mark.parametrize("how", ["run", "run pinned", "submit pinned", "submit pinned ptr", "run_device", "submit_device"])
def test_every_entry_point_takes_the_layout(ctx, how, lname):
    w, h = L.NOISE_SIZES[1]
    px = L.noise_batch(w, h, 5)
    _check_layout(ctx(**NOISE_KW), NOISE_KW, f"noise {w}x{h}x5", px, lname, direct=True, how=how, floor=L.MIN_FEATURES_NOISE)


# ---- the exact span -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["run", "run pinned"])
@pytest.mark.parametrize("lname", ["pad", "side_by_side", "roi_corner"])
def test_exactly_the_span_of_the_pixels_is_copied(ctx, lname, how):
    """hess_submit_host copies from the first pixel to the last one and nothing more: hess_last_input returns the caller's
    bytes of that span and refuses one byte more.  (Before, the span ended with the last row's padding: up to pitch - row
    bytes beyond a region of interest in the last row of an allocation, nearly a row beyond images side by side.)"""
    g = ctx(**NOISE_KW)
    w, h = L.NOISE_SIZES[0]
    px = L.noise_batch(w, h, 5)
    lay = L.build(px, lname)
    _check(g, NOISE_KW, f"noise {w}x{h}x5", px, lay, direct=True, how=how)
    n = L.span(lay)
    assert n == 4 * lay.image_stride + (h - 1) * lay.pitch + w
    assert np.array_equal(g.last_input(n), lay.buf[lay.offset:lay.offset + n])
    with pytest.raises(HessError) as e:
        g.last_input(n + 1)
    assert e.value.code == _abi.HESS_ERR_STATE and "no host input of that size is retained" in str(e.value)


# ---- refusals -----------------------------------------------------------------------------------------------------------

def _refusals():
    """(name, dtype, channels, pitch - row bytes or None, image_stride - pitch * h, device pointer offset, word in the message).
    Only arguments the check refuses before any device work."""
    return [("pitch below the row u8", np.uint8, 1, -1, 0, 0, "pitch"),
            ("pitch below the row u16 rgb", np.uint16, 3, -2, 0, 0, "pitch"),
            ("pitch below the row f32", np.float32, 1, -4, 0, 0, "pitch"),
            ("odd pitch u16", np.uint16, 1, 1, 0, 0, "pitch"),
            ("pitch % 4 == 2 f32", np.float32, 1, 2, 0, 0, "pitch"),
            ("odd image_stride u16", np.uint16, 1, 0, 1, 0, "image_stride"),
            ("image_stride % 4 == 2 f32 rgb", np.float32, 3, 0, 2, 0, "image_stride"),
            ("odd device pointer u16", np.uint16, 1, 0, 0, 1, "dev_pixels"),
            ("device pointer % 4 == 2 f32", np.float32, 1, 0, 0, 2, "dev_pixels")]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refused_layouts(ctx, case):
    import torch

    name, dtype, nch, dpitch, dstride, dptr, word = case
    g = ctx(**COLOUR_KW)
    w, h, b = 96, 80, 2
    isz = np.dtype(dtype).itemsize
    row = w * nch * isz
    pitch = row + dpitch
    stride = pitch * h + dstride
    host = np.zeros(b * (row + 8) * h + 64, np.uint8)            # larger than any reading of it
    dev = torch.zeros(len(host), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lay = L.custom(np.zeros((b, h, w, nch), dtype), 0, max(pitch, row), max(stride, row * h))   # (shape and types only)
    g.profile_reset()
    entries = ("run_device", "submit_device") if dptr else ("run_host", "submit_host", "run_device", "submit_device")
    for entry in entries:
        base = dev.data_ptr() if "device" in entry else host.ctypes.data
        rc = L.run_raw(g, entry, base, lay, offset=dptr, pitch=pitch, image_stride=stride)
        msg = g._f["last_error"](g._h).decode()
        assert rc == _abi.HESS_ERR_ARG and word in msg, f"{name} through hess_{entry}: {rc} {msg!r}"
    assert all(v["launches"] == 0 for v in g.profile().values()), "a refused call launched something"
    with pytest.raises(HessError):
        g.wait()                                                  # nothing was submitted
    if dptr:   # the same misaligned address as a HOST pointer is fine: host pixels are copied bytewise first
        px, fmt = L.colour_batch("u16 lum" if dtype == np.uint16 else "f32 lum", 2)
        _check(g, COLOUR_KW, "u16 lum" if dtype == np.uint16 else "f32 lum", px, L.custom(px, dptr, px[0, 0].nbytes, px[0].nbytes),
               direct=False)
    px, fmt = L.colour_batch("u8 rgb", 2)                         # and the context runs a packed image correctly
    o, no = _reference("u8 rgb", px, fmt, COLOUR_KW)
    g.keep_levels(False)
    compare_results(g, o, g.run(px), no, f"packed after {name}", stages=False)


def test_legal_layouts_stay_legal(ctx):
    """image_stride 0 and image_stride below pitch for wide pixels too (u8: the first-tile tests)."""
    for kind in ("u16 rgb", "f32 lum"):
        px, fmt = L.colour_batch(kind, 2)
        for lname in ("same_image", "side_by_side", "side_by_side_odd", "pad4"):
            _check_layout(ctx(**COLOUR_KW), COLOUR_KW, kind, px, lname, direct=False, fmt=fmt, floor=L.MIN_FEATURES_COLOUR)


# ---- float pixels beyond [0, 1] -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32 lum 0..255 defaults", "f32 rgb 0..255 defaults"])
def test_float_pixels_above_one_through_default_parameters(ctx, name):
    """Float pixels are taken as they come.  The default descriptor order (PIXEL) assumes luminance in [0, 1] and silently
    becomes INTERLEAVED for float pixels (hess_schedule.hip); the oracle states the same rule: bit-identical, packed and
    with a layout."""
    px = detector_cases.cases()[name].image[None]
    _check(ctx(), {}, name, px, L.custom(px, 0, px[0, 0].nbytes, px[0].nbytes, name="packed"), direct=False, stages=True, floor=100)
    _check_layout(ctx(), {}, name, px, "pad", direct=False, stages=True, floor=100)


# ---- one context, one layout after another ------------------------------------------------------------------------------

def test_context_reuse_across_layouts(gpu_ctx_factory):
    g = gpu_ctx_factory(**NOISE_KW)
    g.profile_enable(True)
    (w1, h1), (w2, h2) = L.NOISE_SIZES[0], L.NOISE_SIZES[2]
    a, b = L.noise_batch(w1, h1, 2), L.noise_batch(w2, h2, 2)
    _check(g, NOISE_KW, f"noise {w1}x{h1}x2", a, L.custom(a, 0, w1, w1 * h1, name="packed"), direct=False, stages=True)   # (251: odd pitch)
    _check(g, NOISE_KW, f"noise {w1}x{h1}x2", a, L.build(a, "pad"), direct=True, stages=True)
    _check(g, NOISE_KW, f"noise {w2}x{h2}x2", b, L.custom(b, 0, w2, w2 * h2, name="packed"), direct=True, stages=True)
    _check(g, NOISE_KW, f"noise {w2}x{h2}x2", b, L.build(b, "roi_corner"), direct=True, stages=True)
    _check(g, NOISE_KW, f"noise {w1}x{h1}x2", a, L.build(a, "roi_corner"), direct=True, stages=True, how="run_device")
    assert g.run(a) == _reference(f"noise {w1}x{h1}x2", a, None, NOISE_KW)[1]
