"""Input layouts on the CPU: the Python Session hands a strided array over uncopied, the oracle honours pitch, image_stride
and base, and every case of tests/input_layouts.py can tell a wrong reading of its buffer from the right one.

The last point is what makes tests/test_input_layouts_gpu.py evidence: a kernel that ignored one of the arguments -- took
the packed pitch, the packed image stride, the buffer's start, or the row's bytes for the pitch -- would return one of the wrong
readings computed here, and each of them differs from the right result in the bytes the GPU file compares.

Floors (stated in input_layouts.py, checked here): every image of every case has at least 40 features at 251x50, 260x49 and
324x73 and at least 60 at the 96x80 colour image, so that a comparison of empty lists proves nothing nowhere.
"""
import numpy as np
import pytest

import detector_cases
import input_layouts as L
from oracle_lib import OracleSession

BATCH = 2
# poison behind the buffer, so that a wrong reading stays inside memory the test owns (the longest one, the f32 bgr images
# side by side read with the packed image stride, ends 183 168 bytes behind its buffer)
SLACK = 1 << 18


def _pixel_cases():
    out = {}
    for w, h in L.NOISE_SIZES:
        out[f"u8 lum {w}x{h}"] = (L.noise_batch(w, h, BATCH), None, detector_cases.NOISE_KW, L.MIN_FEATURES_NOISE)
    for kind in L.COLOUR_KINDS:
        px, fmt = L.colour_batch(kind, BATCH)
        out[kind] = (px, fmt, detector_cases.COLOUR_KW, L.MIN_FEATURES_COLOUR)
    return out


PIXELS = _pixel_cases()
CASES = [(p, n) for p in PIXELS for n in L.NAMES if PIXELS[p][0].dtype == np.uint8 or n not in L.U8_ONLY]
_oracles = {}


def _oracle(kw):
    key = tuple(sorted(kw.items()))
    if key not in _oracles:
        _oracles[key] = OracleSession(threads=1, keep_levels=False, **kw)
    return _oracles[key]


def _results(o, batch):
    """Everything the GPU file compares bitwise, as one bytes object."""
    parts = [repr(o.geometry()).encode()]
    for b in range(batch):
        k, d = o.fetch(b)
        parts += [o.rawlist(b).tobytes(), k.tobytes(), d.tobytes()]
    return b"|".join(parts)


_packed = {}


def _packed_results(pname, lname):
    """The reference, computed once per pixel case: the oracle on the packed copy."""
    px, fmt, kw, floor = PIXELS[pname]
    key = (pname, lname == "same_image")
    if key not in _packed:
        o = _oracle(kw)
        counts = o.run(L.reference_pixels(px, lname), fmt=fmt)
        _packed[key] = (_results(o, len(px)), counts)
    return _packed[key]


def _raw(o, lay, buf, **wrong):
    """The oracle on the raw buffer (followed by SLACK bytes of poison) with the layout's arguments, some replaced."""
    big = np.concatenate([buf, np.full(SLACK, lay.poison, np.uint8)])
    rc = L.run_raw(o, "run_host", big.ctypes.data, lay, **wrong)
    assert rc == 0, rc
    return _results(o, lay.batch)


def _bytes_read(lay, pitch):
    """The bytes a reading with this pitch covers."""
    big = np.concatenate([lay.buf, np.full(SLACK, lay.poison, np.uint8)])
    return np.ndarray((lay.batch, lay.height, lay.row), np.uint8, buffer=big, offset=lay.offset,
                      strides=(lay.image_stride, pitch, 1)).copy()


@pytest.mark.parametrize("pname", list(PIXELS))
def test_floors(pname):
    px, fmt, kw, floor = PIXELS[pname]
    counts = _packed_results(pname, "pad")[1]
    print(pname, counts)
    assert min(counts) >= floor, counts
    # the GPU file also runs batches of five: seeds 1..5 of the noise sizes
    if fmt is None and px.ndim == 3 and px.dtype == np.uint8:
        counts = _oracle(kw).run(L.noise_batch(px.shape[2], px.shape[1], 5))
        print(pname, "batch of 5", counts)
        assert min(counts) >= floor, counts


@pytest.mark.parametrize("pname,lname", CASES)
def test_view_is_handed_over_uncopied_and_reproduces_packed(pname, lname):
    px, fmt, kw, _ = PIXELS[pname]
    lay = L.build(px, lname, fmt=fmt)
    v = L.view(lay)
    assert np.array_equal(v, L.reference_pixels(px, lname))
    o = _oracle(kw)
    seen = []
    real = o._f["run_host"]
    o._f["run_host"] = lambda *a: (seen.append(a), real(*a))[1]     # a spy on the bound entry point
    try:
        o.run(v, fmt=fmt)
    finally:
        o._f["run_host"] = real
    (_, ptr, w, h, pitch, stride, b, f, pix), = seen
    assert ptr.value == lay.buf.ctypes.data + lay.offset, f"{lname}: the view was copied"
    want_stride = lay.image_stride if lay.batch > 1 else lay.pitch * lay.height
    assert (w, h, pitch, stride, b, pix) == (lay.width, lay.height, lay.pitch, want_stride, lay.batch, lay.pix)
    assert _results(o, lay.batch) == _packed_results(pname, lname)[0], f"{lname}: differs from the packed run"


@pytest.mark.parametrize("pname", list(PIXELS))
def test_contiguous_array_takes_the_packed_numbers(pname):
    px, fmt, kw, _ = PIXELS[pname]
    a, b, h, w, pitch, stride, f, pix = OracleSession._describe(px, fmt)
    row = px[0, 0].nbytes
    assert a is px and (pitch, stride) == (row, row * h)
    if px.ndim == 3:    # one [H,W] image
        one = OracleSession._describe(px[0], fmt)
        assert one[0].ctypes.data == px.ctypes.data and one[1:6] == (1, h, w, row, row * h)


def test_what_cannot_be_described_is_copied():
    px = L.noise_batch(60, 20, 2)
    rgb = L.colour_batch("u8 rgb", 2)[0]
    f32 = L.colour_batch("f32 lum", 2)[0]
    odd = np.ndarray(f32.shape, np.float32, buffer=np.zeros(f32.nbytes * 2 + 8, np.uint8), offset=0,
                     strides=(f32.strides[0] + 2, f32.strides[1], 4))      # image stride no multiple of the itemsize
    for what, v in (("rows bottom-up", px[:, ::-1]), ("mirrored rows", px[:, :, ::-1]), ("every other pixel", px[:, :, ::2]),
                    ("a channel plane", rgb[..., 1]), ("channels reversed", rgb[..., ::-1]), ("images in reverse", px[::-1]),
                    ("transposed", px.transpose(0, 2, 1)), ("misaligned image stride", odd)):
        a, b, h, w, pitch, stride = OracleSession._describe(v, None)[:6]
        assert a.flags.c_contiguous and np.array_equal(a, v), what
        assert (pitch, stride) == (a[0, 0].nbytes, a[0].nbytes), what
        assert not np.shares_memory(a, v) or v.flags.c_contiguous, what


@pytest.mark.parametrize("pname,lname", CASES)
def test_wrong_readings_differ(pname, lname):
    """pitch off by one pixel, the packed image stride, the offset dropped, the padding read as pixels: whichever of them
    is another reading of this buffer gives another result; the poison byte changes the last one and never the right one."""
    px, fmt, kw, _ = PIXELS[pname]
    o = _oracle(kw)
    lay = L.build(px, lname, 0xA5, fmt=fmt)
    lay2 = L.build(px, lname, 0x5A, fmt=fmt)
    right = _packed_results(pname, lname)[0]
    assert _raw(o, lay, lay.buf) == right
    assert _raw(o, lay2, lay2.buf) == right, "the poison byte changes the right reading"
    caught = []
    for what, wrong in (("pitch + one pixel", dict(pitch=lay.pitch + lay.group)), ("pitch - one pixel", dict(pitch=lay.pitch - lay.group)),
                        ("packed image stride", dict(image_stride=lay.pitch * lay.height)), ("offset dropped", dict(offset=0))):
        (k, val), = wrong.items()
        if val == getattr(lay, k):
            continue                     # not another reading of this layout (pad4's image stride IS pitch * h; offset 0)
        assert _raw(o, lay, lay.buf, **wrong) != right, f"{lname}: reading with {what} is not told from the right one"
        caught.append(what)
    assert "pitch + one pixel" in caught and "pitch - one pixel" in caught
    if lname in ("pad", "odd_stride", "side_by_side", "side_by_side_odd", "same_image", "roi_corner"):
        assert "packed image stride" in caught
    if lname in ("pad", "odd_base", "roi_corner"):
        assert "offset dropped" in caught
    # the padding taken for pixels: the reading that takes the row's bytes for the pitch walks through the padding, so
    # the poison byte must change it (the oracle aligns the width down to a multiple of 4, so a few extra columns at the
    # right edge would not show: this reading puts the padding inside the image)
    if lay.pitch != lay.row:
        a, b = _raw(o, lay, lay.buf, pitch=lay.row), _raw(o, lay2, lay2.buf, pitch=lay.row)
        poisoned = not np.array_equal(_bytes_read(lay, lay.row), _bytes_read(lay2, lay.row))
        if lname in ("pad", "odd_pitch", "roi_corner"):
            assert poisoned
        if poisoned:
            assert a != right and b != right and a != b, f"{lname}: a reading through the padding does not see the poison"
            caught.append("padding as pixels")
    print(pname, lname, caught)
