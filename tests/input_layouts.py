"""Memory layouts of one batch of pixels for the input-layout tests (a plain helper module: builders, no assertions).

build(packed, name, poison) lays the pixels of a packed [B,H,W] or [B,H,W,C] array out in a raw uint8 buffer as the C ABI
describes a layout (include/hess_abi.h, above hess_run_host): pixel (x, y) of image b starts at byte
offset + b * image_stride + y * pitch + x * channels * itemsize.  Every byte of the buffer that is not a pixel holds
`poison`.  view(layout) is the strided NumPy view of that buffer that Session.run hands over uncopied.

  name              pitch                          image_stride         offset
  pad4              row bytes rounded up to 4      pitch * h            0
  pad               that + 8                       pitch * h + 20       12
  odd_pitch         row bytes rounded up to 4, +1  pitch * h            0        u8 only
  odd_stride        as pad4                        pitch * h + 6        0        u8 only, batch >= 2
  odd_base          as pad4                        pitch * h            5        u8 only (device entry points)
  side_by_side      B * row4                       row4                 0        row4 = row bytes rounded up to 4
  side_by_side_odd  B * row bytes                  row bytes            0
  same_image        as pad4                        0                    0        image 0 alone is in the buffer
  roi_corner        frame 24 pixels wider and 9 rows taller (its row bytes rounded up to 4), image_stride one frame; the ROI
                    is the bottom-right corner of each frame, and the last frame's last row ends at the buffer's last byte

For 16-bit and float pixels every pad, offset and stride above is a multiple of 4, hence of the itemsize.  The buffers end
with the last row's padding (pitch - row bytes), except side_by_side*, whose last row ends with the last image, and
roi_corner: there the buffer ends with the last pixel, which is what a region of interest in the last row of an allocation
looks like.
"""
from types import SimpleNamespace

import numpy as np

from hessgpu_amd import _abi

NAMES = ("pad4", "pad", "odd_pitch", "odd_stride", "odd_base", "side_by_side", "side_by_side_odd", "same_image", "roi_corner")
U8_ONLY = ("odd_pitch", "odd_stride", "odd_base")
ROI_DX, ROI_DY = 24, 9

PIX = {np.dtype(np.uint8): _abi.PIX_U8, np.dtype(np.uint16): _abi.PIX_U16, np.dtype(np.float32): _abi.PIX_F32}
FMT = {1: _abi.FMT_LUM, 2: _abi.FMT_LUM_ALPHA, 3: _abi.FMT_RGB, 4: _abi.FMT_RGBA}


NOISE_SIZES = ((251, 50), (260, 49), (324, 73))   # 251: wa = 248 in a 252-byte pitch; each has several 64x32 tiles, a ragged last one
COLOUR_KINDS = ("u8 rgb", "u8 rgba", "u16 lum", "u16 rgb", "f32 lum", "f32 bgr")
MIN_FEATURES_NOISE, MIN_FEATURES_COLOUR = 40, 60      # per image; tests/test_input_layouts.py checks them with the oracle


def noise_batch(w, h, batch):
    """u8 luminance noise, seeds 1 .. batch (detector_cases.noise; run it with detector_cases.NOISE_KW)."""
    import detector_cases

    return np.stack([detector_cases.noise(w, h, seed) for seed in range(1, batch + 1)])


def colour_batch(kind, batch=2, w=96, h=80):
    """-> (pixels [B,H,W(,C)], format or None) of detector_cases.colour, seeds 3 .., as one of COLOUR_KINDS (run it with
    detector_cases.COLOUR_KW)."""
    import detector_cases

    c = np.stack([detector_cases.colour(w, h, seed) for seed in range(3, 3 + batch)])
    if kind == "u8 rgb":
        return c, None
    if kind == "u8 rgba":
        return np.concatenate([c, np.full(c.shape[:3] + (1,), 255, np.uint8)], axis=3), None
    if kind == "u16 lum":
        return c[..., 1].astype(np.uint16) * 257, None
    if kind == "u16 rgb":
        return c.astype(np.uint16) * 257, None
    if kind == "f32 lum":
        return (c[..., 1] / 255.0).astype(np.float32), None
    if kind == "f32 bgr":
        return (c[..., ::-1] / 255.0).astype(np.float32), _abi.FMT_BGR
    raise ValueError(kind)


def _up4(n):
    return (n + 3) // 4 * 4


def span(lay):
    """Bytes from the first pixel to the last one: what an entry point may touch, and hess_last_input retains."""
    return (lay.batch - 1) * lay.image_stride + (lay.height - 1) * lay.pitch + lay.row


def custom(packed, offset, pitch, image_stride, poison=0xA5, tail=0, name="custom"):
    """The pixels of `packed` at an explicit (offset, pitch, image_stride); `tail` poison bytes after the last pixel.
    image_stride 0: only image 0 is stored."""
    packed = np.ascontiguousarray(packed)
    if packed.ndim == 3:
        packed = packed[..., None]
    b, h, w, nch = packed.shape
    isz = packed.dtype.itemsize
    row = w * nch * isz
    lay = SimpleNamespace(name=name, offset=offset, pitch=pitch, image_stride=image_stride, batch=b, height=h, width=w,
                          channels=nch, dtype=packed.dtype, row=row, group=nch * isz, pix=PIX[packed.dtype], fmt=FMT[nch],
                          poison=poison)
    buf = np.full(offset + span(lay) + tail, poison, dtype=np.uint8)
    raw = packed.view(np.uint8).reshape(b, h, row)
    for i in range(b if image_stride or b == 1 else 1):
        for y in range(h):
            at = offset + i * image_stride + y * pitch
            buf[at:at + row] = raw[i, y]
    lay.buf = buf
    return lay


def build(packed, name, poison=0xA5, fmt=None):
    """-> layout: .buf (uint8), .offset, .pitch, .image_stride and the shape; see the table in the module's docstring."""
    packed = np.ascontiguousarray(packed)
    b, h, w = packed.shape[:3]
    nch = 1 if packed.ndim == 3 else packed.shape[3]
    isz = packed.dtype.itemsize
    row = w * nch * isz
    row4 = _up4(row)
    if name in U8_ONLY and isz != 1:
        raise ValueError(f"layout {name} is for u8 pixels only")
    if name == "pad4":
        offset, pitch, stride, tail = 0, row4, row4 * h, row4 - row
    elif name == "pad":
        offset, pitch, stride, tail = 12, row4 + 8, (row4 + 8) * h + 20, row4 + 8 - row
    elif name == "odd_pitch":
        offset, pitch, stride, tail = 0, row4 + 1, (row4 + 1) * h, row4 + 1 - row
    elif name == "odd_stride":
        if b < 2:
            raise ValueError("odd_stride needs a batch of two or more")
        offset, pitch, stride, tail = 0, row4, row4 * h + 6, row4 - row
    elif name == "odd_base":
        offset, pitch, stride, tail = 5, row4, row4 * h, row4 - row
    elif name == "side_by_side":
        offset, pitch, stride, tail = 0, b * row4, row4, 0
    elif name == "side_by_side_odd":
        offset, pitch, stride, tail = 0, b * row, row, 0
    elif name == "same_image":
        offset, pitch, stride, tail = 0, row4, 0, row4 - row
    elif name == "roi_corner":
        pitch = _up4((w + ROI_DX) * nch * isz)
        offset, stride, tail = ROI_DY * pitch + ROI_DX * nch * isz, pitch * (h + ROI_DY), 0
    else:
        raise ValueError(f"unknown layout {name!r}")
    lay = custom(packed, offset, pitch, stride, poison, tail, name)
    lay.fmt = fmt or lay.fmt
    return lay


def reference_pixels(packed, name):
    """The packed batch whose results the layout must reproduce: `packed` itself, or image 0 `batch` times (same_image)."""
    packed = np.ascontiguousarray(packed)
    return np.ascontiguousarray(np.repeat(packed[:1], len(packed), axis=0)) if name == "same_image" else packed


def view(lay, buf=None):
    """The strided view [B,H,W] / [B,H,W,C] on the layout's buffer (or on `buf`, a buffer of the same layout elsewhere,
    e.g. pinned memory)."""
    buf = lay.buf if buf is None else buf
    isz = lay.dtype.itemsize
    shape, strides = (lay.batch, lay.height, lay.width), (lay.image_stride, lay.pitch, lay.group)
    if lay.channels > 1:
        shape, strides = shape + (lay.channels,), strides + (isz,)
    return np.ndarray(shape, dtype=lay.dtype, buffer=buf, offset=lay.offset, strides=strides)


def run_raw(session, entry, base, lay, offset=None, pitch=None, image_stride=None, width=None):
    """Call a run_* / submit_* entry point of `session` on address `base` + offset with the layout's arguments, any of them
    replaced: how the tests hand over a raw pointer, and how they read a buffer wrongly on purpose.  -> return code."""
    import ctypes as C

    return session._f[entry](session._h, C.c_void_p(base + (lay.offset if offset is None else offset)),
                             lay.width if width is None else width, lay.height, lay.pitch if pitch is None else pitch,
                             lay.image_stride if image_stride is None else image_stride, lay.batch, lay.fmt, lay.pix)
