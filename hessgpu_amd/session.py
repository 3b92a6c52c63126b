"""Thin object wrapper over one implementation of the C ABI (include/hess_abi.h).

`Session` owns one `hess_ctx*` and exposes the calls the parity tests and bench need with numpy
arrays at the edge.  It contains no arithmetic: every result comes out of the bound library.
"""
import ctypes as C

import numpy as np

from . import _abi


class HessError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hess error {code}: {msg}")
        self.code = code


_FMT_BY_CHANNELS = {1: _abi.FMT_LUM, 2: _abi.FMT_LUM_ALPHA, 3: _abi.FMT_RGB, 4: _abi.FMT_RGBA}
_PIX_BY_DTYPE = {np.dtype(np.uint8): _abi.PIX_U8, np.dtype(np.uint16): _abi.PIX_U16,
                 np.dtype(np.float32): _abi.PIX_F32}
_DESC_FORMATS = {"f32": _abi.DESC_FORMAT_F32, "u8": _abi.DESC_FORMAT_U8}


def rect_keys(rects):
    """(n, 4) array of x, y, width, height (top-left corner and size in image pixels) -> the KEYPOINT_DTYPE array that
    set_keypoints / run_keypoints take with _abi.KEYS_RECTANGLES: the width travels in `s`, the height in `o`."""
    r = np.asarray(rects, dtype=np.float32).reshape(-1, 4)
    keys = np.zeros(len(r), dtype=_abi.KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["s"], keys["o"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return keys


def make_params(fn_default, **overrides):
    p = _abi.HessParams()
    fn_default(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"hess_params has no field {k!r}")
        setattr(p, k, v)
    return p


class Session:
    """One context of one backend.  `fns` is the dict produced by _abi.bind()."""

    def __init__(self, fns, handle, params):
        self._f = fns
        self._h = handle
        self.params = params
        self._batch = 0
        if not handle:
            raise HessError(_abi.HESS_ERR_DEVICE, "context creation failed")

    def close(self):
        if self._h:
            self._f["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            msg = self._f["last_error"](self._h)
            raise HessError(rc, msg.decode() if msg else "")
        return rc

    @staticmethod
    def _describe(images, fmt):
        """-> (array that owns the pixels, batch, height, width, pitch, image_stride, format, pixel type).  An array whose
        rows are contiguous runs of pixels is handed over as it lies in memory, with its own row pitch and image stride (a
        region of interest of larger frames, padded rows, images side by side, one image repeated); anything else -- a
        negative or misaligned stride, a channel axis that is not contiguous -- is copied into the packed layout."""
        a = np.asarray(images)
        if a.dtype not in _PIX_BY_DTYPE:
            raise TypeError(f"unsupported pixel dtype {a.dtype}")
        if a.ndim == 2:
            a = a[None]
        if a.ndim not in (3, 4):   # [B,H,W] luminance or [B,H,W,C]
            raise ValueError("images must be [H,W], [B,H,W] or [B,H,W,C]")
        nch = 1 if a.ndim == 3 else a.shape[3]
        b, h, w = a.shape[:3]
        isz = a.dtype.itemsize
        row = w * nch * isz
        pitch, stride = a.strides[1], a.strides[0]
        rows_contiguous = a.strides[2] == nch * isz and (a.ndim == 3 or a.strides[3] == isz)
        if h == 1:
            pitch = row        # (a dimension of one element has no stride of its own)
        if b == 1:
            stride = pitch * h
        if not (a.size and rows_contiguous and pitch >= row and stride >= 0 and pitch % isz == 0 and stride % isz == 0
                and pitch < 2 ** 31):
            a = np.ascontiguousarray(a)
            pitch, stride = row, row * h
        fmt = fmt or _FMT_BY_CHANNELS[nch]
        return a, b, h, w, pitch, stride, fmt, _PIX_BY_DTYPE[a.dtype]

    @staticmethod
    def _layout(width, height, channels, pixtype, pitch, image_stride):
        """pitch / image_stride of a raw pointer: None means packed rows / images back to back."""
        isz = {_abi.PIX_U8: 1, _abi.PIX_U16: 2, _abi.PIX_F32: 4}[pixtype]
        pitch = width * channels * isz if pitch is None else pitch
        return pitch, pitch * height if image_stride is None else image_stride

    # -- the path ------------------------------------------------------------------------
    def run(self, images, fmt=None):
        """Host pixels -> features (SiftGPU::RunSIFT(w,h,data,fmt,type) for a batch)."""
        a, b, h, w, pitch, stride, fmt, pix = self._describe(images, fmt)
        self._check(self._f["run_host"](self._h, a.ctypes.data_as(C.c_void_p), w, h, pitch, stride,
                                        b, fmt, pix))
        self._batch = b
        return [self.count(i) for i in range(b)]

    def run_device(self, dev_ptr, batch, height, width, channels=1, pixtype=_abi.PIX_U8, fmt=None, pitch=None,
                   image_stride=None):
        """Pixels already in HBM (raw device pointer, e.g. torch tensor .data_ptr()); pitch / image_stride in bytes,
        None = packed."""
        fmt = fmt or _FMT_BY_CHANNELS[channels]
        pitch, image_stride = self._layout(width, height, channels, pixtype, pitch, image_stride)
        self._check(self._f["run_device"](self._h, C.c_void_p(dev_ptr), width, height, pitch,
                                          image_stride, batch, fmt, pixtype))
        self._batch = batch

    def submit_device(self, dev_ptr, batch, height, width, channels=1, pixtype=_abi.PIX_U8, fmt=None, pitch=None,
                      image_stride=None):
        """Asynchronous half of run_device: enqueue on the context's stream and return."""
        fmt = fmt or _FMT_BY_CHANNELS[channels]
        pitch, image_stride = self._layout(width, height, channels, pixtype, pitch, image_stride)
        self._check(self._f["submit_device"](self._h, C.c_void_p(dev_ptr), width, height, pitch,
                                             image_stride, batch, fmt, pixtype))
        self._batch = batch

    def submit_host(self, images=None, fmt=None, ptr=None, batch=None, height=None, width=None, pitch=None,
                    image_stride=None):
        """Asynchronous half of run(): host pixels (a numpy array, or a raw host pointer `ptr` to `batch` u8
        luminance images, e.g. a pinned torch tensor's .data_ptr(), rows `pitch` and images `image_stride` bytes apart,
        None = packed) -> enqueue transfer + path, return."""
        if ptr is not None:
            pitch, image_stride = self._layout(width, height, 1, _abi.PIX_U8, pitch, image_stride)
            self._check(self._f["submit_host"](self._h, C.c_void_p(ptr), width, height, pitch, image_stride, batch,
                                               _abi.FMT_LUM, _abi.PIX_U8))
            self._batch = batch
            return
        a, b, h, w, pitch, stride, fmt, pix = self._describe(images, fmt)
        self._check(self._f["submit_host"](self._h, a.ctypes.data_as(C.c_void_p), w, h, pitch, stride, b, fmt, pix))
        self._batch = b

    def wait(self):
        """Block until the submitted batch's keypoints and descriptors are in host memory."""
        self._check(self._f["wait"](self._h))

    def set_keypoints(self, keys, have_orientation=True):
        """SiftGPU::SetKeypointList: the next run() of ONE image uses these keypoints, no detection.
        have_orientation: False / _abi.KEYS_NONE (the orientation is computed), True / _abi.KEYS_ORIENTED (the keys' own),
        or _abi.KEYS_RECTANGLES (-1): the keys are rectangles (rect_keys) and each gets a 4 x 4-cell gradient histogram over
        its rectangle (include/hess_abi.h, HESS_KEYS_RECTANGLES); the keys come back as given."""
        k = np.ascontiguousarray(keys, dtype=_abi.KEYPOINT_DTYPE)
        self._check(self._f["set_keypoints"](self._h, k.ctypes.data_as(C.c_void_p), len(k), int(have_orientation)))

    def run_keypoints(self, keys, have_orientation=True):
        """SiftGPU::RunSIFT(num, keys, flag): orientation/descriptors for `keys` on the current image; have_orientation
        as for set_keypoints, _abi.KEYS_RECTANGLES included."""
        k = np.ascontiguousarray(keys, dtype=_abi.KEYPOINT_DTYPE)
        self._check(self._f["run_keypoints"](self._h, k.ctypes.data_as(C.c_void_p), len(k), int(have_orientation)))
        return self.count(0)

    @staticmethod
    def _key_lists(keys_per_image):
        """A sequence of KEYPOINT_DTYPE arrays, one per image -> (the keys back to back, the counts as a C array)."""
        lists = [np.ascontiguousarray(k, dtype=_abi.KEYPOINT_DTYPE).reshape(-1) for k in keys_per_image]
        allk = np.concatenate(lists) if lists else np.zeros(0, dtype=_abi.KEYPOINT_DTYPE)
        return np.ascontiguousarray(allk), (C.c_int * len(lists))(*[len(k) for k in lists])

    def set_keypoints_batch(self, keys_per_image, have_orientation=True):
        """hess_set_keypoints_batch: one keypoint list per image of the next run() / submit_*(), whose batch must be
        len(keys_per_image); an empty list gives that image no results.  have_orientation as for set_keypoints (product
        only).  Rectangles: rect_keys per image with _abi.KEYS_RECTANGLES."""
        k, counts = self._key_lists(keys_per_image)
        self._check(self._f["set_keypoints_batch"](self._h, k.ctypes.data_as(C.c_void_p), counts, len(counts),
                                                   int(have_orientation)))

    def run_keypoints_batch(self, keys_per_image, have_orientation=True):
        """hess_run_keypoints_batch: the lists on the current batch (one per image of the last run), without rebuilding its
        pyramids -> the counts (product only)."""
        k, counts = self._key_lists(keys_per_image)
        self._check(self._f["run_keypoints_batch"](self._h, k.ctypes.data_as(C.c_void_p), counts, len(counts),
                                                   int(have_orientation)))
        self._batch = len(counts)
        return [self.count(i) for i in range(len(counts))]

    def key_list_order(self, img=0):
        """After a keypoint-list run: int32 array, list position -> input index, of image img's list -- the order of its
        records in device_results() (level, then input index; product only, hess_key_list_order)."""
        n = self._check(self._f["key_list_order"](self._h, img, None, 0))
        out = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self._f["key_list_order"](self._h, img, out.ctypes.data_as(C.c_void_p), n))
        return out

    def debug_key_levels(self, levels=None):
        """Parity hook: explicit level index per user keypoint for the following set/run_keypoints (None clears)."""
        if levels is None:
            self._check(self._f["debug_key_levels"](self._h, None, 0))
            return
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        self._check(self._f["debug_key_levels"](self._h, lv.ctypes.data_as(C.c_void_p), len(lv)))

    def reserve(self, width, height, batch):
        self._check(self._f["reserve"](self._h, width, height, batch))

    def count(self, img=0):
        return self._check(self._f["count"](self._h, img))

    def desc_dim(self):
        return self._check(self._f["desc_dim"](self._h))

    def set_descriptor_format(self, fmt):
        """"f32" (the default) or "u8": what the following runs store per descriptor element (product only;
        hess_set_descriptor_format).  Bytes are the matcher's quantisation of the floats, made by the descriptor kernels."""
        if fmt not in _DESC_FORMATS:
            raise ValueError(f"descriptor format must be one of {sorted(_DESC_FORMATS)}, not {fmt!r}")
        self._check(self._f["set_descriptor_format"](self._h, _DESC_FORMATS[fmt]))

    def desc_format(self):
        """"f32" or "u8": the format of the last run's descriptors (product only)."""
        if "desc_format" not in self._f:
            return "f32"
        code = self._check(self._f["desc_format"](self._h))
        return next(k for k, v in _DESC_FORMATS.items() if v == code)

    def fetch(self, img=0):
        """-> (keys structured array [N], descriptors float32 [N, dim] -- uint8 [N, dim] after a "u8" run)."""
        n = self.count(img)
        dim = self.desc_dim()
        u8 = self.desc_format() == "u8"
        keys = np.zeros(n, dtype=_abi.KEYPOINT_DTYPE)
        desc = np.zeros((n, dim), dtype=np.uint8 if u8 else np.float32)
        self._check(self._f["fetch_u8" if u8 else "fetch"](self._h, img, keys.ctypes.data_as(C.c_void_p),
                                                           desc.ctypes.data_as(C.c_void_p) if dim else None))
        return keys, desc

    def geometry(self):
        ws = (C.c_int * 32)()
        hs = (C.c_int * 32)()
        n = self._check(self._f["geometry"](self._h, ws, hs))
        return [(ws[i], hs[i]) for i in range(n)]

    def level(self, img, octave, level, what):
        w, h = self.geometry()[octave]
        n = w * h * (2 if what == _abi.DBG_GOT else 1)
        out = np.zeros(n, dtype=np.float32)
        self._check(self._f["debug_level"](self._h, img, octave, level, what,
                                           out.ctypes.data_as(C.c_void_p)))
        return out.reshape(h, w, 2) if what == _abi.DBG_GOT else out.reshape(h, w)

    def rawlist(self, img=0):
        n = self._check(self._f["debug_list"](self._h, img, None, 0))
        out = np.zeros(n, dtype=_abi.RAWKEY_DTYPE)
        if n:
            self._check(self._f["debug_list"](self._h, img, out.ctypes.data_as(C.c_void_p), n))
        return out

    def timing(self):
        p = self._f["timing"](self._h)
        return np.array([p[i] for i in range(_abi.T_COUNT)], dtype=np.float32)

    def device_results(self):
        """-> (keys_ptr, desc_ptr, total): packed device results of the last run (product only); desc_ptr addresses
        float [total][dim], or uint8 [total][dim] after a "u8" run."""
        k, d, cap = C.c_void_p(), C.c_void_p(), C.c_int()
        self._check(self._f["device_results"](self._h, C.byref(k), C.byref(d), C.byref(cap)))
        return k.value, d.value, cap.value

    def last_input(self, nbytes):
        """The first `nbytes` bytes of the span the last run() / submit_host() handed over (product only; hess_last_input)."""
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self._f["last_input"](self._h, out.ctypes.data_as(C.c_void_p), nbytes))
        return out

    def keep_levels(self, on=True):
        """Product: also store the top Gaussian level of every octave (never materialised by default) so that
        level(..., DBG_GAUSS) can return it; the test oracle keeps all levels anyway."""
        if "debug_keep_levels" in self._f:
            self._check(self._f["debug_keep_levels"](self._h, int(on)))

    def regrown(self):
        """Times the context grew its feature storage after an overflow and ran the batch again (product only)."""
        return self._check(self._f["debug_regrown"](self._h))

    # -- node-shared result buffers (product only; hess_abi.h, hess_share_results) --------
    def share_results(self, name):
        """Keep this context's pinned result buffers in POSIX shared memory objects "/<name>.h|.k<n>|.d<n>" so that
        another process of the node reads them in place (dist.SharedResultsReader).  Before the first batch."""
        self._check(self._f["share_results"](self._h, name.encode()))

    def shared_results_info(self):
        """-> (gen_keys, gen_desc, keys_bytes, desc_bytes) of the shared result buffers."""
        gk, gd, kb, db = C.c_uint(), C.c_uint(), C.c_size_t(), C.c_size_t()
        self._check(self._f["shared_results_info"](self._h, C.byref(gk), C.byref(gd), C.byref(kb), C.byref(db)))
        return gk.value, gd.value, kb.value, db.value

    # -- profiling (product only) --------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self._f["profile_enable"](self._h, int(on)))

    def profile_reset(self):
        self._check(self._f["profile_reset"](self._h))

    def profile(self):
        out = {}
        for k, name in enumerate(_abi.KERNEL_NAMES):
            ms, n, by = C.c_double(), C.c_longlong(), C.c_double()
            self._check(self._f["profile_get"](self._h, k, C.byref(ms), C.byref(n), C.byref(by)))
            out[name] = {"ms": ms.value, "launches": n.value, "bytes": by.value}
            if "profile_get_in_lds" in self._f:   # bytes of the reference's layout that never left LDS (hess_abi.h)
                il = C.c_double()
                self._check(self._f["profile_get_in_lds"](self._h, k, C.byref(il)))
                out[name]["bytes_in_lds"] = il.value
        return out
