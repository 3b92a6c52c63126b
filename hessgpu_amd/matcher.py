"""ctypes wrapper of the descriptor matcher entry points (hess_matcher_* in include/hess_abi.h):
the SiftMatchGPU surface of the reference (SetDescriptors / SetFeatureLocation / GetSiftMatch /
GetGuidedSiftMatch).  Plumbing only; the work happens in libhessgpu.so on the GPU."""
import ctypes as C

import numpy as np

from . import _abi, load_library
from .session import HessError

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        L.hess_matcher_create.restype = C.c_void_p
        L.hess_matcher_create.argtypes = [C.c_int, C.c_int]
        L.hess_matcher_destroy.argtypes = [C.c_void_p]
        L.hess_matcher_set_max.argtypes = [C.c_void_p, C.c_int]
        L.hess_matcher_set_dim.argtypes = [C.c_void_p, C.c_int]
        L.hess_matcher_dim.argtypes = [C.c_void_p]
        L.hess_matcher_set_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.hess_matcher_set_descriptors_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.hess_matcher_set_locations.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.hess_matcher_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                         C.c_float, C.c_float, C.c_float, C.c_int]
        L.hess_matcher_bank_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hess_matcher_bank_set_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hess_matcher_bank_set_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hess_matcher_bank_set_device_u8.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hess_matcher_bank_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.hess_matcher_match_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_float, C.c_float, C.c_int]
        L.hess_matcher_match_pairs_guided.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_void_p, C.c_float, C.c_float, C.c_int]
        L.hess_matcher_set_types.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.hess_matcher_bank_set_types.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hess_matcher_bank_set_types_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hess_geom_sample.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.hess_matcher_estimate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hess_matcher_bank_set_locations.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hess_matcher_bank_set_locations_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.hess_matcher_estimate_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.hess_matcher_verify_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.hess_matcher_last_ms.restype = C.c_float
        L.hess_matcher_last_ms.argtypes = [C.c_void_p]
        L.hess_matcher_last_error.restype = C.c_char_p
        L.hess_matcher_last_error.argtypes = [C.c_void_p]
        _bound = True
    return L


def all_pairs(n):
    """Every pair (i, j), i < j, of n sets: [n (n - 1) / 2, 2] int32."""
    i, j = np.triu_indices(int(n), 1)
    return np.stack([i, j], 1).astype(np.int32)


def window_pairs(n, w):
    """Every pair (i, j) of n sets with i < j <= i + w (a sequence matched against its w successors)."""
    out = [(i, j) for i in range(int(n)) for j in range(i + 1, min(int(n), i + int(w) + 1))]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def check_pairs(pairs):
    """-> C-contiguous int32 [n, 2] of (a, b) bank indices; ValueError for a wrong shape or dtype or a negative index."""
    a = np.asarray(pairs)
    if a.size == 0 and a.ndim <= 2 and (a.ndim < 2 or a.shape[1] in (0, 2)):
        return np.zeros((0, 2), dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"pairs must have shape [n, 2], not {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"pairs must be integers, not {a.dtype}")
    if a.size and (a.min() < 0 or a.max() > np.iinfo(np.int32).max):
        raise ValueError("pair indices must lie in 0 .. 2^31 - 1")
    return np.ascontiguousarray(a, dtype=np.int32)


DIMS = (128, 64)

# hess_geom_params / hess_geom_result (include/hess_abi.h).  Word 0 of the params' reserved[] is `refit`; words 0 and 1 of the
# result's reserved[] are `refits` and `ransac_inliers` (the field names stay those of the arrays).
GEOM_MODELS = {"H": 1, "F": 2, "homography": 1, "fundamental": 2, 1: 1, 2: 2}
GEOM_PARAMS_DTYPE = np.dtype([("model", "<i4"), ("hypotheses", "<i4"), ("seed", "<u4"), ("bound", "<f4"), ("reserved", "<i4", 4)])
GEOM_RESULT_DTYPE = np.dtype([("M", "<f4", 9), ("inliers", "<i4"), ("hypothesis", "<i4"), ("reserved", "<i4", 2)])
assert GEOM_PARAMS_DTYPE.itemsize == 32 and GEOM_RESULT_DTYPE.itemsize == 52
# hess_guided_pair: the geometry of one pair of match_pairs_guided
GUIDED_PAIR_DTYPE = np.dtype([("H", "<f4", 9), ("F", "<f4", 9), ("hdistmax", "<f4"), ("fdistmax", "<f4")])
assert GUIDED_PAIR_DTYPE.itemsize == 80
GUIDED_OFF = 1.0e20  # the bound that switches a gate off (SiftMatchGPU::GetGuidedSiftMatch)
VERIFY_PARAMS_DTYPE, VERIFY_RESULT_DTYPE = _abi.VERIFY_PARAMS_DTYPE, _abi.VERIFY_RESULT_DTYPE  # hess_matcher_verify_pairs
assert VERIFY_PARAMS_DTYPE["geom"] == GEOM_PARAMS_DTYPE and VERIFY_RESULT_DTYPE["putative"] == GEOM_RESULT_DTYPE


def guided_pairs(n, H=None, F=None, hdistmax=32.0, fdistmax=16.0):
    """-> GUIDED_PAIR_DTYPE [n] from H, F ([n, 3, 3] or None) and the bounds (scalars or [n]).  One missing matrix is the
    identity with its bound at 1e20 (SiftMatchGPU::GetGuidedSiftMatch's rule); both missing, a wrong shape, a non-numeric
    dtype or a count other than n: ValueError."""
    if H is None and F is None:
        raise ValueError("guided matching needs H or F (match_pairs is the unguided call)")
    geo = np.zeros(int(n), dtype=GUIDED_PAIR_DTYPE)
    for name, mat, bound in (("H", H, hdistmax), ("F", F, fdistmax)):
        key = name.lower() + "distmax"
        if mat is None:
            geo[name] = np.eye(3, dtype=np.float32).reshape(9)
            geo[key] = GUIDED_OFF
            continue
        a = np.asarray(mat)
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{name} must be numbers, not {a.dtype}")
        if a.shape != (n, 3, 3):
            raise ValueError(f"{name} must have shape [{n}, 3, 3] (one matrix per pair), not {a.shape}")
        b = np.asarray(bound)
        if b.dtype.kind not in "fiu" or b.shape not in ((), (n,)):
            raise ValueError(f"{key} must be a number or {n} numbers, not {b.dtype} {b.shape}")
        geo[name] = a.astype(np.float32).reshape(n, 9)
        geo[key] = b.astype(np.float32)
    return geo


def geom_sample(seed, t, k, n):
    """The sampling rule of the estimator on the host (hess_geom_sample): the k indices of hypothesis t among n matches."""
    out = np.zeros(max(int(k), 1), dtype=np.int32)
    rc = _lib().hess_geom_sample(int(seed) & 0xffffffff, int(t), int(k), int(n), out.ctypes.data)
    if rc < 0:
        raise HessError(rc, f"hess_geom_sample refuses t = {t}, k = {k}, n = {n}")
    return out[:k].copy()


def _geom_params(model, bound, hypotheses, seed, refit=0):
    if model not in GEOM_MODELS:
        raise ValueError(f"model is 'H' or 'F', not {model!r}")
    p = np.zeros(1, dtype=GEOM_PARAMS_DTYPE)
    p["model"], p["hypotheses"], p["seed"], p["bound"] = GEOM_MODELS[model], int(hypotheses), int(seed) & 0xffffffff, bound
    p["reserved"][0, 0] = int(refit)
    return p


def _geom_info(res, k):
    return {"inliers": int(res["inliers"][k]), "refits": int(res["reserved"][k, 0]), "ransac_inliers": int(res["reserved"][k, 1])}


class Matcher:
    """dim: the descriptor length of every set this matcher takes, 128 or 64 (the -half descriptors of a
    HessContext(half_sift=1)).  64-d sets give what the same rows with 64 zero columns appended give at 128."""

    def __init__(self, device=0, max_sift=4096, dim=128):
        if dim not in DIMS:
            raise ValueError(f"the matcher takes 128-d or 64-d descriptors, not {dim}-d")
        self.L = _lib()
        self._dim = 128
        self.h = self.L.hess_matcher_create(device, max_sift)
        if not self.h:
            raise HessError(-3, f"hess_matcher_create failed on device {device}")
        if dim != 128:
            self.set_dim(dim)

    @property
    def dim(self):
        return self._dim

    def set_dim(self, dim):
        """Changing the length empties the bank, both single-pair slots and their locations."""
        self._check(self.L.hess_matcher_set_dim(self.h, int(dim)))
        self._dim = int(self.L.hess_matcher_dim(self.h))

    def close(self):
        if self.h:
            self.L.hess_matcher_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise HessError(rc, (self.L.hess_matcher_last_error(self.h) or b"").decode())
        return rc

    def set_descriptors(self, index, desc):
        d = np.ascontiguousarray(desc)
        if d.ndim == 2 and d.shape[1] != self.dim:
            raise ValueError(f"this matcher takes [n, {self.dim}] descriptors, not {d.shape}")
        if d.ndim != 2 and d.size % self.dim:
            raise ValueError(f"{d.size} values are no whole number of {self.dim}-d descriptors")
        if d.ndim != 2:
            d = d.reshape(-1, self.dim)
        if d.dtype == np.uint8:
            self._check(self.L.hess_matcher_set_descriptors(self.h, index, len(d), d.ctypes.data))
        else:
            d = np.ascontiguousarray(d, dtype=np.float32)
            self._check(self.L.hess_matcher_set_descriptors_f32(self.h, index, len(d), d.ctypes.data))

    def set_locations(self, index, loc, gap=0):
        a = np.ascontiguousarray(loc, dtype=np.float32)
        self._check(self.L.hess_matcher_set_locations(self.h, index, a.ctypes.data, gap))

    @staticmethod
    def _types(types):
        """-> (array that owns the memory, address, stride in bytes) of one u16 per feature.  A structured key array
        (HessContext.fetch) is read in place through its "type" field."""
        a = np.asarray(types)
        if a.dtype.names and "type" in a.dtype.names:
            a = a["type"]
        if a.dtype != np.uint16:
            if a.dtype.kind not in "iu":
                raise ValueError(f"feature types are integers (hess_keypoint.type), not {a.dtype}")
            a = (a.astype(np.int64) & 0xffff).astype(np.uint16)
        if a.ndim != 1:
            raise ValueError(f"feature types must be one value per feature, not an array of shape {a.shape}")
        if len(a) > 1 and (a.strides[0] < 2 or a.strides[0] % 2):
            a = np.ascontiguousarray(a)
        return a, a.ctypes.data, (a.strides[0] if len(a) > 1 else 2)

    def set_types(self, index, types):
        """The feature types (hess_keypoint.type: class = type & 3) of slot `index`, one per descriptor loaded there: with
        both slots typed, match() (unguided) pairs features of the same class only -- best, second best, ratio test and
        mutual best within the class.  None removes them; set_descriptors on the slot removes them too."""
        if types is None:
            self._check(self.L.hess_matcher_set_types(self.h, int(index), None, 2))
            return
        a, ptr, stride = self._types(types)
        if not len(a):
            a = np.zeros(1, np.uint16)      # (an address for a slot without descriptors: nothing is read)
            ptr = a.ctypes.data
        self._check(self.L.hess_matcher_set_types(self.h, int(index), ptr, stride))

    def match(self, max_match=4096, H=None, F=None, distmax=0.7, ratiomax=0.8, hdistmax=32.0, fdistmax=16.0,
              mutual_best=True):
        out = np.zeros((max(max_match, 1), 2), dtype=np.int32)
        h = np.ascontiguousarray(H, dtype=np.float32) if H is not None else None
        f = np.ascontiguousarray(F, dtype=np.float32) if F is not None else None
        n = self._check(self.L.hess_matcher_match(self.h, max_match, out.ctypes.data,
                                                  h.ctypes.data if h is not None else None,
                                                  f.ctypes.data if f is not None else None,
                                                  distmax, ratiomax, hdistmax, fdistmax, int(mutual_best)))
        return out[:n].copy()

    def last_ms(self):
        return float(self.L.hess_matcher_last_ms(self.h))

    # ---- bank of descriptor sets on the device, many pairs per call ----
    def set_bank(self, sets):
        """sets: a list of [n_i, dim] arrays, all u8 (stored as they are) or all float (quantised like
        set_descriptors)."""
        sets = [np.asarray(d) for d in sets]
        for d in sets:
            if d.ndim != 2 or d.shape[1] != self.dim:
                raise ValueError(f"a bank set must be [n, {self.dim}], not {d.shape}")
        counts = np.array([len(d) for d in sets], dtype=np.int32)
        u8 = all(d.dtype == np.uint8 for d in sets)
        dt = np.uint8 if u8 else np.float32
        flat = np.ascontiguousarray(np.concatenate(sets).astype(dt, copy=False) if sets else np.zeros((0, self.dim), dt))
        fn = self.L.hess_matcher_bank_set if u8 else self.L.hess_matcher_bank_set_f32
        self._check(fn(self.h, len(counts), counts.ctypes.data, flat.ctypes.data if flat.size else None))
        self._bank_sets = len(counts)

    def set_bank_device(self, ptr, counts, dtype=np.float32):
        """ptr: device address of float [sum(counts)][dim] on the matcher's device (quantised on the device), or with
        dtype=np.uint8 of bytes [sum(counts)][dim] (stored as they are).  The producer must have finished writing it."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError(f"device descriptors are float32 or uint8, not {dt}")
        c = np.ascontiguousarray(counts, dtype=np.int32)
        fn = self.L.hess_matcher_bank_set_device_u8 if dt == np.uint8 else self.L.hess_matcher_bank_set_device
        self._check(fn(self.h, len(c), c.ctypes.data, ptr))
        self._bank_sets = len(c)

    def set_bank_types(self, types):
        """types: one array per bank set (as passed to set_bank, before truncation to max_sift), or None to remove the
        types.  With types on the bank match_pairs returns the gated match of every pair (see set_types)."""
        if types is None:
            self._check(self.L.hess_matcher_bank_set_types(self.h, None, 2))
            return
        parts = [self._types(t)[0] for t in types]
        flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.uint16), dtype=np.uint16)
        if not len(flat):
            flat = np.zeros(1, np.uint16)   # (an address for a bank without descriptors: nothing is read)
        self._check(self.L.hess_matcher_bank_set_types(self.h, flat.ctypes.data, 2))

    def set_bank_types_device(self, ptr, stride):
        """ptr: device address of the first u16 type on the matcher's device, one per descriptor `stride` bytes apart."""
        self._check(self.L.hess_matcher_bank_set_types_device(self.h, ptr, int(stride)))

    # ---- two-view geometry from matches (hess_matcher_estimate*, the rule is stated in include/hess_abi.h) ----
    def estimate(self, matches, model, bound, hypotheses=0, seed=0, refit=0, info=False):
        """H ("H") or F ("F") from matches [n, 2] of the two single-pair slots (what match() returned), both located by
        set_locations -> (M [3, 3] float32 of unit norm, mask bool [n], hypothesis).  No model: zeros, no inliers and -1.
        M and `bound` are what match(H=M, hdistmax=bound) / match(F=M, fdistmax=bound) take; mask is that gate's decision.
        refit (0..8): at most so many least-squares refits of the RANSAC winner on its inliers (hess_abi.h, step 6); the
        inlier count never falls below refit=0's.  info=True appends a dict: inliers, refits (accepted), ransac_inliers
        (the count before any refit; 0 with refit=0)."""
        mt = check_pairs(matches)
        p = _geom_params(model, bound, hypotheses, seed, refit)
        res = np.zeros(1, dtype=GEOM_RESULT_DTYPE)
        mask = np.zeros(max(len(mt), 1), dtype=np.uint8)
        self._check(self.L.hess_matcher_estimate(self.h, len(mt), mt.ctypes.data, p.ctypes.data, res.ctypes.data, mask.ctypes.data))
        out = (res["M"][0].reshape(3, 3).copy(), mask[:len(mt)].astype(bool), int(res["hypothesis"][0]))
        return out + (_geom_info(res, 0),) if info else out

    def set_bank_locations(self, locs):
        """locs: one [n_i, 2] array of (x, y) per bank set (as passed to set_bank, before truncation to max_sift), or None to
        remove the locations.  Loading the bank again removes them too."""
        if locs is None:
            self._check(self.L.hess_matcher_bank_set_locations(self.h, None, 8))
            return
        parts = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in locs]
        flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2), np.float32), dtype=np.float32)
        if not len(flat):
            flat = np.zeros((1, 2), np.float32)   # (an address for a bank without descriptors: nothing is read)
        self._check(self.L.hess_matcher_bank_set_locations(self.h, flat.ctypes.data, 8))

    def set_bank_locations_device(self, ptr, stride):
        """ptr: device address of the first (x, y) float pair on the matcher's device, one per descriptor `stride` bytes apart."""
        self._check(self.L.hess_matcher_bank_set_locations_device(self.h, ptr, int(stride)))

    def estimate_pairs(self, pairs, matches_list, model, bound, hypotheses=0, seed=0, refit=0, info=False):
        """For every (a, b) of pairs and its matches (match_pairs' list): what estimate() returns for that pair with seed +
        its position and the same refit -> list of (M, mask, hypothesis), with info=True of (M, mask, hypothesis, dict).  The
        bank needs locations (set_bank_locations*)."""
        ab = check_pairs(pairs)
        if len(matches_list) != len(ab):
            raise ValueError(f"{len(ab)} pairs but {len(matches_list)} match lists")
        mts = [check_pairs(m) for m in matches_list]
        n = len(ab)
        mm = max([len(m) for m in mts] + [1])
        buf = np.zeros((max(n, 1), mm, 2), dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        for k, m in enumerate(mts):
            buf[k, :len(m)] = m
            cnt[k] = len(m)
        p = _geom_params(model, bound, hypotheses, seed, refit)
        res = np.zeros(max(n, 1), dtype=GEOM_RESULT_DTYPE)
        mask = np.zeros((max(n, 1), mm), dtype=np.uint8)
        self._check(self.L.hess_matcher_estimate_pairs(self.h, n, ab.ctypes.data, mm, buf.ctypes.data, cnt.ctypes.data,
                                                       p.ctypes.data, res.ctypes.data, mask.ctypes.data))
        out = [(res["M"][k].reshape(3, 3).copy(), mask[k, :cnt[k]].astype(bool), int(res["hypothesis"][k])) for k in range(n)]
        return [o + (_geom_info(res, k),) for k, o in enumerate(out)] if info else out

    def set_bank_from_session(self, session, types=False, locations=False):
        """The descriptors of a HessContext's last batch (run / run_device, or submit_* and wait), one set per image,
        without leaving the device -- floats or bytes, whichever the run made.  The context's descriptor length must be the
        matcher's: Matcher(dim=64) for a half_sift context.  types=True also takes the type field of the device key records,
        so that match_pairs gates by feature type (set_bank_types), again without a host round trip; locations=True takes
        their x, y for estimate_pairs (set_bank_locations_device)."""
        dim = session.desc_dim()
        if dim != self.dim:
            raise ValueError(f"the matcher takes {self.dim}-d descriptors; this context's are {dim}-d (-half / -sd)")
        keys, desc, total = session.device_results()
        counts = [session.count(i) for i in range(session._batch)]
        if sum(counts) != total:
            raise ValueError(f"the context's counts ({sum(counts)}) do not cover its device results ({total})")
        self.set_bank_device(desc, counts, dtype=np.uint8 if session.desc_format() == "u8" else np.float32)
        if types:
            self.set_bank_types_device((keys or 0) + _abi.KEYPOINT_DTYPE.fields["type"][1], _abi.KEYPOINT_DTYPE.itemsize)
        if locations:
            self.set_bank_locations_device((keys or 0) + _abi.KEYPOINT_DTYPE.fields["x"][1], _abi.KEYPOINT_DTYPE.itemsize)

    def bank(self, i):
        """The stored bytes of set i: [n, dim] u8."""
        n = self._check(self.L.hess_matcher_bank_read(self.h, int(i), None))
        out = np.zeros((n, self.dim), dtype=np.uint8)
        if n:
            self._check(self.L.hess_matcher_bank_read(self.h, int(i), out.ctypes.data))
        return out

    def match_pairs(self, pairs, max_match=4096, distmax=0.7, ratiomax=0.8, mutual_best=True):
        """Unguided match of bank[a] against bank[b] for every (a, b) in pairs -> list of [k, 2] int32 arrays, each what
        set_descriptors(0, bank[a]), set_descriptors(1, bank[b]), match(max_match, ...) returns."""
        p = check_pairs(pairs)
        if max_match < 0:
            raise ValueError("max_match must be >= 0")
        n = len(p)
        out = np.zeros((n, max(max_match, 1), 2), dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.L.hess_matcher_match_pairs(self.h, n, p.ctypes.data, max_match, out.ctypes.data, cnt.ctypes.data,
                                                    distmax, ratiomax, int(mutual_best)))
        return [out[k, :cnt[k]].copy() for k in range(n)]

    def match_pairs_guided(self, pairs, H=None, F=None, hdistmax=32.0, fdistmax=16.0, max_match=4096, distmax=0.7,
                           ratiomax=0.8, mutual_best=True):
        """Guided match of bank[a] against bank[b] for every (a, b) in pairs, pair p gated by H[p] and F[p] ([n, 3, 3]; one
        of them may be None: no such gate) within hdistmax and fdistmax (scalars or [n]) -> list of [k, 2] int32 arrays, each
        what set_descriptors / set_locations of the two sets and match(max_match, H[p], F[p], ...) return.  The bank needs
        locations (set_bank_locations*); what estimate_pairs returned goes straight in."""
        p = check_pairs(pairs)
        if max_match < 0:
            raise ValueError("max_match must be >= 0")
        n = len(p)
        geo = guided_pairs(n, H, F, hdistmax, fdistmax)
        out = np.zeros((n, max(max_match, 1), 2), dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.L.hess_matcher_match_pairs_guided(self.h, n, p.ctypes.data, geo.ctypes.data if n else None, max_match,
                                                           out.ctypes.data, cnt.ctypes.data, distmax, ratiomax, int(mutual_best)))
        return [out[k, :cnt[k]].copy() for k in range(n)]

    # ---- verified matches in one call (hess_matcher_verify_pairs, the rule is stated in include/hess_abi.h) ----
    @staticmethod
    def _verify_params(model, bound, hypotheses, seed, refit, guided_bound, final_estimate, distmax, ratiomax, mutual_best):
        """The argument checks of verify_pairs -> VERIFY_PARAMS_DTYPE [1]; ValueError before the library is called."""
        g = _geom_params(model, bound, hypotheses, seed, refit)
        gb = 0.0 if guided_bound is None else guided_bound
        for name, v in (("bound", bound), ("guided_bound", gb), ("distmax", distmax), ("ratiomax", ratiomax)):
            if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isreal(v):
                raise ValueError(f"{name} must be a number, not {v!r}")
        if not np.isfinite(gb) or gb < 0:
            raise ValueError(f"guided_bound must be finite and not negative (None or 0: bound), not {gb!r}")
        if final_estimate not in (True, False, 0, 1):
            raise ValueError(f"final_estimate is True or False, not {final_estimate!r}")
        p = np.zeros(1, dtype=VERIFY_PARAMS_DTYPE)
        p["geom"] = g
        p["distmax"], p["ratiomax"], p["mutual_best"] = distmax, ratiomax, int(bool(mutual_best))
        p["guided_bound"], p["final_estimate"] = gb, int(bool(final_estimate))
        return p

    def verify_pairs_raw(self, pairs, params, max_match=4096, inlier=True, putative=False):
        """hess_matcher_verify_pairs as it stands: params a VERIFY_PARAMS_DTYPE [1] -> (matches int32 [n, max_match, 2], counts
        int32 [n], results VERIFY_RESULT_DTYPE [n], inlier uint8 [n, max_match] or None, putative int32 [n, max_match, 2] or
        None); the two optional outputs are passed as NULL when not asked for."""
        ab = check_pairs(pairs)
        if max_match < 0:
            raise ValueError("max_match must be >= 0")
        n, w = len(ab), max(int(max_match), 1)
        out = np.zeros((max(n, 1), w, 2), dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        res = np.zeros(max(n, 1), dtype=VERIFY_RESULT_DTYPE)
        mask = np.zeros((max(n, 1), w), dtype=np.uint8) if inlier else None
        put = np.zeros((max(n, 1), w, 2), dtype=np.int32) if putative else None
        self._check(self.L.hess_matcher_verify_pairs(self.h, n, ab.ctypes.data, params.ctypes.data, int(max_match), out.ctypes.data,
                                                     cnt.ctypes.data, res.ctypes.data, mask.ctypes.data if inlier else None,
                                                     put.ctypes.data if putative else None))
        return out[:n], cnt[:n], res[:n], (mask[:n] if inlier else None), (put[:n] if putative else None)

    def verify_pairs(self, pairs, model, bound, hypotheses=0, seed=0, refit=0, guided_bound=None, final_estimate=True,
                     max_match=4096, distmax=0.7, ratiomax=0.8, mutual_best=True, putative=False):
        """Geometrically verified matches of bank[a] against bank[b] for every (a, b) in pairs, in one call: what match_pairs,
        estimate_pairs (model, bound, hypotheses, seed + position, refit), match_pairs_guided with each pair's estimate
        within guided_bound (None: bound) and, with final_estimate, estimate_pairs again on the guided matches return when
        chained -- without their host round trips.  -> a list of dicts: matches [k, 2] (the guided matches); M [3, 3],
        hypothesis, inliers (the estimate on the unguided matches; no model: zeros, -1, 0 and no matches); with
        final_estimate M_final [3, 3], mask bool [k] and info (inliers, refits, ransac_inliers of the final estimate); with
        putative=True putative [n, 2] (the unguided matches).  The bank needs locations (set_bank_locations*)."""
        p = self._verify_params(model, bound, hypotheses, seed, refit, guided_bound, final_estimate, distmax, ratiomax, mutual_best)
        fin = bool(final_estimate)
        out, cnt, res, mask, put = self.verify_pairs_raw(pairs, p, max_match, inlier=fin, putative=bool(putative))
        ret = []
        for k in range(len(cnt)):
            d = {"matches": out[k, :cnt[k]].copy(), "M": res["putative"]["M"][k].reshape(3, 3).copy(),
                 "hypothesis": int(res["putative"]["hypothesis"][k]), "inliers": int(res["putative"]["inliers"][k])}
            if fin:
                d["M_final"] = res["final"]["M"][k].reshape(3, 3).copy()
                d["mask"] = mask[k, :cnt[k]].astype(bool)
                d["info"] = _geom_info(res["final"], k)
            if putative:
                d["putative"] = put[k, :res["nputative"][k]].copy()
            ret.append(d)
        return ret
