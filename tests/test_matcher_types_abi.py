"""The feature-type entry points of the matcher without a GPU: include/hess_abi.h declares them with the argument lists
hessgpu_amd/_abi.py binds, the libraries export them, a NULL matcher is refused, SiftGPU.h adds SetFeatureTypes without
touching the vtable, and the Python wrapper normalises type arrays before it calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hessgpu_amd
from hessgpu_amd import _abi
from hessgpu_amd import matcher as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hess_matcher_set_types", "hess_matcher_bank_set_types", "hess_matcher_bank_set_types_device"]
CTYPE = {"hess_matcher*": C.c_void_p, "int": C.c_int, "const uint16_t*": C.c_void_p, "const void*": C.c_void_p,
         "size_t": C.c_size_t}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_prototypes_match_the_header_and_the_library_exports_them():
    text = _header("hess_abi.h")
    lib = hessgpu_amd.load_library()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]   # drop the names
        res, argtypes = _abi.PRODUCT_PROTOTYPES[name[len("hess_"):]]
        assert res is C.c_int and argtypes == [CTYPE[a] for a in args], (name, args)
        assert hasattr(lib, name), name
        assert getattr(hm._lib(), name).argtypes == argtypes, name
    assert _abi.HESS_ABI_VERSION == 5
    assert re.search(r"#define\s+HESS_ABI_VERSION\s+5\b", text)


def test_null_matcher_is_refused():
    L = hm._lib()
    t = np.zeros(4, np.uint16)
    assert L.hess_matcher_set_types(None, 0, t.ctypes.data, 2) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_bank_set_types(None, t.ctypes.data, 2) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_bank_set_types_device(None, t.ctypes.data, 2) == _abi.HESS_ERR_ARG


def test_siftgpu_header_adds_a_non_virtual_member_after_the_virtual_ones():
    text = re.sub(r"//[^\n]*", "", _header("SiftGPU.h"))
    body = re.search(r"class SiftMatchGPU \{(.*?)\n\};", text, flags=re.S).group(1)
    decls = [m.start() for m in re.finditer(r"\bSetFeatureTypes\s*\(", body)]
    assert decls, "SetFeatureTypes is not declared"
    assert max(m.start() for m in re.finditer(r"\bvirtual\b", body)) < min(decls)
    for d in decls:
        line = body[body.rfind("\n", 0, d):d]
        assert "virtual" not in line, line
    assert re.search(r"int\s+SetFeatureTypes\s*\(\s*int\s+index\s*,\s*const\s+SiftGPU::SiftKeypoint\s*\*\s*keys\s*\)", body)
    assert re.search(r"\bint\s+siftmatch_set_types\s*\(\s*SiftMatchGPU\s*\*\s*m\s*,\s*int\s+index\s*,\s*const\s+unsigned\s+short\s*\*"
                     r"\s*types\s*,\s*int\s+stride_bytes\s*\)", text)
    api = C.CDLL(os.path.join(os.path.dirname(hessgpu_amd.__file__), "libsiftgpu.so"))
    assert hasattr(api, "siftmatch_set_types")


def test_type_arrays_are_normalised_before_the_library():
    keys = np.zeros(5, _abi.KEYPOINT_DTYPE)
    keys["type"] = [0, 1, 2, 3, 0xfffe]
    a, ptr, stride = hm.Matcher._types(keys)
    assert stride == _abi.KEYPOINT_DTYPE.itemsize == 24 and ptr == keys.ctypes.data + 22 and a.tolist() == [0, 1, 2, 3, 0xfffe]
    a, ptr, stride = hm.Matcher._types([2, 1, 0])
    assert a.dtype == np.uint16 and stride == 2 and a.tolist() == [2, 1, 0]
    a, ptr, stride = hm.Matcher._types(np.arange(10, dtype=np.uint16)[::-1])      # a negative stride is copied
    assert stride == 2 and a.tolist() == list(range(9, -1, -1))
    a, ptr, stride = hm.Matcher._types(np.arange(10, dtype=np.uint16)[::3])       # a positive even one is used
    assert stride == 6 and a.tolist() == [0, 3, 6, 9]
    for bad in (np.zeros(3, np.float32), np.zeros((2, 2), np.uint16)):
        with pytest.raises(ValueError):
            hm.Matcher._types(bad)
