"""Byte descriptors (hess_set_descriptor_format / hess_desc_format / hess_fetch_u8 / hess_matcher_bank_set_device_u8)
without a GPU: the header declares the entry points, the library exports them, _abi.py mirrors them, NULL handles are
refused, and hess_params keeps its layout (the entry points were added during ABI version 5 without a bump)."""
import ctypes as C
import os
import re

import numpy as np

import hessgpu_amd
from hessgpu_amd import _abi
from hessgpu_amd import matcher as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["set_descriptor_format", "desc_format", "fetch_u8", "matcher_bank_set_device_u8"]


def _header():
    return open(os.path.join(ROOT, "include", "hess_abi.h")).read()


def test_header_declares_library_exports_and_abi_mirrors_the_new_names():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = hessgpu_amd.load_library()
    fns = hessgpu_amd.functions()
    for name in NEW:
        assert re.search(r"\bint\s+hess_" + name + r"\s*\(", text), name
        assert hasattr(lib, "hess_" + name), name
        assert name in _abi.PRODUCT_PROTOTYPES and name in fns, name
        assert _abi.PRODUCT_PROTOTYPES[name][0] is C.c_int
    assert hasattr(hm._lib(), "hess_matcher_bank_set_device_u8")


def test_null_handles_are_refused():
    fns = hessgpu_amd.functions()
    keys = np.zeros(4, _abi.KEYPOINT_DTYPE)
    desc = np.zeros((4, 128), np.uint8)
    counts = np.array([1, 2], np.int32)
    assert fns["set_descriptor_format"](None, _abi.DESC_FORMAT_U8) == _abi.HESS_ERR_ARG
    assert fns["set_descriptor_format"](None, _abi.DESC_FORMAT_F32) == _abi.HESS_ERR_ARG
    assert fns["desc_format"](None) == _abi.HESS_ERR_ARG
    assert fns["fetch_u8"](None, 0, keys.ctypes.data, desc.ctypes.data) == _abi.HESS_ERR_ARG
    assert not desc.any() and not keys.view(np.uint8).any()
    assert fns["matcher_bank_set_device_u8"](None, 2, counts.ctypes.data, desc.ctypes.data) == _abi.HESS_ERR_ARG
    assert hm._lib().hess_matcher_bank_set_device_u8(None, 2, counts.ctypes.data, desc.ctypes.data) == _abi.HESS_ERR_ARG


def test_enum_values_version_and_params_layout():
    assert (_abi.DESC_FORMAT_F32, _abi.DESC_FORMAT_U8) == (0, 1)
    m = re.search(r"enum\s*\{\s*HESS_DESC_FORMAT_F32\s*=\s*(\d+)\s*,\s*HESS_DESC_FORMAT_U8\s*=\s*(\d+)\s*\}", _header())
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert _abi.HESS_ABI_VERSION == 5 and re.search(r"#define\s+HESS_ABI_VERSION\s+5\b", _header())
    # hess_params: 26 words + reserved[6], as before the byte format (which is no field of it)
    assert C.sizeof(_abi.HessParams) == 32 * 4
    assert not any("format" in name for name, _ in _abi.HessParams._fields_)


def test_session_rejects_an_unknown_format_name_before_the_library():
    class _NoLibrary(dict):
        def __getitem__(self, name):
            raise AssertionError(f"the library was called ({name}) for an unknown format name")

    s = hessgpu_amd.Session.__new__(hessgpu_amd.Session)
    s._f, s._h = _NoLibrary(), None
    for bad in ("u16", "U8", 1, None):
        try:
            s.set_descriptor_format(bad)
        except ValueError:
            continue
        raise AssertionError(f"{bad!r} was accepted")


def test_matcher_rejects_other_device_dtypes_before_the_library():
    class _NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name}) for a dtype the matcher does not take")

    m = hm.Matcher.__new__(hm.Matcher)
    m.L, m.h = _NoLibrary(), None
    for bad in (np.float64, np.int8, np.uint16):
        try:
            m.set_bank_device(0, [1], dtype=bad)
        except ValueError:
            continue
        raise AssertionError(f"{bad} was accepted")
