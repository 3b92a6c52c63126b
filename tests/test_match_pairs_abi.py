"""Batched matching (hess_matcher_bank_* / hess_matcher_match_pairs) without a GPU: the header declares the entry points,
the library exports them, a NULL matcher is refused, and the Python wrapper rejects malformed pair arrays before it
calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hessgpu_amd
from hessgpu_amd import _abi
from hessgpu_amd import matcher as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hess_matcher_bank_set", "hess_matcher_bank_set_f32", "hess_matcher_bank_set_device", "hess_matcher_bank_read",
       "hess_matcher_match_pairs"]


def test_header_declares_and_library_exports_the_batched_matcher():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hess_abi.h")).read(), flags=re.S)
    lib = hessgpu_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
    assert _abi.HESS_ABI_VERSION == 5


def test_null_matcher_is_refused():
    L = hm._lib()
    counts = np.array([1, 2], np.int32)
    u8 = np.zeros((3, 128), np.uint8)
    f32 = np.zeros((3, 128), np.float32)
    pairs = np.array([[0, 1]], np.int32)
    out = np.zeros((1, 4, 2), np.int32)
    cnt = np.zeros(1, np.int32)
    assert L.hess_matcher_bank_set(None, 2, counts.ctypes.data, u8.ctypes.data) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_bank_set_f32(None, 2, counts.ctypes.data, f32.ctypes.data) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_bank_set_device(None, 2, counts.ctypes.data, f32.ctypes.data) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_bank_read(None, 0, u8.ctypes.data) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_match_pairs(None, 1, pairs.ctypes.data, 4, out.ctypes.data, cnt.ctypes.data, 0.7, 0.8,
                                      1) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_last_ms(None) == 0.0


def test_pair_helpers():
    assert hm.all_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert hm.all_pairs(1).shape == (0, 2) and hm.all_pairs(16).shape == (120, 2)
    assert hm.window_pairs(5, 2).tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [2, 4], [3, 4]]
    w = hm.window_pairs(64, 8)
    assert len(w) == sum(min(8, 63 - i) for i in range(64)) and (w[:, 1] - w[:, 0]).max() == 8
    assert w.dtype == np.int32


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a malformed pair array")


@pytest.mark.parametrize("pairs", [
    [[0, 1, 2]],                                  # wrong shape
    [0, 1],                                       # one-dimensional
    np.zeros((2, 2, 2), np.int32),                # three-dimensional
    np.array([[0.0, 1.0]]),                       # floats
    np.array([[True, False]]),                    # booleans
    np.array([["0", "1"]]),                       # strings
    [[0, 1], [-1, 2]],                            # negative index
    np.array([[0, 2 ** 40]], np.int64),           # beyond int32
])
def test_match_pairs_rejects_malformed_pairs_before_the_library(pairs):
    m = hm.Matcher.__new__(hm.Matcher)            # no device needed: the checks come first
    m.L, m.h = _NoLibrary(), None
    with pytest.raises(ValueError):
        m.match_pairs(pairs)


def test_check_pairs_normalises():
    p = hm.check_pairs(np.array([[3, 1], [0, 0]], np.int64))
    assert p.dtype == np.int32 and p.flags.c_contiguous and p.tolist() == [[3, 1], [0, 0]]
    assert hm.check_pairs([]).shape == (0, 2)
    assert hm.check_pairs(np.array([[1, 2], [3, 4]], np.uint16)[::-1]).tolist() == [[3, 4], [1, 2]]
