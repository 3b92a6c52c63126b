"""Guided matching for bank pairs (hess_matcher_match_pairs_guided) without a GPU: the header declares the entry point and
its struct, the library exports it, a NULL matcher is refused, the struct is 80 bytes on both sides, and the Python wrapper
rejects malformed geometry before it calls the library and fills a missing matrix by SiftMatchGPU::GetGuidedSiftMatch's rule."""
import os
import re
import subprocess

import numpy as np
import pytest

import hessgpu_amd
from hessgpu_amd import _abi
from hessgpu_amd import matcher as hm
from test_stager_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hess_abi.h")


def test_header_declares_and_library_exports_the_entry_point():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+hess_matcher_match_pairs_guided\s*\(\s*hess_matcher\s*\*\s*m\s*,\s*int\s+npairs\s*,\s*const\s+int\s*\*\s*"
                     r"pairs_ab\s*,\s*const\s+hess_guided_pair\s*\*\s*geo\s*,\s*int\s+max_match\s*,\s*int\s*\*\s*out_pairs\s*,\s*"
                     r"int\s*\*\s*out_counts\s*,\s*float\s+distmax\s*,\s*float\s+ratiomax\s*,\s*int\s+mutual_best\s*\)", text)
    assert re.search(r"typedef\s+struct\s+hess_guided_pair\s*\{\s*float\s+H\[9\]\s*,\s*F\[9\]\s*;\s*float\s+hdistmax\s*,\s*fdistmax\s*;\s*\}",
                     text)
    assert hasattr(hessgpu_amd.load_library(), "hess_matcher_match_pairs_guided")
    assert _abi.HESS_ABI_VERSION == 5
    listed = raw[:raw.index("#define HESS_ABI_VERSION")]
    assert "hess_matcher_match_pairs_guided" in listed and "without a" in listed.split("hess_matcher_match_pairs_guided")[1][:200]


def test_null_matcher_is_refused():
    L = hm._lib()
    pairs = np.array([[0, 1]], np.int32)
    geo = hm.guided_pairs(1, H=np.eye(3)[None])
    out = np.zeros((1, 4, 2), np.int32)
    cnt = np.zeros(1, np.int32)
    assert L.hess_matcher_match_pairs_guided(None, 1, pairs.ctypes.data, geo.ctypes.data, 4, out.ctypes.data, cnt.ctypes.data,
                                             0.7, 0.8, 1) == _abi.HESS_ERR_ARG


def test_the_struct_is_80_bytes_on_both_sides(tmp_path):
    assert hm.GUIDED_PAIR_DTYPE.itemsize == 80
    f = hm.GUIDED_PAIR_DTYPE.fields
    assert [f[k][1] for k in ("H", "F", "hdistmax", "fdistmax")] == [0, 36, 72, 76]
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    src = tmp_path / "size.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "hess_abi.h"\nint main() { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(hess_guided_pair), offsetof(hess_guided_pair, H), offsetof(hess_guided_pair, F), "
                   "offsetof(hess_guided_pair, hdistmax), offsetof(hess_guided_pair, fdistmax)); return 0; }\n")
    exe = str(tmp_path / "size")
    b = subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["80", "0", "36", "72", "76"], r.stdout + r.stderr


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for malformed geometry")


def _bare():
    m = hm.Matcher.__new__(hm.Matcher)            # no device needed: the checks come first
    m.L, m.h = _NoLibrary(), None
    return m


I3 = np.eye(3, dtype=np.float32)


@pytest.mark.parametrize("kw", [
    dict(),                                                        # both matrices missing
    dict(H=None, F=None),
    dict(H=I3),                                                    # [3, 3] for two pairs
    dict(H=np.stack([I3] * 3)),                                    # three matrices for two pairs
    dict(F=np.stack([I3] * 1)),
    dict(H=np.zeros((2, 9), np.float32)),                          # flat
    dict(H=np.zeros((2, 3, 4), np.float32)),
    dict(H=np.stack([I3] * 2), F=np.zeros((2, 2, 3), np.float32)),
    dict(H=np.array([[["a"] * 3] * 3] * 2)),                       # strings
    dict(H=np.stack([I3] * 2), hdistmax=[1.0, 2.0, 3.0]),          # three bounds for two pairs
    dict(F=np.stack([I3] * 2), fdistmax=np.ones((2, 1))),
    dict(F=np.stack([I3] * 2), fdistmax="16"),
])
def test_match_pairs_guided_rejects_malformed_geometry_before_the_library(kw):
    with pytest.raises(ValueError):
        _bare().match_pairs_guided([[0, 1], [1, 0]], **kw)


@pytest.mark.parametrize("pairs", [[[0, 1, 2]], [0, 1], np.array([[0.0, 1.0]]), [[0, 1], [-1, 2]]])
def test_match_pairs_guided_rejects_malformed_pairs_before_the_library(pairs):
    with pytest.raises(ValueError):
        _bare().match_pairs_guided(pairs, H=np.stack([I3] * len(pairs)))
    with pytest.raises(ValueError):
        _bare().match_pairs_guided([[0, 1]], H=I3[None], max_match=-1)


def test_missing_matrix_rule_fills_identity_and_1e20():
    M = np.arange(18, dtype=np.float64).reshape(2, 3, 3)
    g = hm.guided_pairs(2, H=M, hdistmax=[3.0, 4.0], fdistmax=7.0)
    assert g.dtype == hm.GUIDED_PAIR_DTYPE and g.shape == (2,)
    assert np.array_equal(g["H"], M.reshape(2, 9).astype(np.float32)) and g["hdistmax"].tolist() == [3.0, 4.0]
    assert np.array_equal(g["F"], np.tile(I3.reshape(9), (2, 1))) and np.all(g["fdistmax"] == np.float32(1e20))
    g = hm.guided_pairs(2, F=M, hdistmax=5.0, fdistmax=np.array([1, 2]))
    assert np.array_equal(g["H"], np.tile(I3.reshape(9), (2, 1))) and np.all(g["hdistmax"] == np.float32(1e20))
    assert np.array_equal(g["F"], M.reshape(2, 9).astype(np.float32)) and g["fdistmax"].tolist() == [1.0, 2.0]
    g = hm.guided_pairs(1, H=M[:1], F=M[1:], hdistmax=2.5, fdistmax=1.0)
    assert (g["hdistmax"][0], g["fdistmax"][0]) == (2.5, 1.0)
    assert hm.guided_pairs(0, H=np.zeros((0, 3, 3))).shape == (0,)
