"""hess_matcher_verify_pairs without a GPU: the header declares the entry point and both structs, the library exports it, the
structs are 64 and 128 bytes on both sides, a NULL matcher is refused, and the Python wrapper rejects malformed arguments
before it calls the library."""
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

PARAMS_OFFSETS = {"geom": 0, "distmax": 32, "ratiomax": 36, "mutual_best": 40, "guided_bound": 44, "final_estimate": 48, "reserved": 52}
RESULT_OFFSETS = {"putative": 0, "final": 52, "nputative": 104, "nguided": 108, "reserved": 112}


def test_header_declares_and_library_exports_the_entry_point():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+hess_matcher_verify_pairs\s*\(\s*hess_matcher\s*\*\s*m\s*,\s*int\s+npairs\s*,\s*const\s+int\s*\*\s*pairs_ab\s*,"
                     r"\s*const\s+hess_verify_params\s*\*\s*params\s*,\s*int\s+max_match\s*,\s*int\s*\*\s*out_pairs\s*,\s*int\s*\*\s*"
                     r"out_counts\s*,\s*hess_verify_result\s*\*\s*out\s*,\s*unsigned\s+char\s*\*\s*inlier\s*,\s*int\s*\*\s*"
                     r"putative_pairs\s*\)", text)
    p = re.search(r"typedef\s+struct\s+hess_verify_params\s*\{(.*?)\}\s*hess_verify_params\s*;", text, flags=re.S)
    assert p and [w for w in re.findall(r"\b(geom|distmax|ratiomax|mutual_best|guided_bound|final_estimate|reserved)\b", p.group(1))] == \
        ["geom", "distmax", "ratiomax", "mutual_best", "guided_bound", "final_estimate", "reserved"]
    r = re.search(r"typedef\s+struct\s+hess_verify_result\s*\{(.*?)\}\s*hess_verify_result\s*;", text, flags=re.S)
    assert r and re.findall(r"\b(putative|final|nputative|nguided|reserved)\b", r.group(1)) == \
        ["putative", "final", "nputative", "nguided", "reserved"]
    assert hasattr(hessgpu_amd.load_library(), "hess_matcher_verify_pairs")
    assert _abi.HESS_ABI_VERSION == 5
    listed = raw[:raw.index("#define HESS_ABI_VERSION")]
    assert "hess_matcher_verify_pairs" in listed and "without a bump" in listed.split("hess_matcher_verify_pairs")[1][:300]
    rule = raw[raw.index("THE RULE"):raw.index("typedef struct hess_verify_params")]
    for word in ("hess_matcher_match_pairs(", "hess_matcher_estimate_pairs(", "hess_matcher_match_pairs_guided(", "byte for byte",
                 "seed + p", "identity", "1e20", "HESS_ERR_STATE", "HESS_ERR_UNSUPPORTED", "HESS_ERR_ARG", "HESS_ERR_TOO_BIG"):
        assert word in rule, word


def test_null_matcher_is_refused():
    L = hm._lib()
    pairs = np.array([[0, 1]], np.int32)
    p = hm.Matcher._verify_params("H", 8.0, 0, 0, 0, None, True, 0.7, 0.8, True)
    out, cnt = np.zeros((1, 4, 2), np.int32), np.zeros(1, np.int32)
    res = np.zeros(1, hm.VERIFY_RESULT_DTYPE)
    assert L.hess_matcher_verify_pairs(None, 1, pairs.ctypes.data, p.ctypes.data, 4, out.ctypes.data, cnt.ctypes.data, res.ctypes.data,
                                       None, None) == _abi.HESS_ERR_ARG
    assert "matcher_verify_pairs" in _abi.PRODUCT_PROTOTYPES


def test_the_structs_are_64_and_128_bytes_on_both_sides(tmp_path):
    P, R = _abi.VERIFY_PARAMS_DTYPE, _abi.VERIFY_RESULT_DTYPE
    assert P is hm.VERIFY_PARAMS_DTYPE and R is hm.VERIFY_RESULT_DTYPE
    assert P.itemsize == 64 and R.itemsize == 128
    assert {k: P.fields[k][1] for k in PARAMS_OFFSETS} == PARAMS_OFFSETS
    assert {k: R.fields[k][1] for k in RESULT_OFFSETS} == RESULT_OFFSETS
    assert P["geom"] == hm.GEOM_PARAMS_DTYPE and R["putative"] == hm.GEOM_RESULT_DTYPE and R["final"] == hm.GEOM_RESULT_DTYPE
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    src = tmp_path / "size.cpp"
    fields = [f"offsetof(hess_verify_params, {k})" for k in PARAMS_OFFSETS] + [f"offsetof(hess_verify_result, {k})" for k in RESULT_OFFSETS]
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "hess_abi.h"\nint main() {\n'
                   '  const size_t v[] = {sizeof(hess_verify_params), sizeof(hess_verify_result), ' + ", ".join(fields) + "};\n"
                   '  for (size_t x : v) printf("%zu ", x);\n  return 0;\n}\n')
    exe = str(tmp_path / "size")
    b = subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    want = [64, 128] + list(PARAMS_OFFSETS.values()) + list(RESULT_OFFSETS.values())
    assert r.stdout.split() == [str(x) for x in want], r.stdout + r.stderr


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a malformed argument")


def _bare():
    m = hm.Matcher.__new__(hm.Matcher)            # no device needed: the checks come first
    m.L, m.h = _NoLibrary(), None
    return m


@pytest.mark.parametrize("kw", [
    dict(model="G"),
    dict(model=3),
    dict(bound="8"),
    dict(bound=[8.0, 8.0]),
    dict(guided_bound=-1.0),
    dict(guided_bound=float("nan")),
    dict(guided_bound=float("inf")),
    dict(guided_bound="4"),
    dict(final_estimate=2),
    dict(final_estimate="yes"),
    dict(distmax=None),
    dict(ratiomax="0.8"),
    dict(max_match=-1),
])
def test_verify_pairs_rejects_malformed_arguments_before_the_library(kw):
    args = dict(model="H", bound=8.0)
    args.update(kw)
    with pytest.raises(ValueError):
        _bare().verify_pairs([[0, 1], [1, 0]], **args)


@pytest.mark.parametrize("pairs", [[[0, 1, 2]], [0, 1], np.array([[0.0, 1.0]]), [[0, 1], [-1, 2]]])
def test_verify_pairs_rejects_malformed_pairs_before_the_library(pairs):
    with pytest.raises(ValueError):
        _bare().verify_pairs(pairs, "F", 4.0)


def test_params_carry_every_argument():
    p = hm.Matcher._verify_params("F", 4.0, 300, 2 ** 32 + 5, 2, 6.5, False, 0.6, 0.9, False)
    assert p.dtype == hm.VERIFY_PARAMS_DTYPE and p.shape == (1,)
    g = p["geom"][0]
    assert (int(g["model"]), int(g["hypotheses"]), int(g["seed"]), float(g["bound"]), g["reserved"].tolist()) == (2, 300, 5, 4.0, [2, 0, 0, 0])
    assert (float(p["distmax"][0]), float(p["ratiomax"][0])) == (float(np.float32(0.6)), float(np.float32(0.9)))
    assert (int(p["mutual_best"][0]), float(p["guided_bound"][0]), int(p["final_estimate"][0])) == (0, 6.5, 0)
    assert not p["reserved"].any()
    q = hm.Matcher._verify_params("H", 8.0, 0, 0, 0, None, True, 0.7, 0.8, True)
    assert float(q["guided_bound"][0]) == 0.0 and int(q["final_estimate"][0]) == 1 and int(q["mutual_best"][0]) == 1
