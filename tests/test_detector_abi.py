"""hess_params.detector (HESS_DETECTOR_*): the public name of word 0 of reserved[] -- layout from C, C++ and ctypes, its
default, and the SiftGPU switch that sets it.  No device needed."""
import ctypes as C
import os
import subprocess

import pytest

import siftgpu_lib
from hessgpu_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "hessgpu_amd")

_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "hess_abi.h"
int main(void) {
  hess_params p;
  hess_default_params(&p);
  int before = p.detector;
  p.detector = HESS_DETECTOR_DOG;
  printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(hess_params), (int)offsetof(hess_params, detector),
         (int)offsetof(hess_params, reserved), (int)offsetof(hess_params, reserved_tail), p.reserved[0], before,
         HESS_DETECTOR_HESSIAN, HESS_ABI_VERSION);
  return 0;
}
"""


def _probe(tmp_path, compiler, std, suffix):
    src = tmp_path / f"probe{suffix}"
    src.write_text(_PROBE)
    exe = str(tmp_path / f"probe_{compiler}")
    subprocess.run([compiler, std, "-Wall", "-I", INC, str(src), "-o", exe, "-L", LIBDIR, "-lhessgpu",
                    f"-Wl,-rpath,{LIBDIR}"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return [int(v) for v in out]


@pytest.mark.parametrize("compiler,std,suffix", [("gcc", "-std=gnu11", ".c"), ("g++", "-std=c++11", ".cpp")])
def test_detector_aliases_reserved_word_0_in_c_and_cpp(tmp_path, compiler, std, suffix):
    size, off_det, off_res, off_tail, word0, default, hessian, version = _probe(tmp_path, compiler, std, suffix)
    assert size == C.sizeof(_abi.HessParams) == 128        # the struct did not grow
    assert off_det == off_res == _abi.HessParams.reserved.offset == 104
    assert off_tail == off_res + 4
    assert word0 == _abi.DETECTOR_DOG == 1                 # one memory word, two names
    assert default == hessian == _abi.DETECTOR_HESSIAN == 0
    assert version == _abi.HESS_ABI_VERSION == 5


def test_ctypes_alias_and_default():
    import hessgpu_amd

    p = hessgpu_amd.default_params()
    assert p.detector == 0 and list(p.reserved) == [0] * 6
    p.detector = _abi.DETECTOR_DOG
    assert p.reserved[0] == 1 and list(p.reserved_tail) == [0] * 5
    p.reserved[0] = 0
    assert p.detector == 0
    assert hessgpu_amd.default_params(detector=1).reserved[0] == 1
    assert _abi.HessParams.detector.offset == _abi.HessParams.reserved.offset


def _params(args):
    s = siftgpu_lib.SiftGPU(args)
    p = s.params()
    s.close()
    return p


def test_siftgpu_dog_switch_sets_the_detector():
    assert _params([]).detector == _abi.DETECTOR_HESSIAN
    p = _params(["-dog"])
    assert p.detector == _abi.DETECTOR_DOG and p.reserved[0] == 1 and list(p.reserved_tail) == [0] * 5
    # -d N still means scales per octave, with or without -dog
    p = _params(["-d", "5", "-dog"])
    assert p.dog_level_num == 5 and p.detector == _abi.DETECTOR_DOG
    p = _params(["-d", "4"])
    assert p.dog_level_num == 4 and p.detector == _abi.DETECTOR_HESSIAN
