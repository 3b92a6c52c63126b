"""The staging protocol of pageable input (hessgpu_amd/csrc/hess_stager.cpp: helper threads and the calling thread's walk)
under ThreadSanitizer, without a GPU: tests/stager_main.cpp drives one Stager through jobs of six shapes back to back and
checks every job's bytes, callbacks and guard bytes; the sanitizer checks the memory orders and who holds the mutex when."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hessgpu_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread"]


def _compiler():
    # clang++ first: its sanitizer runtime starts under any address-space layout (it re-runs the program without randomisation
    # when the kernel's layout does not suit it); g++'s older one ends with "unexpected memory mapping" on some kernels
    for cxx in ("/opt/rocm/llvm/bin/clang++", "g++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def test_stager_protocol_under_thread_sanitizer(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    exe = str(tmp_path / "stager_main")
    build = subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(CSRC, "hess_stager.cpp"),
                            os.path.join(ROOT, "tests", "stager_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")  # (the program carries the sanitizer's runtime itself)
    setarch = shutil.which("setarch")  # no address randomisation for this one program: what either runtime is happy with
    r = subprocess.run(([setarch, os.uname().machine, "-R"] if setarch else []) + [exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "STAGER OK" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
