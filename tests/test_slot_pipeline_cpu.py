"""The matcher's double-buffered delivery loop (hessgpu_amd/csrc/hess_slot_pipeline.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/slot_pipeline_main.cpp drives it with recording callables for calls of 1, 2, 3 and 5 units --
every call succeeding, then enqueue k failing and collect k failing for every unit k -- and prints what was called.  Here the
printed sequences are held against the ones below, written out by hand: eK.S is enqueue(K, slot S), cK.S is collect(K, slot S);
a failing enqueue k returns 100 + k and a failing collect k 200 + k, nothing is called after it, and its status comes back."""
import os
import shutil
import subprocess

import pytest

from test_stager_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hessgpu_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

EXPECTED = """\
1 ok : e0.0 c0.0 -> 0
1 e0 : e0.0 -> 100
1 c0 : e0.0 c0.0 -> 200
2 ok : e0.0 e1.1 c0.0 c1.1 -> 0
2 e0 : e0.0 -> 100
2 c0 : e0.0 e1.1 c0.0 -> 200
2 e1 : e0.0 e1.1 -> 101
2 c1 : e0.0 e1.1 c0.0 c1.1 -> 201
3 ok : e0.0 e1.1 c0.0 e2.0 c1.1 c2.0 -> 0
3 e0 : e0.0 -> 100
3 c0 : e0.0 e1.1 c0.0 -> 200
3 e1 : e0.0 e1.1 -> 101
3 c1 : e0.0 e1.1 c0.0 e2.0 c1.1 -> 201
3 e2 : e0.0 e1.1 c0.0 e2.0 -> 102
3 c2 : e0.0 e1.1 c0.0 e2.0 c1.1 c2.0 -> 202
5 ok : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 c2.0 e4.0 c3.1 c4.0 -> 0
5 e0 : e0.0 -> 100
5 c0 : e0.0 e1.1 c0.0 -> 200
5 e1 : e0.0 e1.1 -> 101
5 c1 : e0.0 e1.1 c0.0 e2.0 c1.1 -> 201
5 e2 : e0.0 e1.1 c0.0 e2.0 -> 102
5 c2 : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 c2.0 -> 202
5 e3 : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 -> 103
5 c3 : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 c2.0 e4.0 c3.1 -> 203
5 e4 : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 c2.0 e4.0 -> 104
5 c4 : e0.0 e1.1 c0.0 e2.0 c1.1 e3.1 c2.0 e4.0 c3.1 c4.0 -> 204
"""


def test_call_sequences_of_the_slot_pipeline(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    exe = str(tmp_path / "slot_pipeline_main")
    build = subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "slot_pipeline_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    setarch = shutil.which("setarch")  # no address randomisation for this one program, as in test_stager_cpu
    r = subprocess.run(([setarch, os.uname().machine, "-R"] if setarch else []) + [exe, "1", "2", "3", "5"], capture_output=True,
                       text=True, timeout=120)  # (the program carries the sanitizers' runtimes itself)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got, want = r.stdout.splitlines(), EXPECTED.splitlines()
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:3] + [len(got), len(want)]
