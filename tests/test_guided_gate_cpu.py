"""The guided gate (hessgpu_amd/csrc/hess_guided_gate.h: the one copy match_dot_kernel, match_mfma_kernel<GUIDED> and the
estimator's geom_gate call) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/guided_gate_main.cpp computes
the row terms and the column terms once, as the matrix-core kernel does, and prints the decision of every (i, j).  For the cases
of tests/guided_cases.py at their pick_thresholds the decisions must equal the float64 model gc.gates: no pair there is uncertain
(tests/test_guided_cases.py), so equality is required for all of them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import guided_cases as gc
from test_stager_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hessgpu_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def gate(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    exe = str(tmp_path_factory.mktemp("guided_gate") / "guided_gate_main")
    build = subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "guided_gate_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr

    def run(cases):
        """cases: [(loc1, loc2, H, F, hdistmax, fdistmax)] -> [bool [n1, n2]]"""
        def hx(a):
            return " ".join(float(v).hex() for v in np.asarray(a, np.float32).reshape(-1))
        text = "".join(f"case {len(l1)} {len(l2)}\n{hx(H)}\n{hx(F)}\n{hx([h, f])}\n{hx(l1)}\n{hx(l2)}\n" for l1, l2, H, F, h, f in cases)
        setarch = shutil.which("setarch")  # no address randomisation for this one program, as in test_stager_cpu
        r = subprocess.run(([setarch, os.uname().machine, "-R"] if setarch else []) + [exe], input=text, capture_output=True,
                           text=True, timeout=300)  # (the program carries the sanitizers' runtimes itself)
        assert r.returncode == 0 and f"GATE OK {len(cases)}" in r.stdout, r.stdout[-500:] + r.stderr[-6000:]
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        lines = r.stdout.splitlines()
        out, at = [], 0
        for l1, l2, *_ in cases:
            assert lines[at] == f"case {len(l1)} {len(l2)}"
            rows = lines[at + 1:at + 1 + len(l1)]
            out.append(np.array([[ch == "1" for ch in row] for row in rows], bool).reshape(len(l1), len(l2)))
            at += 1 + len(l1)
        return out
    return run


def _model(c, H, F, h, f):
    d0, d1, se = gc.gates(c.loc1, c.loc2, H, F)
    h, f = float(np.float32(h)), float(np.float32(f))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(d0) & np.isfinite(d1) & np.isfinite(se) & (d0 < h) & (d1 < h) & (se < f)


@pytest.mark.parametrize("n1,n2,geometry", gc.CASES)
def test_gate_decisions_equal_the_float64_model(gate, n1, n2, geometry):
    c = gc.case(n1, n2, geometry)
    th = gc.pick_thresholds(n1, n2, geometry)
    got = gate([(c.loc1, c.loc2, c.H, c.F, h, f) for h, f in th])
    for (h, f), g in zip(th, got):
        ref = _model(c, c.H, c.F, h, f)
        assert np.array_equal(g, ref), (h, f, np.argwhere(g != ref)[:5].tolist())
        if c.vanish >= 0:
            assert not g[c.vanish].any()
    assert got[2].sum() >= got[0].sum() >= got[3].sum() and got[1].sum() >= got[0].sum()   # one gate alone passes no less


def test_vanishing_line_row_and_zero_matrices_pass_nothing(gate):
    c = gc.case(300, 333, "projective")
    loc1 = np.concatenate([np.array([gc.VANISH], np.float32), c.loc1])
    zero = np.zeros((3, 3), np.float32)
    a, b, z, zz = gate([(loc1, c.loc2, c.H, c.F, gc.OFF, gc.OFF), (loc1, c.loc2, zero, c.F, gc.OFF, gc.OFF),
                        (loc1, c.loc2, c.H, zero, gc.OFF, gc.OFF), (loc1, c.loc2, zero, zero, gc.OFF, gc.OFF)])
    assert not a[0].any() and a[1:].sum() > 0.9 * a[1:].size      # x2 == 0 exactly: the row fails even with the bounds off
    assert not b.any() and not z.any() and not zz.any()
