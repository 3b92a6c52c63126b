"""The serial arithmetic of the estimator's refit (hessgpu_amd/csrc/hess_geom_refit.h: the scales, the normal matrix from the
moment sums, the cyclic Jacobi eigen solve, de-normalisation, the sign rule, the decision) on the CPU under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/geom_refit_main.cpp runs the header's functions -- the ones geom_refit_kernel runs on one lane
-- on sums that tests/refit_cases.py computes in float64, and its candidate is compared with numpy's eigh solution.

Tolerance: the candidate is a unit-norm matrix rounded to float32 (2^-24 per entry at the most, 8 x 2^-24 allowed as in the
estimator's own tests); the double-precision eigen solve adds about 1e-15 kappa, below it for kappa <= 1e6.  Where the smallest
eigenvalue is not simple (collinear inliers) any vector of its eigenspace is right: there the Rayleigh quotient is compared."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import geom_cases as g
import refit_cases as rc
from test_stager_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hessgpu_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def refit(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    exe = str(tmp_path_factory.mktemp("geom_refit") / "geom_refit_main")
    build = subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "geom_refit_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return functools.partial(_run, exe)


def _run(exe, cases):
    text = "\n".join(" ".join(repr(float(t)) for t in c) for c in cases) + "\n"
    setarch = shutil.which("setarch")  # no address randomisation for this one program, as in test_stager_cpu
    r = subprocess.run(([setarch, os.uname().machine, "-R"] if setarch else []) + [exe], input=text, capture_output=True, text=True,
                       timeout=120)  # (the program carries the sanitizers' runtimes itself)
    assert r.returncode == 0 and f"REFIT OK {len(cases)}" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            v = [float(x) for x in w[5:]]
            out.append(dict(stop=int(w[1]), sweeps=int(w[2]), finite=int(w[3]), decision=int(w[4]), x=np.array(v[:9]),
                            C=np.array(v[9:18], np.float32).reshape(3, 3), N=np.array(v[18:]).reshape(9, 9)))
    assert len(out) == len(cases)
    return out


def _tokens(model, p1, p2, prev, counts=(0, 0, 0)):
    """The program's input for the correspondences p1 -> p2 (all inliers) and the matrix before."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, c2 = p1.mean(0), p2.mean(0)
    sd1, sd2 = np.sqrt(((p1 - c1) ** 2).sum(1)).sum(), np.sqrt(((p2 - c2) ** 2).sum(1)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        s1, s2 = np.sqrt(2) * len(p1) / sd1, np.sqrt(2) * len(p1) / sd2
        sums = rc.moments(model, (p1 - c1) * s1, (p2 - c2) * s2)
    sums = np.where(np.isfinite(sums), sums, 0.0)
    return [g.MODEL_ID[model], len(p1), sd1, sd2, *c1, *c2, *np.asarray(prev, np.float64).reshape(9), *sums, *counts]


def _inliers(name):
    c = g.case(name)
    return c, c.p1[c.planted], c.p2[c.planted]


def test_candidate_against_numpy(refit):
    """Noisy inliers (a simple smallest eigenvalue), exact data (N singular) and k inliers only."""
    cases, want = [], []
    for key, seed in rc.NOISY.items():
        c = rc.noisy(*key, seed)
        M, S, _ = rc.ransac64(c)
        cases.append(_tokens(c.model, c.p1[S], c.p2[S], M))
        want.append((c.name, c.model, c.p1[S], c.p2[S], M))
    for name in ("H 300", "F 300", "H 1031", "F 1031", "clean"):
        c, a, b = _inliers(name)
        prev = -c.truth / np.linalg.norm(c.truth)                   # (the sign rule has to turn the candidate)
        cases.append(_tokens(c.model, a, b, prev))
        want.append((name + " exact", c.model, a, b, prev))
        k = g.K[c.model]
        idx = g.sample(c.seed, c.allin[0], k, c.n) if name != "clean" else g.sample(c.seed, 0, k, c.n)
        cases.append(_tokens(c.model, c.p1[idx], c.p2[idx], prev))
        want.append((name + " k inliers", c.model, c.p1[idx], c.p2[idx], prev))
    got = refit(cases)
    worst = 0.0
    for r, (name, model, a, b, prev) in zip(got, want):
        nm = rc.normal64(model, a, b)
        assert r["stop"] == 0 and r["finite"] == 1 and 1 <= r["sweeps"] <= 12, (name, r["sweeps"])
        assert np.abs(r["N"] - nm.N).max() <= 1e-12 * np.abs(nm.N).max(), name
        assert nm.kappa <= rc.MAX_KAPPA, (name, nm.kappa)
        C = rc.denormalise64(model, nm.x, nm)
        C = C if (C * prev).sum() >= 0 else -C
        d = float(np.linalg.norm(r["C"].astype(np.float64) - C))
        worst = max(worst, d / rc.TOL)
        assert d <= rc.TOL, (name, d, rc.TOL, nm.kappa)
        assert (r["C"].astype(np.float64) * prev).sum() >= 0, name
        assert abs(np.linalg.norm(r["C"].astype(np.float64)) - 1) <= 1e-6
        if model == "F":
            assert np.linalg.svd(r["C"].astype(np.float64))[1][2] <= 1e-6
    print(f"{len(got)} cases, largest distance / (8 x 2^-24): {worst:.3f}")


def test_collinear_inliers(refit):
    """Every first point on one line: the null space of N has more than one dimension.  The eigenvector the program returns is of
    unit length and its Rayleigh quotient is the smallest eigenvalue up to rounding; the candidate is finite and of unit norm."""
    cases, Ns = [], []
    for model in ("H", "F"):
        c = g.degenerate("collinear", model)
        cases.append(_tokens(model, c.p1, c.p2, np.eye(3)))
        Ns.append(rc.normal64(model, c.p1, c.p2))
    for r, nm in zip(refit(cases), Ns):
        x = r["x"]
        assert r["stop"] == 0 and r["finite"] == 1 and abs(np.linalg.norm(x) - 1) <= 1e-12
        assert abs(x @ nm.N @ x - nm.lam[0]) <= 1e-12 * nm.lam[8]
        assert np.isfinite(r["C"]).all() and abs(np.linalg.norm(r["C"].astype(np.float64)) - 1) <= 1e-6


def test_stops_and_decisions(refit):
    c, a, b = _inliers("H 300")
    same = np.repeat(a[:1], 8, 0)
    tok = _tokens("H", same, same, np.eye(3))                       # coincident points: a mean distance of zero
    nan = _tokens("H", a, b, np.eye(3))
    nan[2] = float("nan")
    dec = [_tokens("H", a, b, np.eye(3), counts) for counts in ((10, 9, 1), (10, 10, 0), (10, 10, 2), (10, 12, 2))]
    got = refit([tok, nan] + dec)
    assert got[0]["stop"] == 1 and got[1]["stop"] == 1
    assert [r["decision"] for r in got[2:]] == [0, 2, 1, 1]         # discard, accept and stop, accept, accept
