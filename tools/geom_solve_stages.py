#!/usr/bin/env python3
"""Where the estimator's solve loses its digits, on the CPU: tools/geom_solve_stages.cpp repeats geom_hypothesis
(hess_geom.hip) on the host with the precision of normalisation, elimination and denormalisation selectable, and this
script holds its result against the float64 solve of tests/geom_cases.py on the samples of
tests/test_matcher_estimate_model_gpu.py::test_each_hypothesis_against_float64 -- the same ratio
d / max(d_np32, kappa 2^-24) that the test bounds by 8.  "fff" is the elimination in float32 (the kernel before the
elimination went to double), "fdf" the kernel as built.  Needs g++; no GPU.  Prints a table; --out also writes it."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import geom_cases as g

STAGES = ("fff", "dff", "fdf", "ffd", "ddf", "ddd")
VARIANTS = {0: "Gauss-Jordan", 1: "factor as a quotient", 2: "Gaussian elimination, back substitution"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the table here")
    a = ap.parse_args()
    lines = ["ratio d / max(d_np32, kappa 2^-24) of the host replica; stages: normalisation, elimination, denormalisation "
             "(f float32, d double)"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "geom_solve_stages")
        subprocess.run(["g++", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "geom_solve_stages.cpp")],
                       check=True)
        for name in g.SOLO:
            c, h = g.case(name), g.solo(name)
            pts = np.concatenate([c.p1[h.idx], c.p2[h.idx]], 2).reshape(len(h.idx), -1)
            text = "\n".join(" ".join(f"{v:.9g}" for v in row) for row in pts) + "\n"
            den = np.maximum(g.distance(h.M32, h.M), h.kappa * 2.0 ** -24)
            seeds = np.array(g.SOLO_SEEDS)[h.use]
            for cfg, variant in [(s, 0) for s in STAGES] + [("fff", 1), ("fff", 2)]:
                out = subprocess.run([exe, c.model, cfg, str(variant)], input=text, capture_output=True, text=True,
                                     check=True).stdout
                M = np.array([[float(v) for v in line.split()] for line in out.strip().split("\n")]).reshape(-1, 3, 3)
                M = g.finish64(c.model, M).astype(np.float32)
                r = (g.distance(M, h.M) / den)[h.use]
                lines.append(f"  {name:6s} {cfg}  {VARIANTS[variant]:40s} median {np.median(r):6.3f}  p99 {np.percentile(r, 99):7.3f}  "
                             f"max {r.max():7.3f} (seed {seeds[int(np.argmax(r))]})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
