#!/usr/bin/env python3
"""Device time per pair of Matcher.estimate_pairs (H and F, T hypotheses) next to match_pairs' own time for the same
pairs, on the GPU.

Banks: the two of tools/bench_match_pairs.py (16 sets x 4096 descriptors, all 120 pairs; 64 sets x 2048, window 8) with a
location per descriptor: every pool row has a point in a reference image, and set k sees it through a mild homography of
its own, so the matches of a pair fit a homography (and the run finds it).  The budget is fixed, so the time depends on the
number of matches and T only, not on how good the matches are; the "full lists" rows feed every pair a list of
max_match identity matches, the most a pair can have.  --refit R [R ...] adds a row per form and R with at most R least-squares
refits on the inliers (hess_geom_params.refit) and reports the refits that were accepted.  Forms alternate `--reps` times; medians and ranges of device time
(hipEvents around the call's kernels: last_ms) are reported.  Prints a text table; --out also writes it to a file."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from hessgpu_amd.matcher import Matcher, all_pairs, window_pairs

WORKLOADS = {"16x4096_all": (16, 4096, None), "64x2048_window8": (64, 2048, 8)}
BOUND = {"H": 8.0, "F": 4.0}


def make_bank(nsets, n, seed, size=4096.0):
    """bench_match_pairs.make_sets with the pool rows remembered: -> (descriptor sets, location sets)."""
    rng = np.random.RandomState(seed)
    pool = (rng.rand(4 * n, 128) * 78).astype(np.int32)
    ref = rng.rand(4 * n, 2) * size
    sets, locs = [], []
    for _ in range(nsets):
        idx = rng.choice(len(pool), n, replace=False)
        sets.append(np.clip(pool[idx] + rng.randint(-4, 5, (n, 128)), 0, 255).astype(np.uint8))
        H = np.eye(3) + np.array([[0.1, 0.1, 40.0], [0.1, 0.1, 40.0], [1e-5, 1e-5, 0.0]]) * (rng.rand(3, 3) * 2 - 1)
        x = np.concatenate([ref[idx], np.ones((n, 1))], 1) @ H.T
        locs.append((x[:, :2] / x[:, 2:]).astype(np.float32))
    return sets, locs


def run(name, reps, T, lines, refits=()):
    nsets, n, w = WORKLOADS[name]
    sets, locs = make_bank(nsets, n, seed=nsets)
    pairs = all_pairs(nsets) if w is None else window_pairs(nsets, w)
    m = Matcher(0, max_sift=n)
    m.set_bank(sets)
    m.set_bank_locations(locs)
    matches = m.match_pairs(pairs, max_match=n)
    full = [np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)] * len(pairs)
    forms = [("match_pairs", None, None, 0)] + [(f"estimate_pairs {md}, {kind}" + (f", refit {r}" if r else ""), md, lst, r)
                                                for lst, kind in ((matches, "match_pairs' lists"), (full, "full lists"))
                                                for md in ("H", "F") for r in (0,) + tuple(refits)]
    times = {f[0]: [] for f in forms}
    found = {}
    for rep in range(reps + 1):                      # the first round warms up
        for label, md, lst, refit in forms:
            if md is None:
                m.match_pairs(pairs, max_match=n)
            else:
                out = m.estimate_pairs(pairs, lst, md, BOUND[md], hypotheses=T, seed=1, refit=refit, info=True)
                found[label] = (sum(int(o[1].sum()) for o in out), sum(o[2] >= 0 for o in out), sum(o[3]["refits"] for o in out))
            if rep:
                times[label].append(m.last_ms() / len(pairs))
    m.close()
    mean = float(np.mean([len(x) for x in matches]))
    lines.append(f"{name}: {len(pairs)} pairs, {mean:.0f} matches per pair on average (full lists: {n}), T = {T}, reps = {reps}")
    for label, md, lst, refit in forms:
        t = times[label]
        extra = ""
        if md is not None:
            per = mean if lst is matches else n
            extra = f"   {per * T / (np.median(t) * 1e-3) / 1e9:8.1f} G gate evaluations/s   models {found[label][1]}, inliers {found[label][0]}"
            extra += f", accepted refits {found[label][2]}" if refit else ""
        lines.append(f"  {label:54s} {np.median(t):9.5f} ms/pair  [{min(t):.5f}, {max(t):.5f}]{extra}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hypotheses", type=int, default=2048)
    ap.add_argument("--refit", type=int, nargs="*", default=[], help="also time the calls with these values of refit (1..8)")
    ap.add_argument("--out", help="also write the table here")
    args = ap.parse_args()
    lines = ["tools/bench_estimate.py: device time per pair (hipEvents around the call's kernels), median [min, max]"]
    for nm in (sorted(WORKLOADS) if args.workload == "all" else [args.workload]):
        run(nm, args.reps, args.hypotheses, lines, args.refit)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
