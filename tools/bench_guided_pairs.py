#!/usr/bin/env python3
"""Device and wall time per pair of Matcher.match_pairs_guided (H only, F only, both) next to match_pairs and next to the
per-pair loop that was the only way to match a bank pair guided before (set_descriptors x 2, set_locations x 2, match(H, F)),
on the GPU.

Banks and locations: those of tools/bench_estimate.py (16 sets x 4096 descriptors, all 120 pairs; 64 sets x 2048, window 8).
Matrices: what estimate_pairs returns for match_pairs' lists (H with bound 8 and one refit, F with bound 4), the bounds those
of the estimate.  The per-pair loop runs the first 16 pairs with both matrices.  --parent-lib PATH also times match_pairs of
another build of libhessgpu.so (the parent commit's) in the same run, alternating with this build's.  Forms alternate
`--reps` times after one warm-up round; medians and ranges are reported: device time (hipEvents around the call's kernels:
last_ms) and wall time (the whole call, uploads and compaction included).  Prints a text table; --out also writes it."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from bench_estimate import BOUND, WORKLOADS, make_bank
from hessgpu_amd.matcher import Matcher, all_pairs, window_pairs

LOOP_PAIRS = 16


class OtherBuild:
    """match_pairs of another libhessgpu.so, loaded beside this build's (the libraries bind their own symbols)."""

    def __init__(self, path, sets, max_sift):
        L = self.L = C.CDLL(os.path.abspath(path))
        L.hess_matcher_create.restype = C.c_void_p
        L.hess_matcher_create.argtypes = [C.c_int, C.c_int]
        L.hess_matcher_destroy.argtypes = [C.c_void_p]
        L.hess_matcher_bank_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hess_matcher_match_pairs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                               C.c_float, C.c_int]
        L.hess_matcher_last_ms.restype = C.c_float
        L.hess_matcher_last_ms.argtypes = [C.c_void_p]
        self.h = L.hess_matcher_create(0, max_sift)
        counts = np.array([len(s) for s in sets], np.int32)
        flat = np.ascontiguousarray(np.concatenate(sets))
        if not self.h or L.hess_matcher_bank_set(self.h, len(counts), counts.ctypes.data, flat.ctypes.data) < 0:
            raise RuntimeError(f"{path}: no matcher or no bank")

    def match_pairs(self, pairs, max_match):
        out = np.zeros((len(pairs), max_match, 2), np.int32)
        cnt = np.zeros(len(pairs), np.int32)
        if self.L.hess_matcher_match_pairs(self.h, len(pairs), pairs.ctypes.data, max_match, out.ctypes.data, cnt.ctypes.data,
                                           0.7, 0.8, 1) < 0:
            raise RuntimeError("match_pairs of the other build failed")
        return [out[k, :cnt[k]].copy() for k in range(len(pairs))]

    def last_ms(self):
        return float(self.L.hess_matcher_last_ms(self.h))

    def close(self):
        self.L.hess_matcher_destroy(self.h)


def run(name, reps, lines, parent_lib):
    nsets, n, w = WORKLOADS[name]
    sets, locs = make_bank(nsets, n, seed=nsets)
    pairs = all_pairs(nsets) if w is None else window_pairs(nsets, w)
    m, one = Matcher(0, max_sift=n), Matcher(0, max_sift=n)
    m.set_bank(sets)
    m.set_bank_locations(locs)
    matches = m.match_pairs(pairs, max_match=n)
    Hs = np.stack([e[0] for e in m.estimate_pairs(pairs, matches, "H", BOUND["H"], seed=1, refit=1)])
    Fs = np.stack([e[0] for e in m.estimate_pairs(pairs, matches, "F", BOUND["F"], seed=1)])
    other = OtherBuild(parent_lib, sets, n) if parent_lib else None
    nloop = min(LOOP_PAIRS, len(pairs))

    def loop():
        ms, out = 0.0, []
        for p in range(nloop):
            a, b = pairs[p]
            one.set_descriptors(0, sets[a])
            one.set_descriptors(1, sets[b])
            one.set_locations(0, locs[a])
            one.set_locations(1, locs[b])
            out.append(one.match(max_match=n, H=Hs[p], F=Fs[p], hdistmax=BOUND["H"], fdistmax=BOUND["F"]))
            ms += one.last_ms()
        return out, ms

    forms = [("match_pairs", len(pairs), lambda: (m.match_pairs(pairs, max_match=n), m.last_ms()))]
    if other:
        forms.append(("match_pairs, the other build", len(pairs), lambda: (other.match_pairs(pairs, n), other.last_ms())))
    forms += [
        ("match_pairs_guided, H only", len(pairs),
         lambda: (m.match_pairs_guided(pairs, H=Hs, hdistmax=BOUND["H"], max_match=n), m.last_ms())),
        ("match_pairs_guided, F only", len(pairs),
         lambda: (m.match_pairs_guided(pairs, F=Fs, fdistmax=BOUND["F"], max_match=n), m.last_ms())),
        ("match_pairs_guided, H and F", len(pairs),
         lambda: (m.match_pairs_guided(pairs, H=Hs, F=Fs, hdistmax=BOUND["H"], fdistmax=BOUND["F"], max_match=n), m.last_ms())),
        (f"per-pair loop, H and F (first {nloop} pairs)", nloop, loop),
    ]
    dev = {f[0]: [] for f in forms}
    wall = {f[0]: [] for f in forms}
    found = {}
    for rep in range(reps + 1):                      # the first round warms up
        for label, np_, call in forms:
            t0 = time.perf_counter()
            out, ms = call()
            t1 = time.perf_counter()
            found[label] = out
            if rep:
                dev[label].append(ms / np_)
                wall[label].append((t1 - t0) * 1e3 / np_)
    both, lp = found["match_pairs_guided, H and F"], found[forms[-1][0]]
    assert all(np.array_equal(both[p], lp[p]) for p in range(nloop)), "the batched call and the per-pair loop disagree"
    if other:
        assert all(np.array_equal(x, y) for x, y in zip(found["match_pairs"], found["match_pairs, the other build"]))
    lines.append(f"{name}: {len(pairs)} pairs of {n} x {n}, reps = {reps}; ms per pair, median [min, max]")
    lines.append(f"  {'form':46s} {'device':>31s}   {'wall':>31s}   matches per pair")
    for label, np_, _ in forms:
        d, wl = dev[label], wall[label]
        mean = float(np.mean([len(x) for x in found[label]]))
        lines.append(f"  {label:46s} {np.median(d):9.5f} [{min(d):.5f}, {max(d):.5f}]   {np.median(wl):9.5f} [{min(wl):.5f}, {max(wl):.5f}]"
                     f"   {mean:7.0f}")
    ratio = np.median(wall[forms[-1][0]]) / np.median(wall["match_pairs_guided, H and F"])
    lines.append(f"  wall time per pair, per-pair loop / batched call (H and F): {ratio:.1f}")
    m.close()
    one.close()
    if other:
        other.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="another build of libhessgpu.so whose match_pairs is timed alternately with this build's")
    ap.add_argument("--out", help="also write the table here")
    args = ap.parse_args()
    lines = ["tools/bench_guided_pairs.py: time per pair, device (hipEvents around the call's kernels) and wall (the whole call)"]
    for nm in (sorted(WORKLOADS) if args.workload == "all" else [args.workload]):
        run(nm, args.reps, lines, args.parent_lib)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
