#!/usr/bin/env python3
"""Device and wall time per pair of hess_matcher_verify_pairs next to the chain of calls it replaces (match_pairs,
estimate_pairs, the guided geometry built on the host, match_pairs_guided, estimate_pairs on the guided matches), on the GPU.

Banks and locations: those of tools/bench_estimate.py (16 sets x 4096 descriptors, all 120 pairs; 64 sets x 2048, window 8).
Models H (bound 8) and F (bound 4), T = 2048 hypotheses, refit 0 and 2, final_estimate on, inlier masks taken, putative lists
not.  Both forms call the C entry points on the same matcher with output arrays allocated once, so the wall time is the
calls' own (for the chain plus the numpy lines that build the geometry table).  The chain and the one call alternate `--reps`
times after one warm-up round; medians and ranges are reported: device time (the sum of last_ms over the calls: hipEvents
around each call's kernels) and wall time (time.perf_counter around the calls), and for the chain the wall time of every step.
The two forms' results are compared byte for byte in every round.  --parent-lib PATH also times both forms of another build of
libhessgpu.so (the parent commit's) on a matcher of its own in the same run, alternating with this build's, and compares its
results with this build's.  Prints a text table; --out also writes it."""
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
from hessgpu_amd import matcher as hm

T = 2048
STEPS = ("match", "estimate", "geometry (host)", "guided match", "final estimate")


class OtherBuild:
    """A matcher of another libhessgpu.so with the bank and its locations, loaded beside this build's (the libraries bind their
    own symbols): what Forms needs of a Matcher."""

    def __init__(self, path, sets, locs, max_sift):
        L = self.L = C.CDLL(os.path.abspath(path))
        P = C.c_void_p
        L.hess_matcher_create.restype = P
        L.hess_matcher_create.argtypes = [C.c_int, C.c_int]
        L.hess_matcher_destroy.argtypes = [P]
        L.hess_matcher_bank_set.argtypes = [P, C.c_int, P, P]
        L.hess_matcher_bank_set_locations.argtypes = [P, P, C.c_size_t]
        L.hess_matcher_match_pairs.argtypes = [P, C.c_int, P, C.c_int, P, P, C.c_float, C.c_float, C.c_int]
        L.hess_matcher_match_pairs_guided.argtypes = [P, C.c_int, P, P, C.c_int, P, P, C.c_float, C.c_float, C.c_int]
        L.hess_matcher_estimate_pairs.argtypes = [P, C.c_int, P, C.c_int, P, P, P, P, P]
        L.hess_matcher_verify_pairs.argtypes = [P, C.c_int, P, P, C.c_int, P, P, P, P, P]
        L.hess_matcher_last_ms.restype = C.c_float
        L.hess_matcher_last_ms.argtypes = [P]
        L.hess_matcher_last_error.restype = C.c_char_p
        L.hess_matcher_last_error.argtypes = [P]
        self.h = L.hess_matcher_create(0, max_sift)
        counts = np.array([len(s) for s in sets], np.int32)
        flat = np.ascontiguousarray(np.concatenate(sets))
        xy = np.ascontiguousarray(np.concatenate(locs), dtype=np.float32)
        if (not self.h or L.hess_matcher_bank_set(self.h, len(counts), counts.ctypes.data, flat.ctypes.data) < 0
                or L.hess_matcher_bank_set_locations(self.h, xy.ctypes.data, 8) < 0):
            raise RuntimeError(f"{path}: no matcher, no bank or no locations")

    def last_ms(self):
        return float(self.L.hess_matcher_last_ms(self.h))

    def close(self):
        self.L.hess_matcher_destroy(self.h)


class Forms:
    def __init__(self, m, pairs, n, model, refit):
        self.m, self.ab, self.n, self.np = m, hm.check_pairs(pairs), n, len(pairs)
        self.P = hm.Matcher._verify_params(model, BOUND[model], T, 1, refit, None, True, 0.7, 0.8, True)
        self.g = self.P["geom"].copy()
        self.model = model
        z = lambda *shape, dt=np.int32: np.zeros(shape, dt)
        k = self.np
        self.c = dict(put=z(k, n, 2), nput=z(k), res1=z(k, dt=hm.GEOM_RESULT_DTYPE), out=z(k, n, 2), cnt=z(k),
                      res2=z(k, dt=hm.GEOM_RESULT_DTYPE), mask=z(k, n, dt=np.uint8))
        self.v = dict(out=z(k, n, 2), cnt=z(k), res=z(k, dt=hm.VERIFY_RESULT_DTYPE), mask=z(k, n, dt=np.uint8))

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError(f"hess error {rc}: {self.m.L.hess_matcher_last_error(self.m.h).decode()}")

    def chain(self):
        """-> (device ms, wall ms per step)"""
        L, h, c, k, n, ab = self.m.L, self.m.h, self.c, self.np, self.n, self.ab
        ms, t = 0.0, [time.perf_counter()]
        self._ok(L.hess_matcher_match_pairs(h, k, ab.ctypes.data, n, c["put"].ctypes.data, c["nput"].ctypes.data, 0.7, 0.8, 1))
        ms += self.m.last_ms()
        t.append(time.perf_counter())
        self._ok(L.hess_matcher_estimate_pairs(h, k, ab.ctypes.data, n, c["put"].ctypes.data, c["nput"].ctypes.data, self.g.ctypes.data,
                                               c["res1"].ctypes.data, None))
        ms += self.m.last_ms()
        t.append(time.perf_counter())
        M = c["res1"]["M"].reshape(k, 3, 3)
        geo = hm.guided_pairs(k, H=M, hdistmax=BOUND["H"]) if self.model == "H" else hm.guided_pairs(k, F=M, fdistmax=BOUND["F"])
        t.append(time.perf_counter())
        self._ok(L.hess_matcher_match_pairs_guided(h, k, ab.ctypes.data, geo.ctypes.data, n, c["out"].ctypes.data, c["cnt"].ctypes.data,
                                                   0.7, 0.8, 1))
        ms += self.m.last_ms()
        t.append(time.perf_counter())
        self._ok(L.hess_matcher_estimate_pairs(h, k, ab.ctypes.data, n, c["out"].ctypes.data, c["cnt"].ctypes.data, self.g.ctypes.data,
                                               c["res2"].ctypes.data, c["mask"].ctypes.data))
        ms += self.m.last_ms()
        t.append(time.perf_counter())
        return ms, [(b - a) * 1e3 for a, b in zip(t, t[1:])]

    def verify(self):
        L, h, v = self.m.L, self.m.h, self.v
        t0 = time.perf_counter()
        self._ok(L.hess_matcher_verify_pairs(h, self.np, self.ab.ctypes.data, self.P.ctypes.data, self.n, v["out"].ctypes.data,
                                             v["cnt"].ctypes.data, v["res"].ctypes.data, v["mask"].ctypes.data, None))
        t1 = time.perf_counter()
        return self.m.last_ms(), (t1 - t0) * 1e3

    def compare(self):
        c, v = self.c, self.v
        assert np.array_equal(c["cnt"], v["cnt"]) and np.array_equal(c["nput"], v["res"]["nputative"]), "counts differ"
        assert c["res1"].tobytes() == v["res"]["putative"].tobytes() and c["res2"].tobytes() == v["res"]["final"].tobytes(), "results differ"
        assert c["mask"].tobytes() == v["mask"].tobytes(), "masks differ"
        assert all(np.array_equal(c["out"][p, :c["cnt"][p]], v["out"][p, :c["cnt"][p]]) for p in range(self.np)), "matches differ"


def _fmt(x):
    return f"{np.median(x):9.5f} [{min(x):.5f}, {max(x):.5f}]"


def run(name, reps, lines, parent_lib=None):
    nsets, n, w = WORKLOADS[name]
    sets, locs = make_bank(nsets, n, seed=nsets)
    pairs = hm.all_pairs(nsets) if w is None else hm.window_pairs(nsets, w)
    m = hm.Matcher(0, max_sift=n)
    m.set_bank(sets)
    m.set_bank_locations(locs)
    builds = [("", m)] + ([(", the other build", OtherBuild(parent_lib, sets, locs, n))] if parent_lib else [])
    k = len(pairs)
    lines.append(f"{name}: {k} pairs of {n} x {n}, T = {T}, reps = {reps}; ms per pair, median [min, max]")
    for model in ("H", "F"):
        for refit in (0, 2):
            fs = [Forms(b, pairs, n, model, refit) for _, b in builds]
            f = fs[0]
            labels = [form + tag for tag, _ in builds for form in ("chain", "verify_pairs")]
            dev = {label: [] for label in labels}
            wall = {label: [] for label in labels}
            steps = [[[] for _ in STEPS] for _ in builds]
            for rep in range(reps + 1):                  # the first round warms up
                for (tag, _), g, st in zip(builds, fs, steps):
                    d, ts = g.chain()
                    vd, vw = g.verify()
                    g.compare()
                    assert all(g.v[x].tobytes() == f.v[x].tobytes() for x in f.v), "the two builds' results differ"
                    if rep:
                        dev["chain" + tag].append(d / k)
                        wall["chain" + tag].append(sum(ts) / k)
                        dev["verify_pairs" + tag].append(vd / k)
                        wall["verify_pairs" + tag].append(vw / k)
                        for s_, x in zip(st, ts):
                            s_.append(x / k)
            lines.append(f"  model {model}, refit {refit}: {float(np.mean(f.c['nput'])):.0f} putative, {float(np.mean(f.c['cnt'])):.0f} guided "
                         f"matches per pair, {int((f.c['res1']['hypothesis'] >= 0).sum())} of {k} pairs with a model")
            lines.append(f"    {'form':50s} {'device':>31s}   {'wall':>31s}")
            for label in labels:
                lines.append(f"    {label:50s} {_fmt(dev[label])}   {_fmt(wall[label])}")
            for (tag, _), st in zip(builds, steps):
                for label, s_ in zip(STEPS, st):
                    lines.append(f"    {'chain: ' + label + tag:50s} {'':31s}   {_fmt(s_)}")
            lines.append(f"    wall, chain / verify_pairs: {np.median(wall['chain']) / np.median(wall['verify_pairs']):.2f}; "
                         f"device, verify_pairs / chain: {np.median(dev['verify_pairs']) / np.median(dev['chain']):.3f}")
    for _, b in builds:
        b.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="another build of libhessgpu.so whose two forms are timed alternately with this build's")
    ap.add_argument("--out", help="also write the table here")
    args = ap.parse_args()
    lines = ["tools/bench_verify_pairs.py: time per pair, device (hipEvents around each call's kernels) and wall (the calls themselves)"]
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
