#!/usr/bin/env python3
"""Batched matching against the per-pair loop, on the GPU.

  (a) what a SiftMatchGPU caller runs per pair: set_descriptors(0, A), set_descriptors(1, B), match();
  (b) one bank build (set_bank) and one match_pairs call over all the pairs.

Workloads: 16 sets x 4096 descriptors, all 120 pairs; 64 sets x 2048, window 8.  Per workload and form: wall time per
pair (host clock around work that ends in a synchronise), device time per pair (hipEvents: last_ms), aggregate TMAC/s
(sum of n1 n2 dim over device time, dim = the descriptor length actually multiplied) and its share of the dense i8 peak
DESIGN section 4 uses.  The two forms' matches are compared pair by pair.  The forms alternate `--reps` times; the medians
are reported, with the range of device time per pair over the repetitions.  Prints one JSON object.

  --dim 64   the sets are 64-d (-half descriptors) on a Matcher(dim=64);
  --pad      the same 64-d sets with 64 zero columns appended on a 128-d matcher: how a caller got the same matches before
             the matcher took 64-d sets (dot products of unsigned bytes are unchanged by zero columns)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from hessgpu_amd.matcher import Matcher, all_pairs, window_pairs

PEAK_TMAC = 2500.0   # dense i8 MFMA peak, DESIGN section 4
WORKLOADS = {"16x4096_all": (16, 4096, None), "64x2048_window8": (64, 2048, 8)}


def make_sets(nsets, n, seed, dim=128):
    """Descriptor-like sets: one pool of SIFT-range bytes, noisy copies of its rows, so that pairs have matches."""
    rng = np.random.RandomState(seed)
    amp = 78 if dim == 128 else 110                        # norm about 512, as the matcher expects
    pool = (rng.rand(4 * n, dim) * amp).astype(np.int32)
    return [np.clip(pool[rng.choice(len(pool), n, replace=False)] + rng.randint(-4, 5, (n, dim)), 0, 255).astype(np.uint8)
            for _ in range(nsets)]


def per_pair(m, sets, pairs, max_match):
    dev = 0.0
    out = []
    t0 = time.perf_counter()
    for a, b in pairs:
        m.set_descriptors(0, sets[a])
        m.set_descriptors(1, sets[b])
        out.append(m.match(max_match=max_match))
        dev += m.last_ms()
    return time.perf_counter() - t0, dev, out


def batched(m, sets, pairs, max_match):
    t0 = time.perf_counter()
    m.set_bank(sets)
    t1 = time.perf_counter()
    out = m.match_pairs(pairs, max_match=max_match)
    t2 = time.perf_counter()
    return t2 - t0, m.last_ms(), out, t1 - t0


def run(name, reps, max_match, dim=128, pad=False):
    nsets, n, w = WORKLOADS[name]
    sets = make_sets(nsets, n, seed=nsets, dim=dim)
    if pad:
        sets = [np.ascontiguousarray(np.concatenate([s, np.zeros((len(s), 128 - s.shape[1]), np.uint8)], 1)) for s in sets]
    mdim = sets[0].shape[1]                               # the length the matcher multiplies
    pairs = all_pairs(nsets) if w is None else window_pairs(nsets, w)
    macs = float(sum(len(sets[a]) * len(sets[b]) * mdim for a, b in pairs))
    m = Matcher(0, max_sift=n, dim=mdim)
    per_pair(m, sets, pairs[:4], max_match)          # warm-up: code objects, allocations, both paths
    batched(m, sets, pairs, max_match)
    A, B = [], []
    for _ in range(reps):
        wa, da, oa = per_pair(m, sets, pairs, max_match)
        wb, db, ob, bank_s = batched(m, sets, pairs, max_match)
        same = len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob))
        if not same:
            raise SystemExit(f"{name}: batched matches differ from the per-pair loop")
        A.append((wa, da))
        B.append((wb, db, bank_s))
    m.close()
    npairs = len(pairs)

    def form(wall_s, dev_ms):
        tmac = macs / (dev_ms * 1e-3) / 1e12
        return {"wall_ms_per_pair": round(wall_s * 1e3 / npairs, 4), "device_ms_per_pair": round(dev_ms / npairs, 4),
                "TMAC_per_s": round(tmac, 1), "share_of_i8_peak": round(tmac / PEAK_TMAC, 4)}

    a = form(float(np.median([x[0] for x in A])), float(np.median([x[1] for x in A])))
    b = form(float(np.median([x[0] for x in B])), float(np.median([x[1] for x in B])))
    b["bank_build_ms"] = round(float(np.median([x[2] for x in B])) * 1e3, 3)
    b["bank_build_ms_range"] = [round(min(x[2] for x in B) * 1e3, 3), round(max(x[2] for x in B) * 1e3, 3)]
    a["device_ms_per_pair_range"] = [round(min(x[1] for x in A) / npairs, 4), round(max(x[1] for x in A) / npairs, 4)]
    b["device_ms_per_pair_range"] = [round(min(x[1] for x in B) / npairs, 4), round(max(x[1] for x in B) / npairs, 4)]
    return {"workload": name, "sets": nsets, "descriptors": n, "dim": dim, "padded_to_128": bool(pad), "matcher_dim": mdim,
            "pairs": npairs, "matches": int(sum(len(x) for x in ob)),
            "per_pair_loop": a, "bank_match_pairs": b,
            "wall_speedup": round(a["wall_ms_per_pair"] / b["wall_ms_per_pair"], 2),
            "device_speedup": round(a["device_ms_per_pair"] / b["device_ms_per_pair"], 2),
            "reps": reps, "results_equal": True}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-match", type=int, default=4096)
    ap.add_argument("--dim", type=int, choices=(128, 64), default=128, help="descriptor length of the sets")
    ap.add_argument("--pad", action="store_true", help="build the 64-d sets, match them zero-padded on a 128-d matcher")
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()
    dim = 64 if args.pad else args.dim
    names = sorted(WORKLOADS) if args.workload == "all" else [args.workload]
    res = {"tool": "tools/bench_match_pairs.py", "peak_TMAC_per_s": PEAK_TMAC,
           "results": [run(nm, args.reps, args.max_match, dim, args.pad) for nm in names]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
