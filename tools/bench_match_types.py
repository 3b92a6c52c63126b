#!/usr/bin/env python3
"""The matcher's feature-type gate, on the GPU (built on tools/bench_match_pairs.py: its workloads and sets).

  --ungated [--lib PATH]   bank + match_pairs WITHOUT types on 16 x 4096 all pairs and 64 x 2048 window 8: TMAC/s, device
                           time per pair (hess_matcher_last_ms), bank build.  --lib: another build of libhessgpu.so, e.g.
                           the parent commit's (only the entry points an ungated match needs are bound): the yardstick.
  --gated                  the same banks with types: three equal classes (row i has class i mod 3), and the class mix the
                           detector gives on the bench's 1080p images (measured here, drawn at random per row).  Per form:
                           device time per pair gated and ungated on the same bank, the arithmetic the plan predicts --
                           sum over classes of (rows padded to 256) x (columns padded to 128), over the ungated product --
                           and the bank build with types (set_bank + set_bank_types) against without.  Gated results are
                           checked against the ungated matcher on the class subsets for a few pairs.

Every figure is the median over --reps, with the range.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from bench_match_pairs import PEAK_TMAC, WORKLOADS, make_sets
from hessgpu_amd import matcher as hm
from hessgpu_amd.matcher import Matcher, all_pairs, window_pairs

UNGATED_ENTRY_POINTS = ("hess_matcher_create", "hess_matcher_destroy", "hess_matcher_set_max", "hess_matcher_bank_set",
                        "hess_matcher_bank_read", "hess_matcher_match_pairs", "hess_matcher_last_ms", "hess_matcher_last_error")


def matcher_of(lib_path, max_sift):
    """A Matcher on another build of the library, bound as far as an ungated bank match needs."""
    if not lib_path:
        return Matcher(0, max_sift=max_sift)
    ours = hm._lib()
    L = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    for name in UNGATED_ENTRY_POINTS:
        fn, ref = getattr(L, name), getattr(ours, name)
        fn.restype, fn.argtypes = ref.restype, ref.argtypes
    m = Matcher.__new__(Matcher)
    m.L, m._dim = L, 128
    m.h = L.hess_matcher_create(0, max_sift)
    if not m.h:
        raise SystemExit(f"hess_matcher_create failed in {lib_path}")
    return m


def med(v):
    return [round(float(np.median(v)), 5), round(float(min(v)), 5), round(float(max(v)), 5)]   # median, min, max


def workload(name):
    nsets, n, w = WORKLOADS[name]
    sets = make_sets(nsets, n, seed=nsets)
    pairs = all_pairs(nsets) if w is None else window_pairs(nsets, w)
    return sets, pairs, n


def ungated(name, reps, lib):
    sets, pairs, n = workload(name)
    macs = float(sum(len(sets[a]) * len(sets[b]) * 128 for a, b in pairs))
    m = matcher_of(lib, n)
    m.set_bank(sets)
    m.match_pairs(pairs)                                    # warm-up
    dev, build = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.set_bank(sets)
        build.append((time.perf_counter() - t0) * 1e3)
        out = m.match_pairs(pairs)
        dev.append(m.last_ms())
    m.close()
    return {"workload": name, "pairs": len(pairs), "matches": int(sum(len(x) for x in out)),
            "device_ms_per_pair": med([d / len(pairs) for d in dev]),
            "TMAC_per_s": med([macs / (d * 1e-3) / 1e12 for d in dev]), "bank_build_ms": med(build)}


def detector_mix(images=4):
    """Class shares of the detector on the bench's workload (1920 x 1080 synthetic blobs, top-K 4096)."""
    import fixtures
    import hessgpu_amd
    from hessgpu_amd import _abi

    g = hessgpu_amd.HessContext(0, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=4096)
    g.run(np.stack([fixtures.synthetic_blobs(1920, 1080, i) for i in range(images)]))
    t = np.concatenate([g.fetch(i)[0]["type"] & 3 for i in range(images)])
    g.close()
    return (np.bincount(t, minlength=4) / len(t)).tolist()


def predicted(types, pairs):
    """Sum over the pairs and classes of padded rows x padded columns, over the same of the ungated pairs."""
    cnt = [np.bincount(t & 3, minlength=4) for t in types]
    up = lambda x, k: -(-int(x) // k) * k
    g = sum(up(cnt[a][c], 256) * up(cnt[b][c], 128) for a, b in pairs for c in range(4) if cnt[a][c] and cnt[b][c])
    u = sum(up(len(types[a]), 256) * up(len(types[b]), 128) for a, b in pairs)
    return g / u


def gated(name, reps, mixes):
    sets, pairs, n = workload(name)
    m = Matcher(0, max_sift=n)
    out = {"workload": name, "pairs": len(pairs), "forms": {}}
    for label, shares in mixes.items():
        rng = np.random.RandomState(11)
        if shares is None:
            types = [(np.arange(len(s)) % 3).astype(np.uint16) for s in sets]
        else:
            types = [rng.choice(4, size=len(s), p=shares).astype(np.uint16) for s in sets]
        m.set_bank(sets)
        m.set_bank_types(types)
        got = m.match_pairs(pairs)                          # warm-up, and the check below
        m.set_bank_types(None)
        m.match_pairs(pairs)
        for k in range(0, len(pairs), max(len(pairs) // 4, 1)):
            a, b = pairs[k]
            ref = []
            for c in range(4):
                ia, ib = np.flatnonzero((types[a] & 3) == c), np.flatnonzero((types[b] & 3) == c)
                if len(ia) and len(ib):
                    m.set_descriptors(0, sets[a][ia])
                    m.set_descriptors(1, sets[b][ib])
                    r = m.match(max_match=len(ia))
                    ref.append(np.stack([ia[r[:, 0]], ib[r[:, 1]]], 1))
            ref = np.concatenate(ref)
            ref = ref[np.argsort(ref[:, 0], kind="stable")][:4096]
            if not np.array_equal(ref, got[k]):
                raise SystemExit(f"{name} {label}: gated pair {tuple(pairs[k])} differs from the ungated matcher per class")
        dev_u, dev_g, build_u, build_g = [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            m.set_bank(sets)
            build_u.append((time.perf_counter() - t0) * 1e3)
            m.match_pairs(pairs)
            dev_u.append(m.last_ms() / len(pairs))
            t0 = time.perf_counter()
            m.set_bank(sets)
            m.set_bank_types(types)
            build_g.append((time.perf_counter() - t0) * 1e3)
            res = m.match_pairs(pairs)
            dev_g.append(m.last_ms() / len(pairs))
        out["forms"][label] = {
            "class_shares": [round(float(x), 4) for x in np.bincount(np.concatenate(types) & 3, minlength=4) / sum(map(len, types))],
            "matches_gated": int(sum(len(x) for x in res)),
            "device_ms_per_pair_ungated": med(dev_u), "device_ms_per_pair_gated": med(dev_g),
            "gated_over_ungated_measured": round(float(np.median(dev_g) / np.median(dev_u)), 4),
            "gated_over_ungated_predicted": round(predicted(types, pairs), 4),
            "bank_build_ms_without_types": med(build_u), "bank_build_ms_with_types": med(build_g)}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ungated", action="store_true")
    ap.add_argument("--gated", action="store_true")
    ap.add_argument("--lib", help="another build of libhessgpu.so for --ungated")
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()
    names = sorted(WORKLOADS) if args.workload == "all" else [args.workload]
    res = {"tool": "tools/bench_match_types.py", "peak_TMAC_per_s": PEAK_TMAC, "lib": args.lib or "this build",
           "figures": "[median, min, max]"}
    if args.ungated:
        res["ungated"] = [ungated(nm, args.reps, args.lib) for nm in names]
    if args.gated:
        mix = detector_mix()
        res["detector_class_shares_1080p"] = [round(x, 4) for x in mix]
        res["gated"] = [gated(nm, args.reps, {"three_equal_classes": None, "detector_mix": mix}) for nm in names]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
