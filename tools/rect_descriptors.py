#!/usr/bin/env python3
"""Device time of the rectangle-descriptor launch (keys_have_orientation == -1) beside the oriented launch, one JSON line.

On one 1920x1080 synthetic image (tests/fixtures.py) the tool runs three key lists of 4096 entries on the current image
and reads the descriptor launch's device time from hess_profile_get(HESS_K_DESCRIPTOR):
  rect_24x24    4096 rectangles of 24 x 24 image pixels, flag -1
  rect_200x40   4096 rectangles of 200 x 40 image pixels, flag -1
  oriented      the 24 x 24 list's array with flag 1 (s = 24 a scale, o = 24 an angle): a path that existed before the mode
Per list: ms per launch (mean over --repeats launches after --warmup), the gathered pixels per entry -- counted on the
host from the rule, sum of the clipped cell boxes for a rectangle, 16 boxes of (2 |cos| + 2 |sin|) 3 s for an oriented
key -- and ns per thousand gathered pixels.  --check also runs tests/rect_cases.check_rectangles on the product context and
reports the worst deviation from the float64 model it saw."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import fixtures
import hessgpu_amd
from hessgpu_amd import _abi

W, H, N = 1920, 1080, 4096


def rect_list(w, h, seed):
    rng = np.random.RandomState(seed)
    r = np.empty((N, 4))
    r[:, 0] = rng.uniform(2.0, W - w - 2.0, N)
    r[:, 1] = rng.uniform(2.0, H - h - 2.0, N)
    r[:, 2], r[:, 3] = w, h
    return hessgpu_amd.rect_keys(r)


def level_scale(ctx, sigma):
    """Scale of the octave a caller key of scale `sigma` is binned to (default schedule: sigma0 1.6, three levels)."""
    n = len(ctx.geometry())
    step = 2.0 ** (0.5 / 3)
    for oc in range(n):
        for l in (1, 2, 3):
            s = 1.6 * 2.0 ** (l / 3.0) * 2.0 ** oc
            if s / step <= sigma < s * step:
                return 2.0 ** oc
    return 1.0 if sigma < 2.0 else 2.0 ** (n - 1)


def rect_pixels(ctx, w, h):
    """Pixels a rectangle of w x h image pixels gathers, well inside the plane: four cell rows of 2 spty rows each over the
    1.25 W columns of the box is what the kernel reads; the reference's 16 cells read 4 sptx spty each, the same number."""
    sc = level_scale(ctx, min(w, h) / 12.0)
    return 16 * (2 * (w / sc) / 4 + 1) * (2 * (h / sc) / 4 + 1)


def oriented_pixels(ctx, s, angle):
    sc = level_scale(ctx, s)
    b = (abs(math.cos(angle)) + abs(math.sin(angle))) * 3.0 * s / sc
    return 16 * (2 * b + 1) ** 2


def timed(ctx, keys, flag, warmup, repeats):
    for _ in range(warmup):
        ctx.run_keypoints(keys, flag)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(repeats):
        assert ctx.run_keypoints(keys, flag) == len(keys)
    p = ctx.profile()["descriptor"]
    ctx.profile_enable(False)
    return p["ms"] / max(1, p["launches"])      # (one descriptor launch per list run)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--check", action="store_true", help="also run the model checker of tests/rect_cases.py")
    args = ap.parse_args()

    img = fixtures.synthetic_blobs(W, H, 0)
    ctx = hessgpu_amd.HessContext(0)
    ctx.run(img[None])
    small, wide = rect_list(24.0, 24.0, 1), rect_list(200.0, 40.0, 2)
    lists = {
        "rect_24x24": (small, _abi.KEYS_RECTANGLES, rect_pixels(ctx, 24.0, 24.0)),
        "rect_200x40": (wide, _abi.KEYS_RECTANGLES, rect_pixels(ctx, 200.0, 40.0)),
        "oriented": (small, _abi.KEYS_ORIENTED, oriented_pixels(ctx, 24.0, math.fmod(2 * math.pi - 24.0, 2 * math.pi))),
    }
    out = {"tool": "rect_descriptors", "image": [W, H], "entries": N, "repeats": args.repeats, "lists": {}}
    for _ in range(2):        # the three lists taking turns, twice: the second round is reported beside the first
        for name, (keys, flag, pixels) in lists.items():
            ms = timed(ctx, keys, flag, args.warmup, args.repeats)
            e = out["lists"].setdefault(name, {"flag": flag, "gathered_pixels_per_entry": round(pixels), "ms_per_launch": []})
            e["ms_per_launch"].append(round(ms, 5))
    for e in out["lists"].values():
        e["ns_per_1000_pixels"] = round(min(e["ms_per_launch"]) * 1e6 / (N * e["gathered_pixels_per_entry"]) * 1e3, 2)
    ctx.close()
    if args.check:
        import rect_cases as rc

        g = hessgpu_amd.HessContext(0)
        worst = 0.0
        for case in rc.cases():
            for entry in ("run_keypoints", "set_keypoints"):
                worst = max(worst, rc.check_rectangles(g, case, entry)["worst"])
        g.close()
        out["worst_deviation_from_model"] = worst
        out["bound"] = rc.TOL_DESC
    print(json.dumps(out))


if __name__ == "__main__":
    main()
