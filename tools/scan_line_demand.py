#!/usr/bin/env python3
"""Which 128-byte lines (32 floats) of the outer det-H levels 0 and dog+1 the extrema scan needs, from the CPU oracle's
planes (the scan row).  The outer levels are only ever the P / N neighbours of pixels of levels 1 and
dog, and only of pixels that first pass the tests inside the streamed levels:

  in-level   beyond the first threshold and >= / <= the 9 values of its own 3x3 (key_eval's first two tests, as a
             superset: the kernel's filter form);
  queued     the same over the 9 + 9 values of its own and the inner adjacent level (what extrema_stream_kernel queues
             for key_eval, which then reads the 3x3 of the outer level from memory).

For each, the fraction of the outer levels' lines that the 3x3 (rows y-1..y+1, columns x-1..x+1) of some such pixel
touches, over all octaves of every image (lines counted from the start of each plane row; every plane row is a multiple
of 16 bytes, so this slightly undercounts lines that a row shares with the next).  Synthetic blobs by default:

  python tools/scan_line_demand.py [--images N] [--dog 3] [--photos] [--size 1920x1080]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fixtures  # noqa: E402
from hessgpu_amd import _abi  # noqa: E402
from oracle_lib import OracleSession  # noqa: E402

PHOTOS = ["640-1.jpg", "640-2.jpg", "640-3.jpg", "640-4.jpg", "640-5.jpg", "800-1.jpg", "800-2.jpg", "800-3.jpg",
          "800-4.jpg", "1600.jpg", "sunflowers.png"]


def _box3(a, op):
    """3x3 max / min with the plane's border replicated (border pixels are never tested)."""
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    out = p[0:h, 0:w]
    for dy in range(3):
        for dx in range(3):
            out = op(out, p[dy:dy + h, dx:dx + w])
    return out


def _dilate(m):
    p = np.pad(m, 1)
    h, w = m.shape
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def _lines(need):
    """Distinct 32-float lines of a plane (row-major, rows of width w) that the pixels in `need` lie on."""
    h, w = need.shape
    ys, xs = np.nonzero(need)
    return np.unique((ys.astype(np.int64) * w + xs) // 32).size, -(-h * w // 32)


def image_demand(o, b, thr0):
    dog = o.params.dog_level_num
    tot = {"in-level": [0, 0], "queued": [0, 0], "lines": [0, 0], "survivors": [0, 0, 0]}
    for oc, (w, h) in enumerate(o.geometry()):
        D = [o.level(b, oc, l, _abi.DBG_DETH) for l in range(dog + 2)]
        mx = [_box3(d, np.maximum) for d in D]
        mn = [_box3(d, np.minimum) for d in D]
        interior = np.zeros((h, w), bool)
        interior[1:-1, 1:-1] = True
        for k, (l, outer, inner) in enumerate(((1, 0, 2), (dog, dog + 1, dog - 1))):
            r = D[l]
            base = interior & (np.abs(r) > thr0)
            inl = base & ((r >= mx[l]) | (r <= mn[l]))
            if 1 <= inner <= dog:
                q = base & ((r >= np.maximum(mx[l], mx[inner])) | (r <= np.minimum(mn[l], mn[inner])))
            else:  # dog 1: level 1 is both edge levels, nothing else is streamed
                q = inl
            n_in, n_all = _lines(_dilate(inl))
            n_q, _ = _lines(_dilate(q))
            tot["in-level"][k] += n_in
            tot["queued"][k] += n_q
            tot["lines"][k] += n_all
            tot["survivors"][k] += int(inl.sum())
        tot["survivors"][2] += h * w
    return tot


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=4, help="synthetic blobs images 0..N-1")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--dog", type=int, default=3)
    ap.add_argument("--detector", type=int, default=0, help="0 determinant of Hessian, 1 difference of Gaussians")
    ap.add_argument("--photos", action="store_true", help="the reference's data/ photographs instead of synthetic blobs")
    args = ap.parse_args()
    o = OracleSession(threads=16, keep_levels=True, dog_level_num=args.dog, detector=args.detector,
                      truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=4096)
    thr0 = (0.8 if o.params.subpixel else 1.0) * o.params.dog_threshold
    if args.photos:
        inputs = [(n, fixtures.load_rgb(n)) for n in PHOTOS]
    else:
        w, h = (int(v) for v in args.size.split("x"))
        inputs = [(f"blobs {i}", fixtures.synthetic_blobs(w, h, i)) for i in range(args.images)]
    names = ("level 0", f"level {args.dog + 1}")
    agg = None
    print(f"dog {args.dog}, thr0 {thr0:.6g}; fraction of the outer levels' 128-B lines a tested pixel's 3x3 touches")
    for name, img in inputs:
        o.run(img[None])
        t = image_demand(o, 0, thr0)
        agg = t if agg is None else {k: [a + b for a, b in zip(agg[k], t[k])] for k in t}
        print(f"{name:>14}: " + ", ".join(
            f"{names[k]} in-level {t['in-level'][k] / t['lines'][k]:.3f} queued {t['queued'][k] / t['lines'][k]:.3f}"
            for k in range(2)) + f"  (in-level survivors {t['survivors'][0]} / {t['survivors'][1]} of {t['survivors'][2]} px)")
    print(f"{'all':>14}: " + ", ".join(
        f"{names[k]} in-level {agg['in-level'][k] / agg['lines'][k]:.3f} queued {agg['queued'][k] / agg['lines'][k]:.3f}"
        for k in range(2)))
    o.close()


if __name__ == "__main__":
    main()
