#!/usr/bin/env python3
"""Throughput of the two detectors on bench.py's workload (BASELINE.json configs[1]: batches of eight 1920x1080 synthetic
images, default octaves / levels, top-K = 4096): the pipelined hess_submit_device loop over six contexts, device-resident
pixels, results delivered to host memory -- once with the determinant of the Hessian (the default) and once with the
difference of Gaussians (hess_params.detector = HESS_DETECTOR_DOG).  Prints one JSON line: Gpixel/s, ms per batch and
features per image per mode.  bench.py's headline is the Hessian mode's figure measured its own way; this tool only
puts the two modes side by side under one loop."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fixtures
import hessgpu_amd
from hessgpu_amd import _abi

W, H, B, TOPK = 1920, 1080, 8, 4096


def measure(d_imgs, detector, nctx, steps, warmup):
    ctxs = [hessgpu_amd.HessContext(0, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=TOPK, detector=detector)
            for _ in range(nctx)]
    for c in ctxs:
        c.reserve(W, H, B)
        c.run_device(d_imgs.data_ptr(), B, H, W)

    def run(n):
        inflight = []
        for i in range(n):
            c = ctxs[i % nctx]
            if len(inflight) == nctx:
                inflight.pop(0).wait()
            c.submit_device(d_imgs.data_ptr(), B, H, W)
            inflight.append(c)
        while inflight:
            inflight.pop(0).wait()

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    feats = [ctxs[(steps - 1) % nctx].count(b) for b in range(B)]
    for c in ctxs:
        c.close()
    return {"gpix_per_s": round(B * W * H / dt / 1e9, 2), "ms_per_batch": round(dt * 1e3, 3),
            "features_per_image": int(np.mean(feats))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--contexts", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3, help="alternating Hessian / DoG measurements; the best of each is kept")
    args = ap.parse_args()
    imgs = np.stack([fixtures.synthetic_blobs(W, H, i) for i in range(B)])
    d_imgs = torch.from_numpy(imgs).to("cuda:0")
    best = {}
    for _ in range(args.repeats):
        for name, det in (("hessian", _abi.DETECTOR_HESSIAN), ("dog", _abi.DETECTOR_DOG)):
            r = measure(d_imgs, det, args.contexts, args.steps, args.warmup)
            if name not in best or r["gpix_per_s"] > best[name]["gpix_per_s"]:
                best[name] = r
    print(json.dumps({"workload": f"{B} x {W}x{H} synthetic blobs, top-K={TOPK}, {args.contexts} contexts pipelined, "
                                  f"device-resident input", "steps": args.steps, **best}))


if __name__ == "__main__":
    main()
