#!/usr/bin/env python3
"""Caller keypoint lists over a batch: one hess_set_keypoints_batch run against eight single-image runs, one JSON line.

Eight 1920x1080 synthetic images (tests/fixtures.py), 4096 oriented keys per image (seeded: positions uniform, scales
log-uniform in 1 .. 24).  Host pixels (pageable), host clock around work that ends with the results in host memory:
  loop            per image hess_set_keypoints + hess_run_host          (--mode loop: these calls exist on every commit)
  batch           one hess_set_keypoints_batch + hess_run_host of the eight images
  batch_2ctx      the same submitted on two contexts in turn (set + hess_submit_host on one while the other's batch runs,
                  hess_wait before the context is used again)
--mode both (the default) alternates the three in rounds inside one process; every round runs --repeats / --rounds
repetitions after --warmup, and the figure of a round is its mean ms per IMAGE.  Reported per mode: the rounds, their
median and their spread (min, max).  --check compares the batch results with the loop's, bit for bit."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import fixtures
import hessgpu_amd
from hessgpu_amd import _abi

W, H, B, N = 1920, 1080, 8, 4096


def key_lists():
    rng = np.random.RandomState(7)
    out = []
    for _ in range(B):
        k = np.zeros(N, dtype=_abi.KEYPOINT_DTYPE)
        k["x"] = rng.uniform(8.0, W - 8.0, N)
        k["y"] = rng.uniform(8.0, H - 8.0, N)
        k["s"] = np.exp(rng.uniform(0.0, math.log(24.0), N))
        k["o"] = rng.uniform(0.0, 2.0 * math.pi, N)
        out.append(k)
    return out


def loop_step(ctx, imgs, lists):
    for b in range(B):
        ctx.set_keypoints(lists[b], True)
        ctx.run(imgs[b][None])


def batch_step(ctx, imgs, lists):
    ctx.set_keypoints_batch(lists, True)
    ctx.run(imgs)


def timed(step, reps):
    """-> mean ms per image over `reps` steps of B images."""
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    return (time.perf_counter() - t0) * 1e3 / (reps * B)


def pipelined(ctxs, imgs, lists, reps):
    """`reps` batches over the contexts in turn -> mean ms per image, from the first submission to the last wait."""
    busy = [False] * len(ctxs)
    t0 = time.perf_counter()
    for r in range(reps):
        i = r % len(ctxs)
        if busy[i]:
            ctxs[i].wait()
        ctxs[i].set_keypoints_batch(lists, True)
        ctxs[i].submit_host(imgs)
        busy[i] = True
    for i, c in enumerate(ctxs):
        if busy[i]:
            c.wait()
    return (time.perf_counter() - t0) * 1e3 / (reps * B)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("loop", "batch", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check", action="store_true", help="compare the batch results with the loop's, bit for bit")
    args = ap.parse_args()

    imgs = np.stack([fixtures.synthetic_blobs(W, H, i) for i in range(B)])
    lists = key_lists()
    per_round = max(1, args.repeats // args.rounds)
    modes = {}
    ctx = hessgpu_amd.HessContext(0)
    if args.mode in ("loop", "both"):
        modes["loop"] = lambda: timed(lambda: loop_step(ctx, imgs, lists), per_round)
    if args.mode in ("batch", "both"):
        pair = [hessgpu_amd.HessContext(0) for _ in range(2)]
        modes["batch"] = lambda: timed(lambda: batch_step(ctx, imgs, lists), per_round)
        modes["batch_2ctx"] = lambda: pipelined(pair, imgs, lists, per_round)
    out = {"tool": "keypoint_batch", "image": [W, H], "images": B, "keys_per_image": N, "repeats_per_round": per_round,
           "ms_per_image": {name: [] for name in modes}}
    if args.check and args.mode == "both":
        want = []
        for b in range(B):
            ctx.set_keypoints(lists[b], True)
            ctx.run(imgs[b][None])
            want.append(ctx.fetch(0))
        batch_step(ctx, imgs, lists)
        out["batch_equals_loop"] = all(ctx.fetch(b)[0].tobytes() == want[b][0].tobytes() and
                                       ctx.fetch(b)[1].tobytes() == want[b][1].tobytes() for b in range(B))
    saved, per_round = per_round, args.warmup
    for run in modes.values():      # warm-up: every mode, its buffers and both contexts of the pair
        run()
    per_round = saved
    for _ in range(args.rounds):    # the modes take turns: what drifts over the call drifts for all of them
        for name, run in modes.items():
            out["ms_per_image"][name].append(round(run(), 5))
    out["summary"] = {name: {"median": round(float(np.median(v)), 5), "min": min(v), "max": max(v)}
                      for name, v in out["ms_per_image"].items()}
    if "loop" in modes and "batch" in modes:
        s = out["summary"]
        out["loop_over_batch"] = round(s["loop"]["median"] / s["batch"]["median"], 3)
        out["loop_over_batch_2ctx"] = round(s["loop"]["median"] / s["batch_2ctx"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
