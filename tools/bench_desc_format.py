#!/usr/bin/env python3
"""Float against byte descriptors (hess_set_descriptor_format) under one loop, formats alternated, one JSON line.

Legs (--legs, default all):
  a  bench.py's workload: batches of eight 1920x1080 synthetic images, top-K 4096, six contexts, hess_submit_device
  b  the same from pinned host pixels (hess_submit_host)
  c  BASELINE.json configs[4]: one 4096x4096 image, -maxd 4096 -topk 65536 -half, submitted, one and five contexts
  d  one 1080p image through hess_run_device: the descriptor kernel's own stores into pinned host memory
  e  Matcher.set_bank_from_session for 16 x 4096 descriptors (two batches' worth in one context's batch of 16)
Every leg is measured --repeats times per format, the formats taking turns; per leg and format the JSON holds the list of
figures (ms per batch / image / call) and their range.  `--formats f32` touches nothing a library without the byte format
lacks, so the same file measures an older build (run it from that build's tree)."""
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
S4 = 4096


def blobs(cache, w, h, index):
    """fixtures.synthetic_blobs, kept as .npy under --image-cache if given (the generator is deterministic and slow)."""
    path = os.path.join(cache, f"blobs_{w}x{h}_{index}.npy") if cache else None
    if path and os.path.exists(path):
        return np.load(path)
    img = fixtures.synthetic_blobs(w, h, index)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.save(path, img)
    return img


def context(fmt, **kw):
    c = hessgpu_amd.HessContext(0, **kw)
    if fmt != "f32":           # (an f32 measurement calls nothing new)
        c.set_descriptor_format(fmt)
    return c


def pipelined(ctxs, submit, steps, warmup):
    """ms per step of the submit / wait loop over the contexts (bench.py's loop)."""
    n = len(ctxs)

    def run(k):
        inflight = []
        for i in range(k):
            c = ctxs[i % n]
            if len(inflight) == n:
                inflight.pop(0).wait()
            submit(c)
            inflight.append(c)
        while inflight:
            inflight.pop(0).wait()

    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    return (time.perf_counter() - t0) / steps * 1e3


def leg_batches(fmt, d_imgs, pinned, args, host):
    ctxs = [context(fmt, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=TOPK) for _ in range(args.contexts)]
    for c in ctxs:
        c.reserve(W, H, B)
        c.run_device(d_imgs.data_ptr(), B, H, W)
    if host:
        ms = pipelined(ctxs, lambda c: c.submit_host(ptr=pinned.data_ptr(), batch=B, height=H, width=W), args.steps, args.warmup)
    else:
        ms = pipelined(ctxs, lambda c: c.submit_device(d_imgs.data_ptr(), B, H, W), args.steps, args.warmup)
    for c in ctxs:
        c.close()
    return {"ms_per_batch": ms}


def leg_configs4(fmt, d_big, args):
    ctxs = [context(fmt, tex_max_dim=4096, half_sift=1, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=65536)
            for _ in range(5)]
    for c in ctxs:
        c.reserve(S4, S4, 1)
        c.run_device(d_big.data_ptr(), 1, S4, S4)
    steps = max(10, args.steps // 2)
    sub = lambda c: c.submit_device(d_big.data_ptr(), 1, S4, S4)
    one = pipelined(ctxs[:1], sub, steps, 5)
    five = pipelined(ctxs, sub, steps, 10)
    for c in ctxs:
        c.close()
    return {"ms_per_image_one_context": one, "ms_per_image_five_contexts": five}


def leg_single(fmt, d_imgs, args):
    c = context(fmt, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=TOPK)
    c.reserve(W, H, 1)
    for _ in range(args.warmup):
        c.run_device(d_imgs.data_ptr(), 1, H, W)
    reps = args.steps * 4
    t0 = time.perf_counter()
    for _ in range(reps):
        c.run_device(d_imgs.data_ptr(), 1, H, W)
    ms = (time.perf_counter() - t0) / reps * 1e3
    c.close()
    return {"ms_per_image": ms}


def leg_bank(fmt, d16, args):
    from hessgpu_amd.matcher import Matcher

    c = context(fmt, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=TOPK, max_orientation=1)
    c.run_device(d16.data_ptr(), 16, H, W)
    m = Matcher(0, max_sift=TOPK)
    for _ in range(3):
        m.set_bank_from_session(c)
    reps = max(10, args.steps)
    t0 = time.perf_counter()
    for _ in range(reps):
        m.set_bank_from_session(c)     # (returns when the bank is built)
    ms = (time.perf_counter() - t0) / reps * 1e3
    n = sum(c.count(i) for i in range(16))
    m.close()
    c.close()
    return {"ms_per_call": ms, "descriptors": n}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--contexts", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3, help="measurements per leg and format, the formats taking turns")
    ap.add_argument("--formats", default="f32,u8")
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--image-cache", default=None, help="directory for the generated images (.npy)")
    args = ap.parse_args()
    formats = [f for f in args.formats.split(",") if f]
    legs = [x for x in args.legs.split(",") if x]
    if not set(formats) <= {"f32", "u8"} or not set(legs) <= set("abcde"):
        ap.error("formats are f32, u8; legs are a .. e")

    imgs = np.stack([blobs(args.image_cache, W, H, i) for i in range(B)])
    d_imgs = torch.from_numpy(imgs).to("cuda:0")
    runs = {}
    if "a" in legs:
        runs["a_submit_device_8x1080p"] = lambda f: leg_batches(f, d_imgs, None, args, False)
    if "b" in legs:
        pinned = torch.from_numpy(imgs).pin_memory()
        runs["b_submit_host_pinned_8x1080p"] = lambda f: leg_batches(f, d_imgs, pinned, args, True)
    if "c" in legs:
        d_big = torch.from_numpy(blobs(args.image_cache, S4, S4, 0)[None]).to("cuda:0")
        runs["c_configs4_4096sq_half"] = lambda f: leg_configs4(f, d_big, args)
    if "d" in legs:
        runs["d_run_device_one_1080p"] = lambda f: leg_single(f, d_imgs, args)
    if "e" in legs:
        d16 = torch.cat([d_imgs, d_imgs.flip(1)]).contiguous()
        runs["e_bank_from_session_16_sets"] = lambda f: leg_bank(f, d16, args)

    out = {}
    for name, fn in runs.items():
        per = {f: {} for f in formats}
        for _ in range(args.repeats):
            for f in formats:          # alternated: f32, u8, f32, u8, ...
                for k, v in fn(f).items():
                    per[f].setdefault(k, []).append(v)
        out[name] = {}
        for f in formats:
            out[name][f] = {}
            for k, vals in per[f].items():
                if k == "descriptors":
                    out[name][f][k] = vals[0]
                else:
                    out[name][f][k] = {"runs": [round(v, 4) for v in vals], "range": [round(min(vals), 4), round(max(vals), 4)]}
    print(json.dumps({"tool": "bench_desc_format", "formats": formats, "steps": args.steps, "contexts": args.contexts,
                      "repeats": args.repeats, "legs": out}))


if __name__ == "__main__":
    main()
