"""GPU: the asynchronous submit/wait pair with two contexts, the packed device-resident results,
and the RCCL gather path (backend "nccl", world size 1 on the one-GPU box)."""
import os
import socket

import numpy as np
import pytest

import fixtures

pytestmark = pytest.mark.gpu


def _imgs(n):
    return np.stack([fixtures.synthetic_blobs(320, 240, i) for i in range(n)])


def test_submit_wait_two_contexts_match_synchronous_run(gpu_ctx_factory):
    import torch

    a, b, ref = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    i1, i2 = _imgs(3), _imgs(6)[3:]
    d1, d2 = torch.from_numpy(i1).cuda(), torch.from_numpy(i2).cuda()
    a.submit_device(d1.data_ptr(), 3, 240, 320)
    b.submit_device(d2.data_ptr(), 3, 240, 320)
    from hessgpu_amd.session import HessError
    with pytest.raises(HessError):  # one batch in flight per context
        a.submit_device(d1.data_ptr(), 3, 240, 320)
    a.wait()
    b.wait()
    for ctx, imgs in ((a, i1), (b, i2)):
        n = ref.run(imgs)
        assert [ctx.count(k) for k in range(3)] == n and sum(n) > 0
        for k in range(3):
            kk, dd = ctx.fetch(k)
            rk, rd = ref.fetch(k)
            assert kk.tobytes() == rk.tobytes() and dd.tobytes() == rd.tobytes()
    with pytest.raises(HessError):
        a.wait()  # nothing submitted


def test_every_hand_off_on_one_context_in_a_row(gpu_ctx_factory, monkeypatch):
    """One context takes every route from submit to wait, one after the other: the copier thread enqueues (pinned pixels), the
    caller enqueues and the copier delivers (device pixels, a pageable pair), the in-kernel mirror (a synchronous run), a
    keypoint list on the current image -- and the first route again, which would show descriptor parts left over by the
    others.  Reference: a context with HESS_DELIVERY=blit running the same images synchronously (no copier thread, no split
    descriptor launches)."""
    import torch

    from hessgpu_amd.session import HessError

    ab_switch = any(v in os.environ for v in ("HESS_DELIVERY", "HESS_DESC_PARTS", "HESS_MIRROR_MAX_MB", "HESS_MIRROR_MAX_BATCH"))
    g = gpu_ctx_factory()
    with monkeypatch.context() as m:
        m.setenv("HESS_DELIVERY", "blit")
        ref = gpu_ctx_factory()
    imgs = _imgs(6)
    four, four_dev, one, pair = imgs[:4], imgs[2:], imgs[5:], imgs[4:]
    pinned = torch.from_numpy(four).pin_memory()
    dev = torch.from_numpy(four_dev).cuda()
    g.profile_enable(True)

    def check(step, batch, launches, ref_counts):
        got = g.profile()["descriptor"]["launches"]
        g.profile_reset()
        assert [g.count(k) for k in range(batch)] == ref_counts and min(ref_counts) > 0, step
        for k in range(batch):
            (kk, dd), (rk, rd) = g.fetch(k), ref.fetch(k)
            assert kk.tobytes() == rk.tobytes() and dd.tobytes() == rd.tobytes(), (step, k)
        if not ab_switch:   # (the A/B switches choose otherwise)
            assert got == launches, (step, got)

    def pinned_four(step):   # upload first: the copier thread enqueues; two descriptor launches (policy::kSplitDescriptorsFrom)
        g.submit_host(ptr=pinned.data_ptr(), batch=4, height=240, width=320)
        g.wait()
        check(step, 4, 2, ref.run(four))

    g.profile_reset()
    pinned_four(1)
    g.submit_device(dev.data_ptr(), 4, 240, 320)       # the caller enqueues, the copier delivers
    with pytest.raises(HessError):                     # one batch in flight per context
        g.submit_device(dev.data_ptr(), 4, 240, 320)
    g.wait()
    check(2, 4, 2, ref.run(four_dev))
    g.run(one)                                         # the in-kernel mirror
    check(3, 1, 1, ref.run(one))
    keys = g.fetch(0)[0][:10].copy()
    assert len(keys) == 10
    g.run_keypoints(keys)                              # the current image's pyramid, a local run of one image
    check(4, 1, 1, [ref.run_keypoints(keys)])
    g.submit_host(pair)                                # pageable: staged, the caller enqueues, the copier delivers
    g.wait()
    check(5, 2, 1, ref.run(pair))
    pinned_four(6)
    g.profile_enable(False)


def test_device_results_are_packed_and_gather_over_nccl(gpu_ctx_factory):
    import torch
    import torch.distributed as dist

    from hessgpu_amd import dist as hdist

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        g = gpu_ctx_factory(truncate_method=3, feature_count_threshold=200)
        imgs = _imgs(4)
        counts = g.run(imgs)
        keys, desc = hdist.device_feature_tensors(g, counts, dev)
        assert keys.shape == (sum(counts), 24) and desc.shape == (sum(counts), 128)
        allc, gk, gd = hdist.gather_feature_lists(counts, keys, desc, dst=0)
        assert allc == [counts]
        hk = np.concatenate([np.frombuffer(g.fetch(b)[0].tobytes(), np.uint8).reshape(-1, 24) for b in range(4)])
        hd = np.concatenate([g.fetch(b)[1] for b in range(4)])
        assert np.array_equal(gk[0].cpu().numpy(), hk)
        assert np.array_equal(gd[0].cpu().numpy().view(np.uint32), hd.view(np.uint32))
        # same gather with the counts exchanged over the gloo side group (what bench.py does)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        hdist.enable_host_count_exchange()
        allc2, gk2, gd2 = hdist.gather_feature_lists(counts, keys, desc, dst=0)
        assert allc2 == [counts]
        assert np.array_equal(gk2[0].cpu().numpy(), hk)
        assert np.array_equal(gd2[0].cpu().numpy().view(np.uint32), hd.view(np.uint32))
    finally:
        hdist._count_group.clear()
        dist.destroy_process_group()


def test_one_context_per_host_thread(gpu_ctx_factory):
    """MultiThreadSIFT.cpp's usage: one instance per host thread, RunSIFT concurrently.  Contexts share
    nothing (own stream, buffers, parameters); results must equal the single-threaded ones."""
    import threading

    from oracle_lib import OracleSession

    names = fixtures.list640()[:4]
    imgs = [fixtures.load_rgb(n) for n in names]
    ref = []
    o = OracleSession(threads=8, keep_levels=False)
    for im in imgs:
        o.run(im[None])
        ref.append(tuple(a.tobytes() for a in o.fetch(0)))
    out, errs = {}, []

    def work(tid):
        try:
            g = gpu_ctx_factory()
            for rep in range(6):
                for k in range(len(imgs)):
                    i = (k + tid) % len(imgs)
                    g.run(imgs[i][None])
                    got = tuple(a.tobytes() for a in g.fetch(0))
                    if got != ref[i]:
                        errs.append((tid, rep, i))
            out[tid] = True
        except Exception as e:  # surfaces in the main thread's assert
            errs.append((tid, repr(e)))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and len(out) == 4, errs[:3]
