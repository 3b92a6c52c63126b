"""Byte descriptors on the GPU (hess_set_descriptor_format(HESS_DESC_FORMAT_U8)): the descriptor kernels store dim bytes
per feature and every path behind them carries bytes.  The expected bytes are always oracle_quantize(float descriptors)
-- the matcher's rule, low byte of (int)((double)(512.0f * d) + 0.5) -- with the floats taken from the SAME context in
F32 mode (the rest of the suite holds those bit-identical to the oracle), which also walks the switch F32 -> U8 -> F32.
Every case asserts: the floats are finite, counts and keypoint records are equal between the formats, and the float
results after switching back are the first ones."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
from hessgpu_amd import _abi
from hessgpu_amd.session import HessError
from oracle_lib import OracleSession, oracle_match, oracle_quantize

pytestmark = pytest.mark.gpu


def _three_ways(g, run, first="f32"):
    """run() executes one batch on g and returns the number of images.  The batch in `first`, the other format, `first`
    again -> (float results, byte results) per image as (keys, desc), after the checks every case makes."""
    other = "u8" if first == "f32" else "f32"
    res = {}
    for tag, fmt in (("a", first), ("b", other), ("c", first)):
        g.set_descriptor_format(fmt)
        n = run()
        assert g.desc_format() == fmt
        res[tag] = [g.fetch(b) for b in range(n)]
    f, u = (res["a"], res["b"]) if first == "f32" else (res["b"], res["a"])
    dim = g.desc_dim()
    for b, ((fk, fd), (uk, ud)) in enumerate(zip(f, u)):
        assert fd.dtype == np.float32 and ud.dtype == np.uint8 and fd.shape == ud.shape == (len(fk), dim), b
        assert np.isfinite(fd).all(), b
        assert len(fk) == len(uk) and fk.tobytes() == uk.tobytes(), f"image {b}: keypoint records differ between the formats"
        assert np.array_equal(ud, oracle_quantize(fd)), f"image {b}: bytes differ from the quantised floats"
    for b, ((ak, ad), (ck, cd)) in enumerate(zip(res["a"], res["c"])):   # back in the first format: the first results
        assert ak.tobytes() == ck.tobytes() and ad.tobytes() == cd.tobytes(), f"image {b}: results changed after switching back"
    return f, u


# ---- 1: one image through run(): the in-kernel mirror, every descriptor kernel ----------------------------------------
@pytest.mark.parametrize("kw", [
    dict(),                                                    # descriptor_pixel_kernel / descriptor_pixel_u8_kernel
    dict(half_sift=1),                                         # 64 bytes per feature: neighbouring lanes share a dword
    dict(descriptor_order=_abi.DESC_ORDER_SEQUENTIAL),         # descriptor_kernel<*, true>
    dict(descriptor_order=_abi.DESC_ORDER_INTERLEAVED),        # descriptor_kernel<*, false>
    dict(detector=_abi.DETECTOR_DOG, max_orientation=2),       # the multi-angle decode
], ids=["default", "half", "sequential", "interleaved", "dog_two_angles"])
def test_one_image_through_run(gpu_ctx_factory, kw):
    img = fixtures.load_rgb("640-1.jpg")
    g = gpu_ctx_factory(**kw)
    f, u = _three_ways(g, lambda: len(g.run(img[None])))
    assert len(f[0][0]) > 100 and u[0][1].any()


# ---- 2: five images through submit_host + wait: the copier, two launches over unequal groups of images ----------------
@pytest.mark.parametrize("half", [0, 1], ids=["128d", "half"])
def test_batch_of_five_through_the_copier(gpu_ctx_factory, half):
    imgs = np.stack([fixtures.synthetic_blobs(324, 223, index=i) for i in range(5)])
    g = gpu_ctx_factory(half_sift=half)

    def run():
        g.submit_host(imgs)
        g.wait()
        return len(imgs)

    f, _ = _three_ways(g, run)
    counts = [len(k) for k, _ in f]
    assert min(counts) > 100 and len(set(counts)) > 1          # (images of different counts: the groups' offsets differ)


# ---- 3: one image delivered by the copier in quarters of its feature list ---------------------------------------------
def test_one_image_in_feature_quarters(gpu_ctx_factory, monkeypatch):
    img = fixtures.synthetic_blobs(324, 223, index=3)
    o = OracleSession(threads=8, keep_levels=False)
    want = o.run(img[None])[0]
    o.close()
    assert want > 100 and want % 4 != 0                        # the quarters' bounds are not multiples of anything
    monkeypatch.setenv("HESS_DELIVERY", "dma")
    g = gpu_ctx_factory()
    monkeypatch.delenv("HESS_DELIVERY")
    f, _ = _three_ways(g, lambda: len(g.run(img[None])))
    assert len(f[0][0]) == want


# ---- 4: a batch delivered by the copy on the context's stream ---------------------------------------------------------
def test_batch_under_blit_delivery(gpu_ctx_factory, monkeypatch):
    imgs = np.stack([fixtures.synthetic_blobs(324, 223, index=i) for i in (1, 2, 4)])
    monkeypatch.setenv("HESS_DELIVERY", "blit")
    g = gpu_ctx_factory()
    monkeypatch.delenv("HESS_DELIVERY")
    f, _ = _three_ways(g, lambda: len(g.run(imgs)))
    assert min(len(k) for k, _ in f) > 100


# ---- 5: keypoint lists: the bytes come back in input order -------------------------------------------------------------
@pytest.mark.parametrize("entry", ["set_keypoints", "run_keypoints"])
def test_keypoint_lists(gpu_ctx_factory, entry):
    img = fixtures.load_rgb("640-1.jpg")
    g = gpu_ctx_factory()
    g.run(img[None])
    keys, _ = g.fetch(0)
    pick = np.random.RandomState(5).permutation(len(keys))[:50]   # shuffled: list order is not level order
    assert len(set(keys["level"][pick])) > 2

    def run_list(sel):
        def run():
            if entry == "set_keypoints":
                g.set_keypoints(keys[sel], have_orientation=True)
                assert g.run(img[None]) == [len(sel)]
            else:
                assert g.run_keypoints(keys[sel], have_orientation=True) == len(sel)
            return 1
        return run

    f, u = _three_ways(g, run_list(pick))
    assert u[0][0].tobytes() == keys[pick].tobytes()            # the caller's keypoints, in the caller's order
    _, ur = _three_ways(g, run_list(pick[::-1]))
    assert np.array_equal(ur[0][1], u[0][1][::-1]) and u[0][1].any()   # reversed list -> reversed rows
    # a list run takes the format set NOW, whatever the image was run in; a detection run afterwards is unaffected
    g.set_descriptor_format("u8")
    g.run(img[None])
    ku, du = g.fetch(0)
    assert ku.tobytes() == keys.tobytes() and du.dtype == np.uint8
    g.set_descriptor_format("f32")
    if entry == "run_keypoints":
        assert g.run_keypoints(keys[pick], True) == 50
        assert g.fetch(0)[1].tobytes() == f[0][1].tobytes()


# ---- 6: a batch that overflows its feature storage and is run again ---------------------------------------------------
@pytest.mark.parametrize("mode", ["mirror", "dma"])
def test_overflow_rerun_keeps_the_format(gpu_ctx_factory, monkeypatch, mode):
    monkeypatch.setenv("HESS_INITIAL_CAP", "16")
    monkeypatch.setenv("HESS_DELIVERY", mode)
    g = gpu_ctx_factory(dev_switches=True, dog_threshold=0.0005, edge_threshold=50.0)
    monkeypatch.delenv("HESS_INITIAL_CAP")
    monkeypatch.delenv("HESS_DELIVERY")
    imgs = (np.random.RandomState(11).rand(3, 120, 200) * 255).astype(np.uint8)
    seen = []

    def run():
        n = len(g.run(imgs))
        seen.append(g.regrown())
        return n

    f, _ = _three_ways(g, run, first="u8")                       # the context's FIRST batch is the byte one: it regrows
    assert seen[0] > 0 and seen[-1] == seen[0]                  # ... and the later ones fit (grow-only)
    assert min(len(k) for k, _ in f) > 16 * 4


# ---- 7: refusals and bounds -------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx_factory):
    img = fixtures.load_rgb("640-1.jpg")
    g = gpu_ctx_factory()
    fn, h = g._f, g._h
    for bad in (2, -1, 255):
        assert fn["set_descriptor_format"](h, bad) == _abi.HESS_ERR_ARG
    assert g.desc_format() == "f32"
    # while a submitted batch is pending
    g.submit_host(img[None])
    assert fn["set_descriptor_format"](h, _abi.DESC_FORMAT_U8) == _abi.HESS_ERR_STATE
    assert fn["set_descriptor_format"](h, _abi.DESC_FORMAT_F32) == _abi.HESS_ERR_STATE
    g.wait()
    assert g.desc_format() == "f32" and g.fetch(0)[1].dtype == np.float32
    # unnormalised descriptors are unbounded: no bytes
    raw = gpu_ctx_factory(normalize=0)
    with pytest.raises(HessError) as e:
        raw.set_descriptor_format("u8")
    assert e.value.code == _abi.HESS_ERR_UNSUPPORTED and "normal" in str(e.value)
    raw.set_descriptor_format("f32")
    # shared result buffers carry floats: refused both ways round
    name = f"hess_u8_refusal_{os.getpid()}"
    sh = gpu_ctx_factory()
    sh.share_results(name)
    with pytest.raises(HessError) as e:
        sh.set_descriptor_format("u8")
    assert e.value.code == _abi.HESS_ERR_UNSUPPORTED and "shared" in str(e.value)
    by = gpu_ctx_factory()
    by.set_descriptor_format("u8")
    with pytest.raises(HessError) as e:
        by.share_results(name + "b")
    assert e.value.code == _abi.HESS_ERR_UNSUPPORTED
    assert by.desc_format() == "u8"                               # (no run yet: the format of the runs to come)


def test_fetch_in_the_wrong_format_writes_nothing_and_fetch_u8_writes_exactly_the_bytes(gpu_ctx_factory):
    img = fixtures.load_rgb("640-1.jpg")
    g = gpu_ctx_factory()
    fn, h = g._f, g._h
    g.set_descriptor_format("u8")
    n = g.run(img[None])[0]
    dim = g.desc_dim()
    assert n > 100 and dim == 128
    want_k, want_d = g.fetch(0)
    # hess_fetch after a U8 run
    keys = np.full(n * 24 + 64, 0xA5, np.uint8)
    desc = np.full(n * dim * 4 + 64, 0xA5, np.uint8)
    assert fn["fetch"](h, 0, keys.ctypes.data, desc.ctypes.data) == _abi.HESS_ERR_STATE
    assert (keys == 0xA5).all() and (desc == 0xA5).all()
    assert b"u8" in fn["last_error"](h)
    # hess_fetch_u8: count x dim bytes and not one more
    assert fn["fetch_u8"](h, 0, keys.ctypes.data, desc.ctypes.data) == 0
    assert keys[:n * 24].tobytes() == want_k.tobytes() and (keys[n * 24:] == 0xA5).all()
    assert desc[:n * dim].tobytes() == want_d.tobytes() and (desc[n * dim:] == 0xA5).all()
    # setting the format does not change what the results ARE
    g.set_descriptor_format("f32")
    assert g.desc_format() == "u8" and g.fetch(0)[1].tobytes() == want_d.tobytes()
    # hess_fetch_u8 after an F32 run
    g.run(img[None])
    keys[:] = 0xA5
    desc[:] = 0xA5
    assert fn["fetch_u8"](h, 0, keys.ctypes.data, desc.ctypes.data) == _abi.HESS_ERR_STATE
    assert (keys == 0xA5).all() and (desc == 0xA5).all()
    assert b"f32" in fn["last_error"](h)
    assert np.array_equal(oracle_quantize(g.fetch(0)[1]), want_d)


# ---- 8: the matcher's bank straight from byte results -----------------------------------------------------------------
def _oracle_pairs(bank, pairs):
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
        return list(ex.map(lambda p: oracle_match(bank[p[0]], bank[p[1]]), [tuple(p) for p in pairs]))


def test_matcher_bank_from_byte_results(gpu_ctx_factory):
    from hessgpu_amd.matcher import Matcher, all_pairs

    imgs = np.stack([fixtures.load_rgb(f"640-{i}.jpg") for i in range(1, 6)])
    g = gpu_ctx_factory()
    pairs = all_pairs(5)
    counts = g.run(imgs)
    floats = [g.fetch(i)[1] for i in range(5)]
    assert all(np.isfinite(d).all() for d in floats) and min(counts) > 100
    cut = max(counts) - 50                                       # below one image's count, above none: some sets are cut
    assert cut > 0
    got = {}
    for fmt in ("f32", "u8"):
        g.set_descriptor_format(fmt)
        assert g.run(imgs) == counts
        for max_sift in (8192, cut):
            m = Matcher(0, max_sift=max_sift)
            m.set_bank_from_session(g)
            bank = [m.bank(i) for i in range(5)]
            got[fmt, max_sift] = (bank, m.match_pairs(pairs))
            m.close()
    for max_sift in (8192, cut):
        (bf, mf), (bu, mu) = got["f32", max_sift], got["u8", max_sift]
        for i in range(5):
            assert np.array_equal(bu[i], bf[i]), (max_sift, i)
            assert np.array_equal(bu[i], oracle_quantize(floats[i][:max_sift])), (max_sift, i)
        ref = _oracle_pairs(bu, pairs)
        for k in range(len(pairs)):
            assert np.array_equal(mu[k], mf[k]) and np.array_equal(mu[k], ref[k]), (max_sift, pairs[k])
        assert sum(len(x) for x in mu) > 0
    assert any(len(b) == cut for b in got["u8", cut][0])
    # 64-d bytes are refused like 64-d floats
    half = gpu_ctx_factory(half_sift=1)
    half.set_descriptor_format("u8")
    half.run(imgs[:1])
    m = Matcher(0)
    with pytest.raises(ValueError):
        m.set_bank_from_session(half)
    # host memory is not device memory: an argument check, nothing is launched
    host = np.zeros((10, 128), np.uint8)
    with pytest.raises(HessError) as e:
        m.set_bank_device(host.ctypes.data, [10], dtype=np.uint8)
    assert e.value.code == _abi.HESS_ERR_ARG and "device memory" in str(e.value)
    m.close()
