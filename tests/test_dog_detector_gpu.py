"""The difference-of-Gaussians detector (hess_params.detector = HESS_DETECTOR_DOG, SiftGPU -dog) on the device against
the CPU oracle run with the same detector word (oracle/hess_oracle.c, detector = 1: the reference's #ifndef GPU_HESSIAN
lines), bit for bit: every Gaussian level 0..dog+2, every response plane 0..dog+2 (D_l = G_l - G_(l-1) from level 1),
the gradient planes 1..dog, the raw detection list, the keypoints and the descriptors -- and, through the pixels of the
reference's own feature file (doc/evaluation/box.siftgpu, written by a DoG build), the detection itself."""
import ctypes as C

import numpy as np
import pytest

import box_fixture as bf
import fixtures
import siftgpu_lib
from hessgpu_amd import _abi
from oracle_lib import OracleSession

pytestmark = pytest.mark.gpu

DOG = _abi.DETECTOR_DOG


def _bits_equal(a, r):
    return np.array_equal(a.view(np.uint32), r.view(np.uint32))


def _compare(g, o, imgs, what, stages=True):
    g.keep_levels(stages)   # the top Gaussian level (dog+2) is only readable on request (hess_debug_keep_levels)
    ng = g.run(imgs)
    no = o.run(imgs)
    assert g.geometry() == o.geometry(), what
    if stages:
        dog = o.params.dog_level_num
        for b in range(len(no)):
            for oc in range(len(o.geometry())):
                for l in range(dog + 3):
                    a, r = g.level(b, oc, l, _abi.DBG_GAUSS), o.level(b, oc, l, _abi.DBG_GAUSS)
                    assert _bits_equal(a, r), f"{what}: gauss img {b} oct {oc} lvl {l}: {np.sum(a != r)} px differ"
                    a, r = g.level(b, oc, l, _abi.DBG_DETH), o.level(b, oc, l, _abi.DBG_DETH)
                    assert _bits_equal(a, r), f"{what}: response img {b} oct {oc} lvl {l}: {np.sum(a != r)} px differ"
                for l in range(1, dog + 1):
                    a, r = g.level(b, oc, l, _abi.DBG_GOT), o.level(b, oc, l, _abi.DBG_GOT)
                    assert _bits_equal(a, r), f"{what}: grad/theta img {b} oct {oc} lvl {l}: {np.sum(a != r)} differ"
    for b in range(len(no)):
        gl, ol = g.rawlist(b), o.rawlist(b)
        assert len(gl) == len(ol), f"{what}: img {b} list length {len(gl)} != {len(ol)}"
        assert gl.tobytes() == ol.tobytes(), f"{what}: img {b} detection list differs"
    assert ng == no, f"{what}: feature counts {ng} != {no}"
    for b in range(len(no)):
        gk, gd = g.fetch(b)
        ok, od = o.fetch(b)
        assert gk.tobytes() == ok.tobytes(), f"{what} img {b}: keypoints differ"
        assert _bits_equal(gd, od), f"{what} img {b}: descriptors differ"
    return no


def _pair(gpu_ctx_factory, **kw):
    return gpu_ctx_factory(detector=DOG, **kw), OracleSession(threads=8, detector=1, **kw)


@pytest.mark.parametrize("dog", [1, 3, 5, 10])
@pytest.mark.parametrize("first_octave", [-1, 0, 1])
def test_every_stage_equals_the_oracle(gpu_ctx_factory, dog, first_octave):
    g, o = _pair(gpu_ctx_factory, dog_level_num=dog, first_octave=first_octave)
    n = _compare(g, o, fixtures.load_rgb("640-1.jpg")[None], f"dog {dog} fo {first_octave}")
    assert n[0] > 20
    o.close()


@pytest.mark.parametrize("name", ["640-2.jpg", "800-1.jpg", "sunflowers.png", "1600.jpg"])
def test_reference_data_images(gpu_ctx_factory, name):
    g, o = _pair(gpu_ctx_factory)
    img = fixtures.load_rgb(name)
    assert _compare(g, o, img[None], name, stages=name != "1600.jpg")[0] > 100
    o.close()


def test_synthetic_blobs_u8_luminance(gpu_ctx_factory):
    # u8 luminance with the first octave at full size: levels 0 and 1 of octave 0 from one launch (FIRST tiles)
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, fixtures.synthetic_blobs(960, 544, 3)[None], "blobs u8")
    o.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_first_tile_level_0_feeds_d1_without_keep_levels(gpu_ctx_factory, batch):
    # the launch that makes levels 0 and 1 of octave 0 from u8 pixels keeps level 0 in LDS in the Hessian mode; D_1 needs it
    imgs = np.stack([fixtures.synthetic_blobs(800, 600, 20 + i) for i in range(batch)])
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, imgs, f"first tile, batch {batch}", stages=False)
    for b in range(batch):
        assert _bits_equal(g.level(b, 0, 1, _abi.DBG_DETH), o.level(b, 0, 1, _abi.DBG_DETH))
    o.close()


@pytest.mark.parametrize("kw", [dict(subpixel=0), dict(max_orientation=1), dict(max_orientation=4),
                                dict(fixed_orientation=1), dict(half_sift=1), dict(half_sift=1, max_orientation=4),
                                dict(descriptor_order=_abi.DESC_ORDER_INTERLEAVED),
                                dict(descriptor_order=_abi.DESC_ORDER_SEQUENTIAL),
                                dict(descriptor_order=_abi.DESC_ORDER_PIXEL, dynamic_indexing=1),
                                dict(lowe_origin=1, first_octave=-1)])
def test_options(gpu_ctx_factory, kw):
    g, o = _pair(gpu_ctx_factory, **kw)
    _compare(g, o, fixtures.load_rgb("640-3.jpg")[None], f"{kw}", stages=False)
    o.close()


def test_two_peak_orientations_reach_the_features(gpu_ctx_factory):
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, fixtures.load_rgb("640-4.jpg")[None], "two peaks", stages=False)
    k, _ = g.fetch(0)
    raw = g.rawlist(0)
    assert len(raw) < len(k) <= 2 * len(raw)   # some keypoints carry a second orientation, none a third


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("rgb", [False, True])
def test_input_formats(gpu_ctx_factory, dtype, rgb):
    img = fixtures.load_rgb("640-5.jpg")
    if not rgb:
        img = np.ascontiguousarray(img[..., 0])
    if dtype == np.uint16:
        img = img.astype(np.uint16) * 257
    elif dtype == np.float32:
        img = img.astype(np.float32) / 255.0
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, img[None], f"{np.dtype(dtype).name} rgb={rgb}", stages=dtype == np.uint8)
    o.close()


@pytest.mark.parametrize("batch", [1, 2, 3, 8])
def test_batches(gpu_ctx_factory, batch):
    imgs = np.stack([fixtures.synthetic_blobs(640, 480, 40 + i) for i in range(batch)])
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, imgs, f"batch {batch}", stages=batch <= 3)
    o.close()


def test_pipelined_batches_of_eight(gpu_ctx_factory):
    # hess_submit_host (the throughput path: copier delivery, descriptors in two launches)
    imgs = np.stack([fixtures.synthetic_blobs(1920, 1080, i) for i in range(8)])
    g, o = _pair(gpu_ctx_factory, truncate_method=_abi.TRUNC_TOPK, feature_count_threshold=4096)
    g.submit_host(imgs)
    g.wait()
    no = o.run(imgs)
    assert [g.count(b) for b in range(8)] == no
    for b in range(8):
        gk, gd = g.fetch(b)
        ok, od = o.fetch(b)
        assert gk.tobytes() == ok.tobytes() and _bits_equal(gd, od), f"img {b}"
    o.close()


@pytest.mark.parametrize("size", [(333, 251), (517, 97), (1001, 733)])
def test_ragged_sizes(gpu_ctx_factory, size):
    w, h = size
    img = np.ascontiguousarray(fixtures.load_rgb("800-2.jpg")[:h, :w])
    g, o = _pair(gpu_ctx_factory)
    _compare(g, o, img[None], f"{w}x{h}")
    o.close()


@pytest.mark.parametrize("method,thr", [(_abi.TRUNC_TOPK, 300), (_abi.TRUNC_HIGHEST_0, 400),
                                        (_abi.TRUNC_HIGHEST_1, 400), (_abi.TRUNC_LOWEST, 400)])
def test_feature_limits(gpu_ctx_factory, method, thr):
    imgs = np.stack([fixtures.synthetic_blobs(640, 480, 60 + i) for i in range(2)])
    g, o = _pair(gpu_ctx_factory, truncate_method=method, feature_count_threshold=thr)
    _compare(g, o, imgs, f"limit {method} {thr}", stages=False)
    o.close()


@pytest.mark.parametrize("have_orientation", [1, 0])
@pytest.mark.parametrize("kw", [dict(), dict(max_orientation=1), dict(dog_level_num=5, first_octave=-1)])
def test_keypoint_lists(gpu_ctx_factory, kw, have_orientation):
    img = fixtures.load_rgb("640-1.jpg")
    g, o = _pair(gpu_ctx_factory, **kw)
    g.run(img[None]); o.run(img[None])
    keys, _ = o.fetch(0)
    keys = keys.copy()
    keys["s"][::7] *= 3.1      # other levels (the level mapping follows the DoG level sigmas) and the catch-alls
    keys["s"][3::11] *= 0.2
    keys["s"][5] = 400.0
    assert g.run_keypoints(keys, have_orientation) == o.run_keypoints(keys, have_orientation) == len(keys)
    gk, gd = g.fetch(0)
    ok, od = o.fetch(0)
    assert gk.tobytes() == ok.tobytes() and _bits_equal(gd, od)
    other = fixtures.load_rgb("640-2.jpg")
    for s in (g, o):
        s.set_keypoints(keys[:200], have_orientation=bool(have_orientation))
    assert g.run(other[None]) == o.run(other[None]) == [200]
    gk, gd = g.fetch(0)
    ok, od = o.fetch(0)
    assert gk.tobytes() == ok.tobytes() and _bits_equal(gd, od)
    o.close()


def test_hessian_and_dog_contexts_alternate(gpu_ctx_factory):
    img = fixtures.load_rgb("640-2.jpg")[None]
    gh, gd = gpu_ctx_factory(), gpu_ctx_factory(detector=DOG)
    oh, od = OracleSession(threads=8), OracleSession(threads=8, detector=1)
    for _ in range(2):
        _compare(gh, oh, img, "hessian", stages=False)
        _compare(gd, od, img, "dog", stages=False)
    assert gh.rawlist(0).tobytes() != gd.rawlist(0).tobytes()
    oh.close(); od.close()


@pytest.mark.parametrize("word,value", [(0, 2), (0, 3), (0, -1), (1, 1), (3, 7), (5, -1)])
def test_create_refuses_other_detectors_and_reserved_words(word, value):
    import hessgpu_amd

    hessgpu_amd.load_library()
    create, destroy = hessgpu_amd.functions()["create"], hessgpu_amd.functions()["destroy"]
    p = hessgpu_amd.default_params()
    p.reserved[word] = value
    assert not create(0, C.byref(p))
    for det in (0, 1):   # the values it accepts, for contrast
        q = hessgpu_amd.default_params(detector=det)
        h = create(0, C.byref(q))
        assert h
        destroy(h)
    old = hessgpu_amd.default_params(detector=1)
    old.abi_version = 4   # a version-4 struct has no detector word
    assert not create(0, C.byref(old))


def test_siftgpu_dog_switch_equals_the_context(gpu_ctx_factory):
    img = fixtures.load_rgb("640-1.jpg")
    s = siftgpu_lib.SiftGPU(["-dog"])
    assert s.create_context() and s.params().detector == DOG
    assert s.run(img, siftgpu_lib.GL_RGB, siftgpu_lib.GL_UNSIGNED_BYTE)
    sk, sd = s.features()
    s.close()
    g = gpu_ctx_factory(detector=DOG)
    g.run(img[None])
    gk, gd = g.fetch(0)
    assert len(gk) > 100 and sk.tobytes() == gk.tobytes() and _bits_equal(sd, gd)


def test_reference_file_pins_the_detection(gpu_ctx_factory):
    """box.pgm with the parameters of the reference's feature file: the device's raw detection list is the one of the
    oracle in the file's own build (detector 2: only the orientation stage's level sigma differs), and the file's
    keypoint locations are found again."""
    img, vals = bf.load()
    kw = dict(bf.DOG_PARAMS, detector=DOG)
    g = gpu_ctx_factory(**kw)
    o2 = OracleSession(threads=8, **bf.DOG_PARAMS)
    g.run(img[None]); o2.run(img[None])
    raw = g.rawlist(0)
    assert len(raw) > 500 and raw.tobytes() == o2.rawlist(0).tobytes()
    k, _ = g.fetch(0)
    locs = np.unique(vals[:, :2], axis=0)                       # (y, x) per file row
    assert len(locs) == 541
    d = np.hypot(k["x"][None, :].astype(np.float64) - locs[:, 1:2], k["y"][None, :].astype(np.float64) - locs[:, 0:1])
    assert (d.min(axis=1) <= 0.03).sum() >= 534
    o2.close()
