"""Keypoint lists for whole batches: hess_set_keypoints_batch / hess_run_keypoints_batch / hess_key_list_order against the
CPU oracle's single-image runs (bit-exact), cases of tests/keybatch_cases.py.

The expected result of image b is the oracle's `run(img_b[None]); run_keypoints(keys_b, flag)`; for rectangles, which the
oracle does not restate, the product's own single-image run (tests/test_rect_gpu.py checks that one against its model).
Keys are compared as bytes, descriptors by bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixtures
import keybatch_cases as kc
from hessgpu_amd import _abi
from hessgpu_amd.session import HessError
from oracle_lib import OracleSession, oracle_quantize

pytestmark = pytest.mark.gpu

CONFIGS = {"default": dict(), "half": dict(half_sift=1), "m1": dict(max_orientation=1), "u8": dict()}
RECT = _abi.KEYS_RECTANGLES


@functools.lru_cache(maxsize=None)
def _oracle(config):
    return OracleSession(threads=8, **CONFIGS[config])


@functools.lru_cache(maxsize=None)
def _expected(case, config, flag):
    """-> per image (keys, float descriptors) of the oracle's single-image runs; None for an image without keys."""
    o = _oracle("default" if config == "u8" else config)
    out = []
    for b, keys in enumerate(kc.CASES[case]()):
        if not len(keys):
            out.append(None)
            continue
        o.run(kc.image(b)[None])
        assert o.run_keypoints(keys, flag) == len(keys)
        out.append(o.fetch(0))
    return out


def _context(gpu_ctx_factory, config):
    g = gpu_ctx_factory(**CONFIGS[config])
    if config == "u8":
        g.set_descriptor_format("u8")
    return g


def _check_image(g, b, keys, want, what):
    assert g.count(b) == len(keys), what
    gk, gd = g.fetch(b)
    if want is None:
        assert len(gk) == 0 and len(gd) == 0, what
        return
    wk, wd = want
    assert gk.tobytes() == wk.tobytes(), f"{what}: keypoints differ"
    if gd.dtype == np.uint8 and wd.dtype != np.uint8:
        wd = oracle_quantize(wd)
    assert gd.shape == wd.shape and gd.tobytes() == wd.tobytes(), f"{what}: descriptors differ"


def _single_image_runs(gpu_ctx_factory, config, lists, flag):
    """The product's own single-image results (rectangles)."""
    g = _context(gpu_ctx_factory, config)
    out = []
    for b, keys in enumerate(lists):
        if not len(keys):
            out.append(None)
            continue
        g.set_keypoints(keys, flag)
        assert g.run(kc.image(b)[None]) == [len(keys)]
        out.append(g.fetch(0))
    return out


@pytest.mark.parametrize("flag", [0, 1, RECT])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_lists_of_a_batch(gpu_ctx_factory, config, flag):
    case = "D" if flag == RECT else "A"
    lists = kc.CASES[case]()
    want = _single_image_runs(gpu_ctx_factory, config, lists, flag) if flag == RECT else _expected(case, config, flag)
    g = _context(gpu_ctx_factory, config)
    g.set_keypoints_batch(lists, flag)
    assert g.run(kc.images(len(lists))) == [len(k) for k in lists]
    assert len(g.geometry()) == kc.octaves()
    for b, keys in enumerate(lists):
        _check_image(g, b, keys, want[b], f"case {case} {config} flag {flag} image {b}")
    if flag != 0:  # the caller's keys come back as given
        assert all(g.fetch(b)[0].tobytes() == keys.tobytes() for b, keys in enumerate(lists))
    # the lists are consumed: the next plain run detects again
    o = _oracle("default" if config == "u8" else config)
    assert g.run(kc.images(2)) == o.run(kc.images(2))


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("case", ["B", "C"])
def test_seams(gpu_ctx_factory, case, flag):
    lists = kc.CASES[case]()
    want = _expected(case, "default", flag)
    g = _context(gpu_ctx_factory, "default")
    g.set_keypoints_batch(lists, flag)
    assert g.run(kc.images(len(lists))) == [len(k) for k in lists]
    for b, keys in enumerate(lists):
        _check_image(g, b, keys, want[b], f"case {case} flag {flag} image {b}")


@pytest.mark.parametrize("case,flag", [("A", 1), ("A", 0), ("B", 1), ("D", RECT), ("C", 1)])
def test_key_list_order(gpu_ctx_factory, case, flag):
    lists = kc.CASES[case]()
    g = _context(gpu_ctx_factory, "default")
    g.set_keypoints_batch(lists, flag)
    g.run(kc.images(len(lists)))
    total = 0
    for b, keys in enumerate(lists):
        order = g.key_list_order(b)
        total += len(order)
        if case == "C":  # a seam key may be listed twice or nowhere: any valid index sequence
            assert len(order) <= 2 * len(keys) and np.all((order >= 0) & (order < len(keys)))
        else:
            assert np.array_equal(order, kc.list_order(keys, flag)), f"case {case} image {b}"
        # the level of every list entry rises along the list, and within a level the input index does
        raw = g.rawlist(b)
        assert len(raw) == len(order)
        lv = raw["level_index"].astype(np.int64)
        assert np.all(np.diff(lv * (len(keys) + 1) + order) > 0)
        if case != "C":
            assert np.all(kc.membership(keys, flag)[lv, order])
    assert g.device_results()[2] == total
    with pytest.raises(HessError):
        g.key_list_order(len(lists))
    g.run(kc.images(1))
    with pytest.raises(HessError) as e:
        g.key_list_order(0)  # a plain run has no list
    assert e.value.code == _abi.HESS_ERR_STATE


@pytest.mark.parametrize("flag", [1, 0])
def test_run_keypoints_batch_on_current_batch(gpu_ctx_factory, flag):
    imgs = kc.images(3)
    g, o = _context(gpu_ctx_factory, "default"), _oracle("default")
    assert g.run(imgs) == o.run(imgs)
    lists = []
    for b in range(3):
        keys = o.fetch(b)[0].copy()
        # perturb scales so that some keys change level and the first/last level catch-alls are hit
        keys["s"][::7] *= 3.1
        keys["s"][3::11] *= 0.2
        keys["s"][5] = 400.0
        lists.append(keys)
    assert g.run_keypoints_batch(lists, flag) == [len(k) for k in lists]
    for b, keys in enumerate(lists):
        o.run(imgs[b][None])
        assert o.run_keypoints(keys, flag) == len(keys)
        _check_image(g, b, keys, o.fetch(0), f"run_keypoints_batch flag {flag} image {b}")
    # the lists are consumed: the next plain run detects again
    assert g.run(imgs) == o.run(imgs)
    for b in range(3):
        gk, gd = g.fetch(b)
        ok, od = o.fetch(b)
        assert gk.tobytes() == ok.tobytes() and np.array_equal(gd.view(np.uint32), od.view(np.uint32))


def test_two_contexts_alternate(gpu_ctx_factory):
    """set_keypoints_batch + submit_host / wait on two contexts in turn, two steps each: the synchronous results."""
    lists, imgs = kc.case_a(), kc.images(4)
    sets = [lists, lists[::-1]]
    sync = _context(gpu_ctx_factory, "default")
    want = []
    for ls in sets:
        sync.set_keypoints_batch(ls, 0)
        sync.run(imgs)
        want.append([sync.fetch(b) for b in range(4)])
    ctx = [_context(gpu_ctx_factory, "default") for _ in range(2)]
    for step in range(2):
        for i, g in enumerate(ctx):
            g.set_keypoints_batch(sets[(step + i) % 2], 0)
            g.submit_host(imgs)
        for i, g in enumerate(ctx):
            g.wait()
            ls = sets[(step + i) % 2]
            for b in range(4):
                _check_image(g, b, ls[b], want[(step + i) % 2][b] if len(ls[b]) else None, f"step {step} context {i} image {b}")


PINNED_W, PINNED_H = 320, 240


@functools.lru_cache(maxsize=None)
def _pinned_case():
    """-> (four 320 x 240 images, one list per image): case A's lists (image 0 has none), image 2's with one key listed twice.
    "Twice" is an exact repeat in the caller's list: no scale belongs to two levels (in binary32 a level's sigma_max never
    exceeds the next one's sigma_min: kc.level_table), so that is the only way a key comes twice."""
    imgs = np.stack([fixtures.synthetic_blobs(PINNED_W, PINNED_H, i) for i in range(4)])
    imgs.setflags(write=False)
    lists = list(kc.case_a())
    lists[2] = np.concatenate([lists[2], lists[2][5:6]])
    return imgs, tuple(lists)


@functools.lru_cache(maxsize=None)
def _pinned_expected(flag):
    """The oracle's single-image runs of _pinned_case()."""
    imgs, lists = _pinned_case()
    o = _oracle("default")
    out = []
    for b, keys in enumerate(lists):
        if not len(keys):
            out.append(None)
            continue
        o.run(imgs[b][None])
        assert o.run_keypoints(keys, flag) == len(keys)
        out.append(o.fetch(0))
    return out


@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("side", [True, False])
def test_lists_on_pinned_pixels(gpu_ctx_factory, monkeypatch, side, flag):
    """set_keypoints_batch + submit_host of PINNED pixels + wait: a submitted batch of four is delivered by the copier thread,
    so the lists' order crosses by its copy -- behind the side upload (the thread enqueues the batch itself), or behind a copy
    on the stream (HESS_NO_SIDE_UPLOAD=1).  Same counts, bytes and list order as run_keypoints_batch on the same pixels from
    pageable memory on a second context, and as the oracle."""
    import torch
    imgs, lists = _pinned_case()
    assert len(lists[0]) == 0 and lists[2][-1].tobytes() == lists[2][5].tobytes()
    if not side:
        monkeypatch.setenv("HESS_NO_SIDE_UPLOAD", "1")
    g = gpu_ctx_factory(dev_switches=True)
    monkeypatch.delenv("HESS_NO_SIDE_UPLOAD", raising=False)
    ref = _context(gpu_ctx_factory, "default")
    ref.run(np.array(imgs))
    assert ref.run_keypoints_batch(lists, flag) == [len(k) for k in lists]
    pinned = torch.from_numpy(np.array(imgs)).pin_memory()
    g.set_keypoints_batch(lists, flag)
    g.submit_host(ptr=pinned.data_ptr(), batch=4, height=PINNED_H, width=PINNED_W)
    g.wait()
    want = _pinned_expected(flag)
    table = kc.level_table(noct=kc.octaves(PINNED_W, PINNED_H))
    for b, keys in enumerate(lists):
        what = f"pinned pixels, side upload {side}, flag {flag}, image {b}"
        assert g.count(b) == ref.count(b) == len(keys), what
        (gk, gd), (rk, rd) = g.fetch(b), ref.fetch(b)
        assert gk.tobytes() == rk.tobytes() and gd.tobytes() == rd.tobytes(), what
        assert np.array_equal(g.key_list_order(b), ref.key_list_order(b)), what
        assert np.array_equal(g.key_list_order(b), kc.list_order(keys, flag, table)), what
        _check_image(g, b, keys, want[b], what)


def test_errors(gpu_ctx_factory):
    lists, imgs = kc.case_a(), kc.images(4)
    g = _context(gpu_ctx_factory, "default")
    with pytest.raises(HessError) as e:
        g.run_keypoints_batch(lists, 1)  # no current batch
    assert e.value.code == _abi.HESS_ERR_STATE
    # nimg != batch: refused with both numbers, the lists stay
    g.set_keypoints_batch(lists[1:], 1)
    with pytest.raises(HessError) as e:
        g.run(imgs)
    assert e.value.code == _abi.HESS_ERR_ARG and "3" in str(e.value) and "4" in str(e.value)
    assert g.run(imgs[:3]) == [len(k) for k in lists[1:]]
    # a negative count
    k = np.ascontiguousarray(lists[3])
    assert g._f["set_keypoints_batch"](g._h, k.ctypes.data_as(C.c_void_p), (C.c_int * 2)(5, -1), 2, 1) == _abi.HESS_ERR_ARG
    # set while a batch is pending
    g.submit_host(imgs)
    with pytest.raises(HessError) as e:
        g.set_keypoints_batch(lists, 1)
    assert e.value.code == _abi.HESS_ERR_STATE
    g.wait()
    assert g.count(0) > 0  # a plain detection run: the refused lists (none for image 0) were not stored
    # a pending hess_debug_key_levels override: the hook is a single-image affair
    g.debug_key_levels(np.zeros(4, np.int32))
    with pytest.raises(HessError) as e:
        g.set_keypoints_batch(lists, 1)
    assert e.value.code == _abi.HESS_ERR_STATE
    with pytest.raises(HessError) as e:
        g.run_keypoints_batch(lists, 1)
    assert e.value.code == _abi.HESS_ERR_STATE
    g.debug_key_levels(None)
    # run_keypoints_batch with the wrong number of images (the current batch has four)
    with pytest.raises(HessError) as e:
        g.run_keypoints_batch(lists[:3], 1)
    assert e.value.code == _abi.HESS_ERR_ARG and "3" in str(e.value) and "4" in str(e.value)
    # a total of 0 clears pending lists
    g.set_keypoints_batch(lists, 1)
    g.set_keypoints_batch([lists[0]], 1)
    o = _oracle("default")
    assert g.run(imgs[:2]) == o.run(imgs[:2])
