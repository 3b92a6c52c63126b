"""Rectangle descriptors (keys_have_orientation == -1) on the HIP path: the checker of tests/rect_cases.py on a product
context -- every rectangle against the float64 model computed from the context's own gradient planes -- for every option
the mode meets, through both entries; reproducibility of the bits whatever the list; the byte format; the SiftGPU class;
and flag 1 on the same array, unchanged.

tests/test_rect_model.py shows without a GPU that the checker raises for each wrong rule, the oriented descriptor at
(x, y, s, o) -- what flag -1 returned before the mode existed -- among them."""
import ctypes as C

import numpy as np
import pytest

import rect_cases as rc
from hessgpu_amd import _abi
from oracle_lib import OracleSession, oracle_quantize

pytestmark = pytest.mark.gpu

SETTINGS = {
    "defaults": {},
    "half_sift": dict(half_sift=1),
    "dynamic_indexing": dict(dynamic_indexing=1),
    "normalize 0": dict(normalize=0),
    "lowe_origin": dict(lowe_origin=1),
    "first_octave -1": dict(first_octave=-1),
    "dog detector": dict(detector=_abi.DETECTOR_DOG),
    "float luminance": {},
}


def _cases(name):
    cases = rc.cases(SETTINGS[name])
    if name == "float luminance":          # values up to 255: floats are taken as they are
        for c in cases:
            c.image = c.image.astype(np.float32)
            assert c.image.max() > 200
    return cases


@pytest.mark.parametrize("entry", ["run_keypoints", "set_keypoints"])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_rectangles_follow_the_model(gpu_ctx_factory, name, entry):
    g = gpu_ctx_factory(**SETTINGS[name])
    worst, levels, empty = 0.0, set(), 0
    for case in _cases(name):
        st = rc.check_rectangles(g, case, entry)
        print(name, entry, case.name, {k: v for k, v in st.items() if k != "levels"})
        worst, levels, empty = max(worst, st["worst"]), levels | st["levels"], empty + st["empty"]
    assert levels == set(range(len(g.geometry()) * 3)), "a rectangle on every level of every octave"
    assert empty >= 8          # the four empty windows of the 65- and of the 300-list
    # the list is consumed: a plain run detects again
    assert g.run(case.image[None])[0] > 0


def eight_case():
    """A float image that doubles every two columns, with noise of an ulp or two: the gradient points along +x, its
    vertical part is a few ulps of the value either way, so theta is within 2e-7 rad of zero on both sides -- and where it
    is above, -theta 4/pi + 8 rounds to 8.0: dropped without dynamic_indexing, bin 8 = bin 0 with it."""
    h, w = 80, 96
    _, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.RandomState(3)
    img = (2.0 ** (xx / 2) * (1 + 3e-7 * (rng.rand(h, w) - 0.5))).astype(np.float32)
    keys = rc.rect_keys([[20.0, 15.0, 30.0, 28.0], [40.5, 30.25, 27.0, 40.0]])
    return rc.SimpleNamespace(name="doubling columns", image=img, fmt=None, keys=keys)


def test_dynamic_indexing_sample_at_eight(gpu_ctx_factory):
    case = eight_case()
    out = {}
    for di in (0, 1):
        g = gpu_ctx_factory(dynamic_indexing=di, normalize=0)
        rc.check_rectangles(g, case)
        out[di] = g.fetch(0)[1].copy()
    assert not np.array_equal(out[0], out[1]), "the bin coordinate 8.0 was not met"


def test_debug_key_levels_still_override_the_binning(gpu_ctx_factory):
    """The parity hook puts a rectangle on a given level: the record is packed with that octave's scale and the descriptor
    comes from that level's plane.  Every square moves to another level of its own octave."""
    import np_restatement as R

    case = rc.cases()[2]
    g = gpu_ctx_factory()
    m = R.DetectorModel(g.params)
    h, w = case.image.shape[:2]
    _, _, geo, scales = m.plan(w, h)
    keys = case.keys[:len(scales) * m.dog]          # the squares, one per level
    own = [m.bin_key(rc.rect_sigma(k), scales)[0] for k in keys]
    assert own == list(range(len(keys)))
    forced = [(li // m.dog) * m.dog + (li % m.dog + 1) % m.dog for li in own]
    g.run(case.image[None])
    g.debug_key_levels(forced)
    assert g.run_keypoints(keys, rc.RECT) == len(keys)
    out, desc = g.fetch(0)
    assert out.tobytes() == keys.tobytes()
    for i, (k, li) in enumerate(zip(keys, forced)):
        oc, l = li // m.dog, li % m.dog + 1
        plane = g.level(0, oc, l, _abi.DBG_GOT).astype(np.float64)
        d = rc.rect_descriptor_ex(plane[..., 0], plane[..., 1], *rc.rect_record(m, k, scales[oc]))
        assert float(np.abs(d - desc[i]).max()) < rc.TOL_DESC, (i, li)
    # the hook covers one run: the same list again is binned by its sizes
    assert g.run_keypoints(keys, rc.RECT) == len(keys)
    again = g.fetch(0)[1]
    assert not np.array_equal(again, desc)


def test_bits_do_not_depend_on_the_list(gpu_ctx_factory):
    case = rc.cases()[3]
    keys = case.keys
    assert len(keys) == 300
    g = gpu_ctx_factory()
    g.run(case.image[None])

    def run(sel):
        assert g.run_keypoints(keys[sel], rc.RECT) == len(sel)
        return g.fetch(0)[1].copy()

    order = np.arange(300)
    first = run(order)
    assert np.array_equal(run(order).view(np.uint32), first.view(np.uint32)), "the same list twice"
    for _ in range(2):
        back = run(order[::-1])
        assert np.array_equal(back[::-1].view(np.uint32), first.view(np.uint32)), "the list reversed"
    # squares, 5 : 1 and 1 : 5, the boxes across the band seams, the tall one, the wrapped width, seeded ones
    for i in (0, 10, 11, 12, 13, 14, 18, 23, 150, 299):
        for _ in range(2):
            alone = run(np.array([i]))
            assert np.array_equal(alone[0].view(np.uint32), first[i].view(np.uint32)), f"rectangle {i} alone"


@pytest.mark.parametrize("half", [0, 1])
def test_byte_descriptors(gpu_ctx_factory, half):
    case = rc.cases(dict(half_sift=half))[2]
    g = gpu_ctx_factory(half_sift=half)
    g.run(case.image[None])
    assert g.run_keypoints(case.keys, rc.RECT) == len(case.keys)
    floats = g.fetch(0)[1].copy()
    assert floats.dtype == np.float32 and floats.shape[1] == (64 if half else 128)
    g.set_descriptor_format("u8")
    for entry in ("run_keypoints", "set_keypoints"):
        assert rc.run_case(g, case, entry) == len(case.keys)
        keys, got = g.fetch(0)
        assert got.dtype == np.uint8 and keys.tobytes() == case.keys.tobytes()
        assert np.array_equal(got, oracle_quantize(floats)), f"{entry}: bytes differ from the quantised floats"


def test_siftgpu_class_and_flat_mirror(gpu_ctx_factory):
    import siftgpu_lib

    case = rc.cases()[2]
    keys = case.keys
    g = gpu_ctx_factory()
    want = {}
    for entry in ("run_keypoints", "set_keypoints"):
        assert rc.run_case(g, case, entry) == len(keys)
        want[entry] = tuple(a.tobytes() for a in g.fetch(0))
    s = siftgpu_lib.SiftGPU([])
    L = s.L
    L.siftgpu_run_keys.restype = C.c_int
    L.siftgpu_run_keys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.siftgpu_set_keys.restype = None
    L.siftgpu_set_keys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    # the list before the context exists: it waits in the class and reaches the context created by the run, flag and all
    L.siftgpu_set_keys(s.h, len(keys), keys.ctypes.data, -1)
    assert s.run(case.image, siftgpu_lib.GL_LUMINANCE, siftgpu_lib.GL_UNSIGNED_BYTE) == 1
    assert tuple(a.tobytes() for a in s.features()) == want["set_keypoints"]
    # on the current image
    assert L.siftgpu_run_keys(s.h, len(keys), keys.ctypes.data, -1) == 1
    assert tuple(a.tobytes() for a in s.features()) == want["run_keypoints"]
    # and the list set on a live context
    L.siftgpu_set_keys(s.h, len(keys), keys.ctypes.data, -1)
    assert s.run(case.image, siftgpu_lib.GL_LUMINANCE, siftgpu_lib.GL_UNSIGNED_BYTE) == 1
    assert tuple(a.tobytes() for a in s.features()) == want["set_keypoints"]
    s.close()


def test_flag_one_is_unchanged(gpu_ctx_factory):
    """The same array with flag 1 is a list of oriented keypoints, as ever: bit-equal to the oracle."""
    case = rc.cases()[2]
    g, o = gpu_ctx_factory(), OracleSession(threads=8)
    g.run(case.image[None]); o.run(case.image[None])
    assert g.run_keypoints(case.keys, 1) == o.run_keypoints(case.keys, 1) == len(case.keys)
    (gk, gd), (ok, od) = g.fetch(0), o.fetch(0)
    assert gk.tobytes() == ok.tobytes() == case.keys.tobytes()
    assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), "flag 1 differs from the oracle"
    rect = g.run_keypoints(case.keys, rc.RECT) and g.fetch(0)[1]
    assert not np.array_equal(rect, gd), "flag -1 and flag 1 give the same descriptors"
    o.close()
