"""Planes below one tile on the HIP path: every case of detector_cases.small_cases() -- one-octave planes from 4 x 1 up,
the smallest pyramids with a second and a third octave, the input stages, batches of eight and keypoint lists on them --
(a) against the float64 model, (b) bit for bit against the CPU oracle, with and without the kept levels; then (c) the kernel
form each size is there for, from the per-kernel launch counters; (d) one context through large and small sizes and batches;
(e) keypoints whose window holds no sample, in both descriptor formats; (f) a stack with feature-less images under every
delivery; (g) the refusals.  tests/test_small_images.py holds the oracle to the model on the same cases.

The kernels work on fixed blocks (64 x 32 Gaussian tiles with halos of up to 16 taps, 32 x 32 chain tiles, 128 x 4 extrema
tiles, 124-column scan strips in 24- or 12-row segments, 64-column row-mask words): here every block is a partial one and
every index a clamped or a wrapped one.

Contexts are shared between the tests of this file by parameter set: a context that runs one size after another is part of
what is tested (grow-only buffers, the plan's shortcut for an unchanged size).

(c) reads launches per kernel family (hess_schedule.hip books one per launch): "input" is convert_kernel (+ the
up-sampling), "gauss" every pyramid launch, "gauss_octave0" those of octave 0, "hessian" the det-H launches outside the
pyramid (none while the top level's det-H is fused into its launch; two in the difference-of-Gaussians mode), "extrema"
the scan and the placing.  The two extrema scans book the same two launches: which one runs follows from dog_level_num alone
(k_detect.hip, extrema_streams: the streaming scan up to 5, the LDS-tiled one above), so those two cases assert the count
and rest on that rule.
"""
import os
from contextlib import closing

import numpy as np
import pytest

import detector_cases as dc
from hessgpu_amd import _abi
from hessgpu_amd.session import HessError
from oracle_lib import OracleSession, oracle_quantize
from parity_compare import assert_same_features, compare_all, compare_results

pytestmark = pytest.mark.gpu

SMALL = dc.small_cases()
NAMES = list(SMALL)
K = dc.NOISE_KW
SWITCHES = ("HESS_CHAIN_FROM", "HESS_NO_PAIR", "HESS_NO_TOP_FUSION", "HESS_DELIVERY")


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    """One product context per (parameters, switches) for the whole file, with the launch counters on.  env: switches read
    when the context is created (HESS_DELIVERY by either build, the others by the developer build)."""
    made = {}

    def get(env=None, **kw):
        key = (tuple(sorted(kw.items())), tuple(sorted((env or {}).items())))
        if key not in made:
            old = {k: os.environ.get(k) for k in SWITCHES}
            try:
                for k in SWITCHES:
                    os.environ.pop(k, None)
                os.environ.update(env or {})
                dev = any(k != "HESS_DELIVERY" for k in (env or {}))
                made[key] = gpu_ctx_factory(dev_switches=True, **kw) if dev else gpu_ctx_factory(**kw)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            made[key].profile_enable(True)
        return made[key]

    return get


def _results(g, case, index=0):
    """The results the context holds now; a keypoint-list run has no raw list of its own."""
    keys, desc = g.fetch(index)
    raw = g.rawlist(index).tobytes() if case is None or case.keys is None else b""
    return raw, keys.tobytes(), desc.tobytes()


def _all_results(g, batch):
    return [_results(g, None, b) for b in range(batch)]


# ---- a: the model on the HIP path ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_hip_path_follows_the_model(ctx, name):
    case = SMALL[name]
    g = ctx(**case.kw)
    st = dc.check_against_model(g, case)
    print(name, st)
    dc.check_small_statistics(st, case)
    # the production schedule gives what the model has just judged
    stack, index = dc.case_input(case)
    kept = _results(g, case, index)
    g.keep_levels(False)
    g.run(stack, fmt=case.fmt)
    if case.keys is not None:
        g.run_keypoints(case.keys, case.have_orientation)
    prod = _results(g, case, index)
    for what, a, b in zip(("raw list", "keypoints", "descriptors"), kept, prod):
        assert a == b, f"{what}: keep_levels(False) differs from the kept-levels run"


# ---- b: bit parity with the oracle --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_bit_parity_with_the_oracle(ctx, name):
    """Every plane of every level, the raw list, keypoints and descriptors; a batch case compares its whole stack of eight."""
    case = SMALL[name]
    g = ctx(**case.kw)
    stack, _ = dc.case_input(case)
    with closing(OracleSession(threads=4, **case.kw)) as o:
        for stages in (True, False):
            what = f"{name} stages={stages}"
            no = compare_all(g, o, stack, what, stages=stages)
            if case.keys is None:
                assert no[dc.case_input(case)[1]] == case.min_features, what
            if case.keys is not None:
                ng, nk = g.run_keypoints(case.keys, case.have_orientation), o.run_keypoints(case.keys, case.have_orientation)
                assert ng == nk == len(case.keys), what
                assert_same_features(*g.fetch(0), *o.fetch(0), what + " keypoint list")


def test_stack_with_featureless_images_parity(ctx):
    stack = dc.constant_stack(65, 33)
    g = ctx(**K)
    with closing(OracleSession(threads=4, **K)) as o:
        for stages in (True, False):
            no = compare_all(g, o, stack, f"constant stack stages={stages}", stages=stages)
        assert [no[j] for j in (0, 3, 4, 7)] == [0, 0, 0, 0] and min(no[j] for j in (1, 2, 5, 6)) > 0, no


# ---- c: the kernel forms --------------------------------------------------------------------------------------------------
# Launch counts of the default schedule (dog_level_num 3: levels 0 .. 4, level 3 decimated, the top level's det-H fused), per
# hess_schedule.hip.  One octave of u8 luminance: gauss_first_kernel (levels 0 + 1), levels 2, 3, 4 = 4 launches and no
# convert_kernel; any other input: convert_kernel, level 0 and four levels = 5.  A second octave, level by level: its level 1
# rides with octave 0's top level (the pair launch, booked with octave 0) and levels 2, 3, 4 follow = 3 + 1 + 3; without the
# pair 4 + 4.  Chained (one or two images by size; HESS_CHAIN_FROM): octave 0's levels up to 3, one chain launch per further
# octave, one multi-level launch for all top levels = 3 + 1 + 1.  A u8 row pitch that is no multiple of 4 (a packed image
# of odd width) is not read directly either: convert_kernel and a level-0 launch, one launch more in octave 0.

def _one(w, h):
    return lambda: dc.noise(w, h)[None]


def _n(inp, gauss, oct0, hessian=None, extrema=None):
    want = dict(input=inp, gauss=gauss, gauss_octave0=oct0, hessian=hessian, extrema=extrema)
    return {k: v for k, v in want.items() if v is not None}


def _eight():
    return dc.constant_stack(64, 33)


CHAIN_OFF, NO_PAIR, NO_TOP = dict(HESS_CHAIN_FROM="99"), dict(HESS_NO_PAIR="1"), dict(HESS_NO_TOP_FUSION="1")
FORMS = {
    # name: (stack, parameters, switches, launches: input, gauss, gauss_octave0, hessian, extrema)
    "gauss_first_kernel: u8 luminance 200x16": (_one(200, 16), {}, None, _n(0, 4, 4, 0, 2)),
    "gauss_first_kernel: 4x1": (_one(4, 1), {}, None, _n(0, 4, 4, 0, 2)),
    "convert_kernel + level launches: u8 rgb 36x5": (lambda: SMALL["u8 rgb 36x5"].image[None], {}, None, _n(1, 5, 5, 0)),
    "convert_kernel + level launches: f32 4x1": (lambda: SMALL["f32 lum 4x1"].image[None], {}, None, _n(1, 5, 5, 0)),
    "convert_kernel, then the chain: f32 65x33": (lambda: SMALL["f32 lum 65x33"].image[None], {}, None, _n(1, 6, 4, 0)),
    "chain + multi-level top launch by size: 64x33": (_one(64, 33), {}, None, _n(0, 5, 3, 0)),
    "chain on a thin second octave 500x16": (_one(1000, 33), {}, None, _n(0, 5, 3, 0)),
    "odd row pitch, convert_kernel, chain on a thin second octave 16x350": (_one(33, 700), {}, None, _n(1, 6, 4, 0)),
    "odd row pitch, convert_kernel, then the chain: 65x33": (_one(65, 33), {}, None, _n(1, 6, 4, 0)),
    "chain on two octaves: 128x64": (_one(128, 64), {}, None, _n(0, 6, 3, 0)),
    "pair launch: 64x33 in a stack of eight": (_eight, {}, None, _n(0, 7, 4, 0)),
    "chain forced on a stack of eight": (_eight, {}, dict(HESS_CHAIN_FROM="1"), _n(0, 5, 3, 0)),
    "pair launch: one image, chain off": (_one(64, 33), {}, CHAIN_OFF, _n(0, 7, 4, 0)),
    "level by level: chain and pair off": (_one(64, 33), {}, dict(CHAIN_OFF, **NO_PAIR), _n(0, 8, 4, 0)),
    "pair, then chain from octave 2: 128x64": (_one(128, 64), {}, dict(HESS_CHAIN_FROM="2"), _n(0, 8, 4, 0)),
    "top fusion off: 64x33": (_one(64, 33), {}, NO_TOP, _n(0, 5, 3, 1)),
    "top fusion off: 4x1": (_one(4, 1), {}, NO_TOP, _n(0, 4, 4, 1)),
    "streaming extrema scan: 300x3": (_one(300, 3), {}, None, _n(0, 4, 4, 0, 2)),
    "LDS-tiled extrema scan: dog_level_num 6, 200x16": (_one(200, 16), dict(dog_level_num=6), None, _n(0, 8, 8, 0, 2)),
    "33 taps: dog_level_num 1, 200x16": (_one(200, 16), dict(dog_level_num=1), None, _n(0, 3, 3, 0, 2)),
    "difference of Gaussians: 64x33": (_one(64, 33), dc.DOG, None, _n(0, 9, 5, 2, 2)),
    "up-sampling: first_octave -1, 36x5": (_one(36, 5), dict(first_octave=-1), None, _n(1, 5, 5)),
    "up-sampling, no first blur: first_octave -2, 36x5": (_one(36, 5), dict(first_octave=-2), None, _n(1, 4, 4)),
    "decimation to 148x1: first_octave 1, 300x3": (_one(300, 3), dict(first_octave=1), None, _n(1, 5, 5)),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_the_case_runs_the_kernel_form_it_is_there_for(ctx, form):
    make, kw, env, want = FORMS[form]
    kw = dict(K, **kw)
    stack = make()
    g = ctx(env=env, **kw)
    g.keep_levels(False)
    g.profile_reset()
    ng = g.run(stack)
    prof = g.profile()
    got = {k: prof[k]["launches"] for k in want}
    print(form, got, "counts", ng)
    assert got == want, f"{form}: launches {got}, expected {want}"
    if want["input"] == 0 and "detector" not in kw:
        # Whatever launches the form takes, their booked bytes sum to SURVEY 8(d)'s layout (the identity of test_gpu_parity.py::
        # test_profile_bytes_are_the_layouts_of_survey_8d, for dog levels): per octave pixel dog + 2 Gaussian levels x (4 W + 4 R),
        # dog + 2 det-H planes x 4 W and dog gradient/theta planes x 8 W = 20 dog + 24 B, + 1 B per u8 pixel read directly.
        dog = kw.get("dog_level_num") or 3
        planes = [w * h for w, h in g.geometry()]
        layout = len(stack) * ((20.0 * dog + 24.0) * sum(planes) + 1.0 * planes[0])
        booked = prof["gauss"]["bytes"] + prof["gauss"]["bytes_in_lds"] + prof["hessian"]["bytes"]
        print(form, "booked bytes", booked, "layout", layout)
        assert abs(booked - layout) < 1e-6 * layout, (prof["gauss"], prof["hessian"], layout)
    if form.startswith("gauss_first_kernel"):   # level 0 of octave 0 existed in LDS only: the dump is refused
        with pytest.raises(HessError):
            g.level(0, 0, 0, _abi.DBG_GAUSS)
    with closing(OracleSession(threads=4, **kw)) as o:   # and whatever the form, the oracle's bits
        for stages in (False, True):
            compare_all(g, o, stack, f"{form} stages={stages}", stages=stages)


# ---- d: one context through sizes and batches ---------------------------------------------------------------------------

def test_size_changes_on_one_context(gpu_ctx_factory):
    """Grow-only buffers, the plan's shortcut for an unchanged size, the zeroed block sized per plan: every step byte-equal to
    a fresh context on the same input."""
    g = gpu_ctx_factory(**K)
    fresh = {}
    for w, h in ((640, 480), (4, 1), (65, 33), (4, 300), (1000, 33), (12, 3), (640, 480)):
        img = dc.noise(w, h)[None]
        if (w, h) not in fresh:
            f = gpu_ctx_factory(**K)
            fresh[w, h] = (f.run(img), _all_results(f, 1))
        assert (g.run(img), _all_results(g, 1)) == fresh[w, h], f"{w}x{h} after other sizes differs from a fresh context"
    assert fresh[640, 480][0][0] > 100 and fresh[1000, 33][0][0] > 100 and fresh[4, 1][0] == [0]


def test_batch_changes_on_one_context(gpu_ctx_factory):
    stack = dc.constant_stack(65, 33)
    g = gpu_ctx_factory(**K)
    fresh = {}
    for n in (8, 1, 8):
        imgs = stack[5:6] if n == 1 else stack
        if n not in fresh:
            f = gpu_ctx_factory(**K)
            fresh[n] = (f.run(imgs), _all_results(f, n))
        assert (g.run(imgs), _all_results(g, n)) == fresh[n], f"batch {n} after another batch size differs from a fresh context"
    assert fresh[1][0] == [fresh[8][0][5]] and fresh[1][1][0] == fresh[8][1][5]


# ---- e: keypoints whose window holds no sample, in both descriptor formats ----------------------------------------------
# (model rows with an empty window, of the 40 keys of detector_cases._user_keys: every key on a plane of one or two rows; the
# keys at and beyond the border with first_octave -1: tests/test_small_images.py::test_the_key_lists_meet_empty_windows)
EMPTY = [((4, 1), m, 40) for m in ("defaults", "dog", "half_sift", "first_octave -1")] + \
        [((7, 2), m, 40) for m in ("defaults", "half_sift")] + [((64, 1), m, 40) for m in ("defaults", "dog")] + \
        [((7, 2), "first_octave -1", 9), ((4, 3), "first_octave -1", 9), ((12, 3), "first_octave -1", 9),
         ((36, 5), "first_octave -1", 9), ((300, 3), "first_octave -1", 9), ((4, 300), "first_octave -1", 9),
         ((17, 23), "first_octave -1", 1)]


@pytest.mark.parametrize("have_orientation", [1, 0])
@pytest.mark.parametrize("size,mode,empty", EMPTY, ids=[f"{w}x{h} {m}" for (w, h), m, _ in EMPTY])
def test_empty_windows_in_both_descriptor_formats(ctx, size, mode, empty, have_orientation):
    """min(0.2f, 0 * rsqrt(0)) keeps the operand that is not NaN (np_restatement.descriptor_ex): every component of such a
    row is 1 / sqrt(dim), as a float and as the matcher's byte -- never NaN, never zero."""
    w, h = size
    case = SMALL[f"keypoint list {w}x{h} {mode} orient={have_orientation}"]
    g = ctx(**case.kw)
    got = {}
    try:
        for fmt in ("f32", "u8", "f32"):
            g.set_descriptor_format(fmt)
            g.run(case.image[None])
            assert g.run_keypoints(case.keys, have_orientation) == len(case.keys)
            keys, desc = g.fetch(0)
            assert g.desc_format() == fmt and keys.tobytes() == case.keys.tobytes()
            if fmt in got:
                assert got[fmt].tobytes() == desc.tobytes(), "the floats changed after the byte run"
            got[fmt] = desc
    finally:
        g.set_descriptor_format("f32")   # (the context is shared with the other tests of this file)
    with closing(OracleSession(threads=4, **case.kw)) as o:
        o.run(case.image[None])
        o.run_keypoints(case.keys, have_orientation)
        want = o.fetch(0)[1]
    f, u = got["f32"], got["u8"]
    dim = f.shape[1]
    assert dim == (64 if mode == "half_sift" else 128) and f.dtype == np.float32 and u.dtype == np.uint8
    assert np.array_equal(f.view(np.uint32), want.view(np.uint32)), "floats differ from the oracle's"
    assert np.array_equal(u, oracle_quantize(f)), "bytes differ from the quantised floats"
    rows = np.ptp(want, axis=1) == 0                       # one value in every component: nothing was under the window
    assert int(rows.sum()) == empty, (int(rows.sum()), empty)
    assert np.isfinite(f).all()
    assert np.abs(f[rows] - 1.0 / np.sqrt(dim)).max() < dc.TOL_DESC
    assert (u[rows] == int(512.0 / np.sqrt(dim) + 0.5)).all() and u[rows].min() > 0


@pytest.mark.parametrize("have_orientation", [1, 0])
def test_empty_windows_without_normalisation_are_zero(ctx, have_orientation):
    case = SMALL[f"keypoint list 4x1 normalize 0 orient={have_orientation}"]
    g = ctx(**case.kw)
    with pytest.raises(HessError):                          # unnormalised descriptors have no byte format
        g.set_descriptor_format("u8")
    g.run(case.image[None])
    assert g.run_keypoints(case.keys, have_orientation) == len(case.keys)
    assert not g.fetch(0)[1].any()


# ---- f: delivery ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def constant_reference():
    stack = dc.constant_stack(65, 33)
    o = OracleSession(threads=4, keep_levels=False, **K)
    no = o.run(stack)
    yield stack, o, no
    o.close()


@pytest.mark.parametrize("how", ["mirror", "dma", "blit", "submit_host"])
def test_featureless_images_between_others_under_every_delivery(ctx, constant_reference, how):
    """Zero-feature images first, last and between non-empty ones in the packed results."""
    stack, o, no = constant_reference
    g = ctx(**K) if how == "submit_host" else ctx(env=dict(HESS_DELIVERY=how), **K)
    g.keep_levels(False)
    for imgs, want in ((stack, no), (stack[3:6], no[3:6]), (stack, no)):      # (3:6: empty, empty, non-empty)
        if how == "submit_host":
            g.submit_host(imgs)
            g.wait()
            ng = [g.count(b) for b in range(len(imgs))]
        else:
            ng = g.run(imgs)
        assert ng == want, f"{how}: counts {ng}, oracle {want}"
        if len(imgs) == len(stack):
            compare_results(g, o, ng, no, f"constant stack via {how}", stages=False)
    assert no[0] == no[3] == no[4] == no[7] == 0 and no[5] > 0


# ---- g: refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,kw", [(1, 5, {}), (2, 5, {}), (3, 5, {}), (3, 1, {}), (7, 1, dict(first_octave=1)),
                                    (4, 300, dict(first_octave=1))], ids=lambda v: str(v))
def test_too_small_is_refused_and_the_context_goes_on(ctx, w, h, kw):
    kw = dict(K, **kw)
    g = ctx(**kw)
    legal = dc.noise(300, 3)[None]
    g.keep_levels(False)
    g.run(legal)                                            # (a plan exists: the refusal must not leave half of another)
    g.profile_reset()
    with pytest.raises(HessError) as e:
        g.run(dc.noise(w, h)[None])
    assert e.value.code == _abi.HESS_ERR_ARG and "too small" in str(e.value)
    assert all(v["launches"] == 0 for v in g.profile().values()), "a refused call launched something"
    with closing(OracleSession(threads=4, **kw)) as o:
        for imgs in (legal, dc.noise(65, 33)[None]):
            compare_all(g, o, imgs, f"legal image after the refused {w}x{h}", stages=True)
