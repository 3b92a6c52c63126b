"""Float pixels of any range on the HIP path: every case of tests/float_range_cases.py -- luminance in 0 .. 2^8, 2^10, 2^16,
2^-8 .. 2^-20, 0 .. 255, 0 .. 65535, zero-mean and negated, as luminance, RGB and BGR, with the options that meet the value
range, keypoint lists and a batch --
(a) bit for bit against the CPU oracle: kept planes, raw list, keypoints, descriptors as floats and as bytes, through run,
    submit_host / wait and run_device on a torch tensor, with the levels kept and without;
(b) against the float64 model on the device session itself (detector_cases.check_against_model), nothing flagged;
(c) homogeneity on the device alone, no oracle and no tolerance: the planes, the list, the keypoints and the descriptors of
    A b from those of b for A a power of two (float_range_cases.check_homogeneous);
(d) the kernels such an image takes, from the launch counters and from the descriptor bits;
(e) the lists whose top-K keys are all equal, against the oracle and against the list model applied to the device's own
    untruncated list; the batch of three; one context through the amplitudes and back;
(f) the SiftGPU class with GL_FLOAT pixels above 1.
tests/test_float_range.py holds the oracle to the model on the same cases and shows that each wrong rule is caught.

Contexts: one per test, closed after it (nearly every case has its own threshold).
"""
from contextlib import closing

import numpy as np
import pytest

import detector_cases as dc
import float_range_cases as fc
import list_cases as L
import siftgpu_lib
from hessgpu_amd import _abi
from oracle_lib import OracleSession, oracle_quantize
from parity_compare import assert_same_features, compare_results
from test_list_boundaries_gpu import device_runner

pytestmark = pytest.mark.gpu

CASES = list(fc.cases())
PAIRS = fc.pairs()
LISTS = fc.list_cases()


def _results(s, b, raw=True):
    keys, desc = s.fetch(b)
    return (s.rawlist(b).tobytes() if raw else b""), keys.tobytes(), desc.tobytes()


def _all(s, n, raw=True):
    return [_results(s, b, raw) for b in range(n)]


def _on_device(stack):
    import torch

    d = torch.from_numpy(np.ascontiguousarray(stack)).to("cuda:0")
    torch.cuda.synchronize()
    return d


# ---- a: bit parity with the oracle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_bit_parity_with_the_oracle(gpu_ctx_factory, name):
    case = fc.cases()[name]
    stack, bi = dc.case_input(case)
    n, (h, w) = len(stack), stack.shape[1:3]
    channels = 1 if stack.ndim == 3 else stack.shape[3]
    g = gpu_ctx_factory(**case.kw)
    try:
        with closing(OracleSession(threads=4, **case.kw)) as o:
            no = o.run(stack, fmt=case.fmt)
            want = _all(o, n)
            assert no[bi] >= case.min_features and len(want[bi][0]) > 0
            for stages in (True, False):
                g.keep_levels(stages)
                ng = g.run(stack, fmt=case.fmt)
                compare_results(g, o, ng, no, f"{name} run stages={stages}", stages=stages)
            # (the production schedule from here on)
            g.submit_host(stack, fmt=case.fmt)
            g.wait()
            assert _all(g, n) == want, f"{name}: submit_host / wait differs from the oracle"
            d = _on_device(stack)
            g.run_device(d.data_ptr(), n, h, w, channels, _abi.PIX_F32, case.fmt)
            assert _all(g, n) == want, f"{name}: run_device differs from the oracle"
            del d
            if case.keys is not None:
                ng, nk = g.run_keypoints(case.keys, case.have_orientation), o.run_keypoints(case.keys, case.have_orientation)
                assert ng == nk == len(case.keys), name
                assert_same_features(*g.fetch(0), *o.fetch(0), name + " keypoint list")
            if g.params.normalize:      # the bytes are the matcher's quantisation of the floats (unnormalised ones have none)
                g.set_descriptor_format("u8")
                assert g.run(stack, fmt=case.fmt) == no
                if case.keys is not None:
                    g.run_keypoints(case.keys, case.have_orientation)
                for b in range(1 if case.keys is not None else n):
                    (gk, gu), (ok, od) = g.fetch(b), o.fetch(b)
                    assert gu.dtype == np.uint8 and gk.tobytes() == ok.tobytes(), f"{name}: keypoints of the byte run, image {b}"
                    assert np.array_equal(gu, oracle_quantize(od)), f"{name}: bytes differ from the quantised floats, image {b}"
    finally:
        g.close()


# ---- b: the model on the device -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_hip_path_follows_the_model(gpu_ctx_factory, name):
    case = fc.cases()[name]
    g = gpu_ctx_factory(**case.kw)
    try:
        st = dc.check_against_model(g, case)
        print(name, st)
        fc.check_statistics(st, case)
        # the production schedule gives what the model has just judged
        stack, index = dc.case_input(case)
        pixel = case.keys is None
        kept = _results(g, index if pixel else 0, raw=pixel)
        g.keep_levels(False)
        g.run(stack, fmt=case.fmt)
        if not pixel:
            g.run_keypoints(case.keys, case.have_orientation)
        prod = _results(g, index if pixel else 0, raw=pixel)
        assert len(kept[1]) > 0
        for what, a, b in zip(("raw list", "keypoints", "descriptors"), kept, prod):
            assert a == b, f"{what}: keep_levels(False) differs from the kept-levels run"
    finally:
        g.close()


# ---- c: homogeneity on the device alone -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PAIRS))
def test_hip_path_is_homogeneous(gpu_ctx_factory, name):
    ca, cb, k, lists = PAIRS[name]
    ga, gb = gpu_ctx_factory(**ca.kw), gpu_ctx_factory(**cb.kw)
    try:
        a, b = fc.snapshot(ga, ca), fc.snapshot(gb, cb)
    finally:
        ga.close()
        gb.close()
    fc.check_homogeneous(a, b, k, lists, fc.half_regime(ca), fc.half_regime(cb))


# ---- d: the kernels a float image takes -------------------------------------------------------------------------------------
# The launch counters are per family (hess_schedule.hip books one per launch): "input" is convert_kernel with the
# up-sampling, and a u8 luminance image that gauss_first_kernel reads directly books none.  The descriptor family does not
# say which of its kernels ran; the bits do: under the default order (PIXEL) a float image gets the descriptors of
# descriptor_order = INTERLEAVED, an 8-bit image of the same content does not.

def _profiled(gpu_ctx_factory, stack, **kw):
    g = gpu_ctx_factory(**kw)
    try:
        g.profile_enable(True)
        g.keep_levels(False)
        g.profile_reset()
        n = g.run(stack)
        prof = {k: v["launches"] for k, v in g.profile().items()}
        return n, prof, g.geometry(), _all(g, len(stack))
    finally:
        g.close()


def test_a_float_image_takes_convert_kernel_and_the_interleaved_descriptor(gpu_ctx_factory):
    case = fc.cases()["float: blobs 2^8"]
    u8 = dc.blobs_noise()[None]
    kw = dict(dog_threshold=float(fc.T_DEFAULT))
    nf, pf, _, rf = _profiled(gpu_ctx_factory, case.image[None], **case.kw)
    ni, pi, _, ri = _profiled(gpu_ctx_factory, case.image[None], descriptor_order=_abi.DESC_ORDER_INTERLEAVED, **case.kw)
    nu, pu, _, ru = _profiled(gpu_ctx_factory, u8, **kw)
    nv, pv, _, rv = _profiled(gpu_ctx_factory, u8, descriptor_order=_abi.DESC_ORDER_INTERLEAVED, **kw)
    print("float", pf, "u8", pu)
    assert pf["input"] == 1 and pu["input"] == 0                       # convert_kernel / gauss_first_kernel on the pixels
    assert pf["gauss_octave0"] == pu["gauss_octave0"] + 1              # level 0 is a launch of its own after convert_kernel
    assert pf["descriptor"] >= 1 and pf["descriptor"] == pi["descriptor"]
    assert nf == ni and nf[0] >= 50 and rf == ri, "the default order of a float image is not the interleaved one"
    assert nu == nv and ru[0][1] == rv[0][1] and ru[0][2] != rv[0][2], "an 8-bit image has the pixel order's bits by default"


@pytest.mark.parametrize("fo,geometry", [(-1, (192, 160)), (1, (80, 60))])
def test_up_sampling_and_decimation_of_a_float_plane_run(gpu_ctx_factory, fo, geometry):
    case = fc.cases()[f"float: blobs 2^8 first_octave {fo}"]
    n, prof, geo, _ = _profiled(gpu_ctx_factory, case.image[None], **case.kw)
    print(fo, prof, geo)
    assert prof["input"] == 1 and geo[0] == geometry and n[0] >= 50, (prof, geo, n)


# ---- e: lists, the batch, one context through the amplitudes -------------------------------------------------------------

@pytest.mark.parametrize("name", list(LISTS))
def test_lists_with_equal_keys(gpu_ctx_factory, name):
    """Against the oracle's bytes (run and submit_host / wait) and against the list model applied to the device's own
    untruncated list; all keys equal, the first K kept."""
    case = LISTS[name]
    run = device_runner(case, gpu_ctx_factory, [])
    st = L.check_case(run, case)
    fc.check_list_reach(st, case, run)


def test_each_image_of_the_batch_equals_its_single_run(gpu_ctx_factory):
    stack = fc.batch_stack()
    kw = dict(dog_threshold=fc.BATCH_THRESHOLD)
    g = gpu_ctx_factory(**kw)
    try:
        assert g.run(stack) == fc.BATCH_FEATURES
        batch = _all(g, 3)
        g.submit_host(stack)
        g.wait()
        assert _all(g, 3) == batch
    finally:
        g.close()
    for b in range(3):
        f = gpu_ctx_factory(**kw)
        try:
            assert f.run(stack[b:b + 1]) == fc.BATCH_FEATURES[b:b + 1]
            assert _results(f, 0) == batch[b], f"image {b} of the batch differs from its single-image run"
        finally:
            f.close()
    with closing(OracleSession(threads=4, keep_levels=False, **kw)) as o:
        assert o.run(stack) == fc.BATCH_FEATURES and _all(o, 3) == batch


def test_one_context_through_the_amplitudes_and_back(gpu_ctx_factory):
    """[0, 1], 2^16 (every response inf), 2^-14 (no response reaches the threshold) and [0, 1] again on one context, each
    byte-equal to a fresh context: nothing of an image's range stays behind."""
    stack = fc.batch_stack()
    kw = dict(dog_threshold=fc.BATCH_THRESHOLD)
    fresh = []
    for b in range(3):
        f = gpu_ctx_factory(**kw)
        try:
            fresh.append((f.run(stack[b:b + 1]), _results(f, 0)))
        finally:
            f.close()
    assert [f[0][0] for f in fresh] == fc.BATCH_FEATURES
    g = gpu_ctx_factory(**kw)
    try:
        for b in (0, 1, 2, 0, 2, 1):
            assert (g.run(stack[b:b + 1]), _results(g, 0)) == fresh[b], f"image {b} on the travelled context"
    finally:
        g.close()


# ---- f: the SiftGPU class -------------------------------------------------------------------------------------------------
# ParseParam takes -t only inside (0, 0.5), as the reference does (SiftGPU.cpp:1197): the threshold of a 0 .. 255 image,
# 0.00667 x 255^2 = 433.5, cannot be given to the class, and such an image runs under the threshold the class has.  An
# amplitude up to 8 leaves the scaled threshold below 0.5.

def _class_against_oracle(args, img, gl_format, fmt, threshold, **kw):
    s = siftgpu_lib.SiftGPU(args)
    try:
        assert s.create_context() == 2
        p = s.params()
        assert p.dog_threshold == np.float32(threshold), (p.dog_threshold, threshold)
        assert s.run(img, gl_format, siftgpu_lib.GL_FLOAT) == 1
        k, d = s.features()
    finally:
        s.close()
    with closing(OracleSession(threads=4, keep_levels=False, dog_threshold=float(np.float32(threshold)), **kw)) as o:
        o.run(img[None], fmt=fmt)
        ok, od = o.fetch(0)
    assert len(k) >= 50 and k.tobytes() == ok.tobytes() and np.array_equal(d.view(np.uint32), od.view(np.uint32))
    return len(k)


def test_siftgpu_class_float_luminance_0_255():
    img = fc.cases()["float: blobs 255"].image
    scaled = fc.threshold(fc.T_DEFAULT, 255.0)
    # the scaled threshold is refused and the default stays: every extremum of ordinary contrast passes
    n = _class_against_oracle(["-t", "%.9g" % scaled], img, siftgpu_lib.GL_LUMINANCE, None, fc.T_DEFAULT)
    assert scaled > 0.5 and n > 80


def test_siftgpu_class_float_rgb_above_one_with_its_threshold():
    img = fc.times(fc.unit(dc.colour(96, 80)), 8.0)
    scaled = fc.threshold(dc.COLOUR_KW["dog_threshold"], 8.0)
    assert img.max() > 7.0 and scaled < 0.5
    _class_against_oracle(["-t", "%.9g" % scaled, "-e", "%.9g" % dc.COLOUR_KW["edge_threshold"]], img, siftgpu_lib.GL_RGB, None, scaled,
                          edge_threshold=dc.COLOUR_KW["edge_threshold"])
