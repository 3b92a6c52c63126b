"""The 64-d matcher on the GPU (Matcher(dim=64), hess_matcher_set_dim, SiftMatchGPU "-half"): match_mfma_kernel<*, 64>,
match_dot_kernel<64> and bank_build_kernel<*, 64> against the CPU oracle.

The result for 64-d sets is by definition what the oracle returns for the same rows with 64 zero columns appended
(matcher_cases_half.pad128): integer work, every comparison is exact, and every one asserts first that the expectation is
not empty where tests/test_matcher_half_cases.py shows it is not.  The inputs are the cases of matcher_cases.py and
guided_cases.py folded to 64 columns: the same sizes, so the same row blocks, super tiles, segments and placed ties."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
import guided_cases as gc
import matcher_cases as mc
import matcher_cases_half as mh
from oracle_lib import oracle_match, oracle_quantize

pytestmark = pytest.mark.gpu


def _ref(a, b, **kw):
    return oracle_match(mh.pad128(a), mh.pad128(b), **kw)


def _check_single(m, a, b, label):
    """set 1 = a, set 2 = b through the single-pair entry point: every configuration, and a max_match at half the count."""
    assert m.dim == 64 and a.shape[1] == b.shape[1] == 64
    m.set_descriptors(0, a)
    m.set_descriptors(1, b)
    n1 = len(a)
    for dm, rm, mutual in mc.CONFIGS:
        ref = _ref(a, b, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
        assert len(ref) > 0, (label, dm, rm, mutual)
        got = m.match(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
        assert np.array_equal(got, ref), (label, dm, rm, mutual, mc.first_difference(ref, got))
        cut = len(ref) // 2
        if cut:
            got = m.match(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=cut)
            assert len(got) == cut and np.array_equal(got, ref[:cut]), (label, dm, rm, mutual, cut)


# ---- single pairs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", mc.MATRIX_CORE_SIZES)
def test_single_pair_on_the_matrix_cores(n1, n2):
    """n1 * n2 > 3 Mi: match_mfma_kernel<*, 64> + match_finish_kernel, on the geometry matcher_cases.MATRIX_CORE_SIZES names
    (a ragged row block, a one-column last super tile, 47 row blocks, 12-tile segments)."""
    from hessgpu_amd.matcher import Matcher

    a, b = mh.single_pair(n1, n2)
    m = Matcher(0, max_sift=max(n1, n2), dim=64)
    _check_single(m, a, b, (n1, n2))
    m.close()


@pytest.mark.parametrize("n1,n2", mc.SMALL_PATH_SIZES)
def test_single_pair_under_the_threshold(n1, n2):
    """match_dot_kernel<64> / match_row_kernel / match_col_kernel."""
    from hessgpu_amd.matcher import Matcher

    a, b = mh.single_pair(n1, n2)
    m = Matcher(0, max_sift=4096, dim=64)
    _check_single(m, a, b, (n1, n2))
    m.close()


def test_single_pair_straddling_the_threshold():
    """The switch counts scores, not bytes: 1536 x 2048 is the largest small-path problem at 64-d too."""
    from hessgpu_amd.matcher import Matcher

    s1, s2 = mh.straddle_sets()
    m = Matcher(0, max_sift=4096, dim=64)
    for a in (s1[:-1], s1):
        _check_single(m, a, s2, ("straddle", len(a)))
    m.close()


# ---- bank -------------------------------------------------------------------------------------------------------------

BANK_CONFIGS = [dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=mc.BANK_MAX_SIFT) for dm, rm, mutual in mc.CONFIGS]
BANK_CONFIGS += [dict(distmax=2.0, ratiomax=2.0, mutual_best=False, max_match=100),      # max_match below the match count
                 dict(distmax=0.7, ratiomax=0.8, mutual_best=True, max_match=100)]


@functools.lru_cache(maxsize=None)
def _bank_ref(k):
    """The oracle on the padded bank for BANK_CONFIGS[k]: {(a, b): matches} over all ordered pairs.  Computed once, shared."""
    pads = [mh.pad128(s) for s in mh.bank_sets()]
    uniq = [tuple(p) for p in mc.bank_all_pairs()]
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
        res = list(ex.map(lambda p: oracle_match(pads[p[0]], pads[p[1]], **BANK_CONFIGS[k]), uniq))
    for r in res:
        r.setflags(write=False)
    return dict(zip(uniq, res))


def _expect_matches(p, ref, cfg):
    """Every expected result is non-empty, but for the named exceptions: an empty side and the all-zero set."""
    if mc.BANK_SIZES.index(0) in p or mc.BANK_ZERO_SET in p:
        assert len(ref) == 0, (cfg, p)
    else:
        assert len(ref) > 0, (cfg, p)


def _check_pairs_against(m, pairs, k):
    cfg, ref = BANK_CONFIGS[k], _bank_ref(k)
    got = m.match_pairs(pairs, **cfg)
    for g, (a, b) in zip(got, pairs):
        _expect_matches((a, b), ref[a, b], cfg)
        assert np.array_equal(g, ref[a, b]), (cfg, a, b, mc.first_difference(ref[a, b], g))
    return got


@pytest.fixture(scope="module")
def bank64():
    from hessgpu_amd.matcher import Matcher

    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT, dim=64)
    m.set_bank(mh.bank_sets())
    yield m
    m.close()


def test_bank_reads_back():
    from hessgpu_amd.matcher import Matcher

    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT, dim=64)
    sets = mh.bank_sets()
    m.set_bank(sets)
    for i, s in enumerate(sets):
        got = m.bank(i)
        assert got.shape == (len(s), 64) and np.array_equal(got, s), i
    # truncation to max_sift happens at load time, at 64 bytes a row
    m.close()
    m = Matcher(0, max_sift=1000, dim=64)
    m.set_bank(sets)
    for i, s in enumerate(sets):
        assert np.array_equal(m.bank(i), s[:1000]), i
    m.close()


@pytest.mark.parametrize("k", range(len(BANK_CONFIGS)))
def test_bank_all_ordered_pairs(bank64, k):
    """match_pairs == oracle == the single-pair call, pair by pair, over all ordered pairs ((a, a) included)."""
    pairs = mc.bank_all_pairs()
    assert len(pairs) > mc.BANK_CHUNK
    got = _check_pairs_against(bank64, pairs, k)
    if BANK_CONFIGS[k]["max_match"] == 100:
        assert max(len(g) for g in got) == 100
    sets = mh.bank_sets()
    for g, (a, b) in zip(got, pairs):
        bank64.set_descriptors(0, sets[a])
        bank64.set_descriptors(1, sets[b])
        assert np.array_equal(bank64.match(**BANK_CONFIGS[k]), g), (BANK_CONFIGS[k], a, b)


@pytest.mark.parametrize("k", (3, 7, 0, 8))
def test_bank_chunk_at_the_segment_cap(bank64, k):
    """One chunk of 64 pairs of the three large sets: segments of up to 15 super tiles (tiles 0..59 of a segment); called
    twice, and one pair per call."""
    pairs = mc.bank_big_chunk_pairs()
    cfg = BANK_CONFIGS[k]
    whole = _check_pairs_against(bank64, pairs, k)
    again = bank64.match_pairs(pairs, **cfg)
    for j, p in enumerate(pairs):
        assert len(whole[j]) > 0
        assert np.array_equal(again[j], whole[j]), (cfg, tuple(p))
    for j in range(9):                       # (the chunk repeats nine distinct pairs)
        assert np.array_equal(bank64.match_pairs(pairs[j][None], **cfg)[0], whole[j]), (cfg, tuple(pairs[j]))


def test_bank_from_floats_and_from_device_memory():
    """The same bank as floats q / 512 on the host (quantise), as a device float tensor [sum n][64] (bank_build_kernel<true,
    64>) and as a device byte tensor (<false, 64>): byte-equal to the input, with equal matches."""
    import torch

    from hessgpu_amd.matcher import Matcher

    sets = mh.bank_sets()
    counts = [len(s) for s in sets]
    floats = [s.astype(np.float32) / np.float32(512.0) for s in sets]
    pairs = mc.bank_all_pairs()
    tf = torch.from_numpy(np.concatenate(floats)).to("cuda:0")
    tu = torch.from_numpy(np.concatenate(sets)).to("cuda:0")
    assert tuple(tf.shape) == (sum(counts), 64) and tuple(tu.shape) == (sum(counts), 64)
    torch.cuda.synchronize()
    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT, dim=64)
    for load in (lambda: m.set_bank(floats), lambda: m.set_bank_device(tf.data_ptr(), counts),
                 lambda: m.set_bank_device(tu.data_ptr(), counts, dtype=np.uint8)):
        load()
        for i, s in enumerate(sets):
            assert np.array_equal(m.bank(i), s), i
        for k in (3, 7, 0):
            _check_pairs_against(m, pairs, k)
    # the range check counts rows of 64 bytes: all the rows an allocation holds are taken, counts that reach 64 MiB past it
    # (further than any pool segment around a 3 MiB tensor) are refused and nothing is launched
    from hessgpu_amd import _abi
    from hessgpu_amd.session import HessError

    whole = torch.zeros((3 << 20,), dtype=torch.uint8, device="cuda:0")     # an allocation of its own
    torch.cuda.synchronize()
    rows = whole.numel() // 64
    m.set_bank_device(whole.data_ptr(), [rows], dtype=np.uint8)
    assert len(m.bank(0)) == mc.BANK_MAX_SIFT
    with pytest.raises(HessError) as e:
        m.set_bank_device(whole.data_ptr(), [rows + 1 + (1 << 20)], dtype=np.uint8)
    assert e.value.code == _abi.HESS_ERR_ARG
    m.close()


def test_a_128d_matcher_on_the_padded_sets_returns_the_same():
    """Equivalence inside the product: match_mfma_kernel<*, 128> / match_dot_kernel<128> on pad128 of the sets."""
    from hessgpu_amd.matcher import Matcher

    s1, s2 = mh.straddle_sets()
    m64 = Matcher(0, max_sift=4096, dim=64)
    m128 = Matcher(0, max_sift=4096)
    assert m64.dim == 64 and m128.dim == 128
    for a in (s1[:-1], s1):
        m64.set_descriptors(0, a)
        m64.set_descriptors(1, s2)
        m128.set_descriptors(0, mh.pad128(a))
        m128.set_descriptors(1, mh.pad128(s2))
        for dm, rm, mutual in mc.CONFIGS:
            kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=len(a))
            got = m64.match(**kw)
            assert len(got) > 0 and np.array_equal(got, m128.match(**kw)), (len(a), dm, rm, mutual)
    sets = mh.bank_sets()
    m64.set_bank(sets)
    m128.set_bank([mh.pad128(s) for s in sets])
    pairs = np.array([(8, 7), (6, 8), (5, 3)], np.int32)
    for cfg in BANK_CONFIGS[3], BANK_CONFIGS[0]:
        for x, y in zip(m64.match_pairs(pairs, **cfg), m128.match_pairs(pairs, **cfg)):
            assert len(x) > 0 and np.array_equal(x, y), cfg
    m64.close()
    m128.close()


# ---- guided -----------------------------------------------------------------------------------------------------------

def _load(m, c):
    m.set_descriptors(0, c.d1)
    m.set_descriptors(1, c.d2)
    m.set_locations(0, c.loc1)
    m.set_locations(1, c.loc2)


def _kw(h, f, dm, rm, mutual, max_match):
    return dict(hdistmax=h, fdistmax=f, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=max_match)


def _guided_ref(c, H, F, **kw):
    return oracle_match(mh.pad128(c.d1), mh.pad128(c.d2), c.loc1, c.loc2, H, F, **kw)


@pytest.mark.parametrize("n1,n2,geometry", gc.CASES)
def test_guided_match_equals_the_oracle(n1, n2, geometry):
    from hessgpu_amd.matcher import Matcher

    cs = (n1, n2, geometry)
    c = mh.guided_case(*cs)
    m = Matcher(0, max_sift=max(n1, n2), dim=64)
    _load(m, c)
    for k, (h, f) in enumerate(gc.pick_thresholds(*cs)):
        for dm, rm, mutual in gc.CONFIGS:
            ref = _guided_ref(c, c.H, c.F, **_kw(h, f, dm, rm, mutual, n1))
            assert (len(ref) == 0) == ((cs, k) in gc.EMPTY), (cs, h, f, dm, rm, mutual, len(ref))
            got = m.match(H=c.H, F=c.F, **_kw(h, f, dm, rm, mutual, n1))
            assert np.array_equal(got, ref), (cs, h, f, dm, rm, mutual, mc.first_difference(ref, got))
            cut = len(ref) // 2
            if cut:
                got = m.match(H=c.H, F=c.F, **_kw(h, f, dm, rm, mutual, cut))
                assert len(got) == cut and np.array_equal(got, ref[:cut]), (cs, h, f, dm, rm, mutual, cut)
    m.close()


def test_guided_and_unguided_calls_on_one_handle():
    """2049 x 2081: the unguided call runs on the matrix cores, the guided one on match_dot_kernel<64>; they share the slots."""
    from hessgpu_amd.matcher import Matcher

    cs = (2049, 2081, "affine")
    c = mh.guided_case(*cs)
    th = gc.pick_thresholds(*cs)
    m = Matcher(0, max_sift=2081, dim=64)
    _load(m, c)
    plain = dict(distmax=2.0, ratiomax=2.0, mutual_best=True, max_match=c.n1)
    plain_ref = _ref(c.d1, c.d2, **plain)
    for t in (None, th[0], None, th[3], None):
        if t is None:
            ref, got = plain_ref, m.match(**plain)
        else:
            kw = _kw(t[0], t[1], 2.0, 2.0, True, c.n1)
            ref, got = _guided_ref(c, c.H, c.F, **kw), m.match(H=c.H, F=c.F, **kw)
            assert not np.array_equal(ref, plain_ref)
        assert len(ref) > 0 and np.array_equal(got, ref), (t, mc.first_difference(ref, got))
    m.close()


# ---- hess_matcher_set_dim on one handle -------------------------------------------------------------------------------

def test_set_dim_on_one_handle():
    from hessgpu_amd import _abi
    from hessgpu_amd.matcher import Matcher
    from hessgpu_amd.session import HessError

    n1, n2 = mc.SMALL_PATH_SIZES[0]
    a128, b128 = mc.single_pair(n1, n2)
    a64, b64 = mh.single_pair(n1, n2)
    kw = dict(distmax=2.0, ratiomax=2.0, mutual_best=True, max_match=n1)
    ref128 = oracle_match(a128, b128, **kw)
    ref64 = _ref(a64, b64, **kw)
    assert len(ref128) > 0 and len(ref64) > 0 and not np.array_equal(ref128, ref64)
    pair = np.array([[0, 1]], np.int32)

    m = Matcher(0, max_sift=4096)
    L, h = m.L, m.h
    assert m.dim == 128 and L.hess_matcher_dim(h) == 128

    def load(a, b):
        m.set_descriptors(0, a)
        m.set_descriptors(1, b)
        m.set_bank([a, b])

    load(a128, b128)
    first = m.match(**kw)
    assert np.array_equal(first, ref128) and np.array_equal(m.match_pairs(pair, **kw)[0], ref128)
    # the current dim: a no-op, the sets stay
    m.set_dim(128)
    assert np.array_equal(m.match(**kw), ref128) and np.array_equal(m.bank(1), b128)
    # the other dim: the bank and both slots are empty
    m.set_dim(64)
    assert m.dim == 64 and L.hess_matcher_dim(h) == 64
    with pytest.raises(HessError) as e:
        m.match_pairs(pair, **kw)
    assert e.value.code == _abi.HESS_ERR_ARG
    out = np.zeros((n1, 2), np.int32)
    assert L.hess_matcher_match(h, n1, out.ctypes.data, None, None, 2.0, 2.0, 0.0, 0.0, 1) == 0
    assert len(m.match(**kw)) == 0
    with pytest.raises(ValueError):
        m.set_descriptors(0, a128)
    load(a64, b64)
    assert np.array_equal(m.match(**kw), ref64) and np.array_equal(m.match_pairs(pair, **kw)[0], ref64)
    assert np.array_equal(m.bank(0), a64)
    # back: empty again, then the first result again
    m.set_dim(128)
    assert m.dim == 128 and len(m.match(**kw)) == 0
    load(a128, b128)
    assert np.array_equal(m.match(**kw), first) and np.array_equal(m.match_pairs(pair, **kw)[0], first)
    # 96: refused by name, and the handle is as it was
    assert L.hess_matcher_set_dim(h, 96) == _abi.HESS_ERR_ARG
    assert b"96" in L.hess_matcher_last_error(h)
    with pytest.raises(HessError) as e:
        m.set_dim(96)
    assert e.value.code == _abi.HESS_ERR_ARG and "96" in str(e.value)
    assert m.dim == 128 and L.hess_matcher_dim(h) == 128
    assert np.array_equal(m.match(**kw), first) and np.array_equal(m.bank(1), b128)
    m.close()


# ---- the bank straight from a -half context ---------------------------------------------------------------------------

def test_matcher_bank_from_a_half_context(gpu_ctx_factory):
    from hessgpu_amd.matcher import Matcher

    imgs = np.stack([fixtures.load_rgb(f"640-{i}.jpg") for i in range(1, 6)])
    g = gpu_ctx_factory(half_sift=1)
    pairs = np.array([(a, b) for a in range(5) for b in range(5) if a != b], np.int32)
    assert len(pairs) == 20
    counts = g.run(imgs)
    assert g.desc_dim() == 64 and min(counts) > 100
    floats = [g.fetch(i)[1] for i in range(5)]
    assert all(d.shape == (n, 64) and np.isfinite(d).all() for d, n in zip(floats, counts))
    want = [oracle_quantize(d) for d in floats]
    cfgs = (dict(), dict(distmax=1.2, ratiomax=0.95))            # the defaults, and a looser pair
    got = {}
    for fmt in ("f32", "u8"):
        g.set_descriptor_format(fmt)
        assert g.run(imgs) == counts
        m = Matcher(0, max_sift=8192, dim=64)
        m.set_bank_from_session(g)
        got[fmt] = ([m.bank(i) for i in range(5)], [m.match_pairs(pairs, **cfg) for cfg in cfgs])
        m.close()
        with pytest.raises(ValueError):                              # a default matcher still refuses it
            Matcher(0).set_bank_from_session(g)
    for i in range(5):
        assert got["u8"][0][i].shape == (counts[i], 64)
        assert np.array_equal(got["u8"][0][i], want[i]) and np.array_equal(got["f32"][0][i], want[i]), i
    pads = [mh.pad128(b) for b in want]
    for k, cfg in enumerate(cfgs):
        with ThreadPoolExecutor(8) as ex:
            ref = list(ex.map(lambda p: oracle_match(pads[p[0]], pads[p[1]], **cfg), [tuple(p) for p in pairs]))
        assert sum(len(r) for r in ref) > 0, cfg                     # (several pairs of these images have no match)
        for j, p in enumerate(pairs):
            assert np.array_equal(got["u8"][1][k][j], ref[j]), (cfg, tuple(p), mc.first_difference(ref[j], got["u8"][1][k][j]))
            assert np.array_equal(got["f32"][1][k][j], ref[j]), (cfg, tuple(p))
    # a 128-d context on this matcher is refused
    full = gpu_ctx_factory()
    full.run(imgs[:1])
    m = Matcher(0, dim=64)
    with pytest.raises(ValueError) as e:
        m.set_bank_from_session(full)
    assert "64" in str(e.value) and "128" in str(e.value)
    m.close()


# ---- SiftMatchGPU "-half" through the C mirror --------------------------------------------------------------------------

def test_siftmatchgpu_half_through_the_c_mirror():
    import siftgpu_lib
    from hessgpu_amd.matcher import Matcher

    L = siftgpu_lib.lib()
    f32, vp, i32 = C.c_float, C.c_void_p, C.c_int
    for name, res, args in [("siftmatch_create", vp, [i32]), ("siftmatch_destroy", None, [vp]),
                            ("siftmatch_set_device_param", None, [vp, i32, C.POINTER(C.c_char_p)]),
                            ("siftmatch_set_descriptors_f32", None, [vp, i32, i32, vp]),
                            ("siftmatch_set_descriptors_u8", None, [vp, i32, i32, vp]),
                            ("siftmatch_get_match", i32, [vp, i32, vp, f32, f32, i32])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    n1, n2 = mc.SMALL_PATH_SIZES[0]
    a, b = mh.single_pair(n1, n2)
    fa, fb = (np.ascontiguousarray(d.astype(np.float32) / np.float32(512.0)) for d in (a, b))   # quantise back to the bytes
    m = Matcher(0, max_sift=1024, dim=64)
    m.set_descriptors(0, a)
    m.set_descriptors(1, b)
    argv = (C.c_char_p * 3)(b"-cuda", b"0", b"-half")            # one argv for SiftGPU::ParseParam and this call
    buf = np.zeros((n1, 2), np.int32)
    # siftmatch_create makes the matcher at once, so "-half" reaches one that exists; CreateNewSiftMatchGPU makes it at the
    # first SetDescriptors, after the parameter
    for use_u8, create in ((True, L.siftmatch_create), (False, L.CreateNewSiftMatchGPU)):
        hnd = create(1024)
        L.siftmatch_set_device_param(hnd, 3, argv)
        if use_u8:
            L.siftmatch_set_descriptors_u8(hnd, 0, n1, a.ctypes.data)
            L.siftmatch_set_descriptors_u8(hnd, 1, n2, b.ctypes.data)
        else:
            L.siftmatch_set_descriptors_f32(hnd, 0, n1, fa.ctypes.data)
            L.siftmatch_set_descriptors_f32(hnd, 1, n2, fb.ctypes.data)
        for dm, rm, mutual in ((0.7, 0.8, True), (2.0, 2.0, False)):
            ref = _ref(a, b, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
            n = L.siftmatch_get_match(hnd, n1, buf.ctypes.data, dm, rm, int(mutual))
            assert len(ref) > 0 and np.array_equal(buf[:n], ref), (use_u8, dm, rm, mutual, mc.first_difference(ref, buf[:n]))
            assert np.array_equal(m.match(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1), ref)
        L.siftmatch_destroy(hnd)
    m.close()
