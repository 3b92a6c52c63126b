"""The 64-d matcher tests' inputs, checked on the CPU (tests/matcher_cases_half.py), and the ABI of the 64-d matcher
without a GPU.

Inputs.  The cases of matcher_cases.py and guided_cases.py folded to 64 columns must still be cases: norms under the clamp,
ties still ties, every expected result non-empty where the 128-d one is.  The expectation of every GPU test is
oracle_match(pad128(a), pad128(b)): the oracle is untouched and knows nothing of 64-d.  These input tests pass with and
without the 64-d matcher -- they say that a GPU test that compares with the oracle on these inputs compares something.

ABI.  hess_matcher_set_dim / hess_matcher_dim are declared and exported, refuse NULL, the version stays 5, and the Python
wrapper checks shapes and lengths before it calls the library.  These need the feature."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import guided_cases as gc
import matcher_cases as mc
import matcher_cases_half as mh
from oracle_lib import oracle_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_sets():
    out = []
    for n1, n2 in mc.MATRIX_CORE_SIZES + mc.SMALL_PATH_SIZES:
        out += [(mc.single_pair(n1, n2)[k], mh.single_pair(n1, n2)[k], (n1, n2, k)) for k in (0, 1)]
    out += [(s, h, ("straddle", k)) for k, (s, h) in enumerate(zip(mc.straddle_sets(), mh.straddle_sets()))]
    out += [(s, h, ("bank", k)) for k, (s, h) in enumerate(zip(mc.bank_sets(), mh.bank_sets()))]
    return out


def test_fold_and_pad():
    s = np.zeros((3, 128), np.uint8)
    s[0, 0], s[0, 1] = 3, 4                  # hypot 5
    s[1, 2], s[1, 3] = 255, 255              # hypot 360.6: saturates
    s[2, 126], s[2, 127] = 1, 1              # hypot 1.41: floored
    h = mh.fold(s)
    assert h.shape == (3, 64) and h.dtype == np.uint8
    assert h[0, 0] == 5 and h[1, 1] == 255 and h[2, 63] == 1 and int(h.sum()) == 261
    p = mh.pad128(h)
    assert p.shape == (3, 128) and p.flags.c_contiguous and np.array_equal(p[:, :64], h) and not p[:, 64:].any()
    # zero columns leave every dot product as it is
    a, b = mh.single_pair(1000, 877)
    d64 = a.astype(np.int64) @ b.astype(np.int64).T
    assert np.array_equal(d64, mh.pad128(a).astype(np.int64) @ mh.pad128(b).astype(np.int64).T)


def test_folded_norms_stay_below_the_clamp_and_ties_stay_ties():
    """fold only lowers a row's norm (floor of a 2-norm of two components): every dot product stays under 2^18.  Equal rows
    stay equal and the number of distinct rows does not change, so every placed tie is a tie of the folded sets."""
    largest = 0.0
    for s, h, label in _all_sets():
        if not len(s):
            continue
        assert (mh.norms(h) <= mh.norms(s) + 1e-9).all(), label
        largest = max(largest, float(mh.norms(h).max()))
        assert mh.distinct_rows(h) == mh.distinct_rows(s), label
        assert np.array_equal(~h.any(1), ~s.any(1)), label          # the all-zero rows, and only they
    print(f"largest folded row norm {largest:.1f}")
    assert largest < 512.0
    a, b = mc.single_pair(2049, 2081)
    assert mh.distinct_rows(a) == mh.distinct_rows(mh.single_pair(2049, 2081)[0]) == 2034
    for n, sps in ((2049, (1,)), (3825, (1, 2, 6, mc.MAX_SPS))):
        s = mh.single_pair(2049, 2081)[0] if n == 2049 else mh.bank_sets()[mc.BANK_SIZES.index(3825)]
        for name, pos in mc.tie_groups(n, sps).items():
            assert all(np.array_equal(s[pos[0]], s[p]) for p in pos[1:]), (n, name)


def _padded(a, b, dm, rm, mutual, max_match):
    return oracle_match(mh.pad128(a), mh.pad128(b), distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=max_match)


def test_single_pairs_still_match():
    want = {(2049, 2081): 1327, (255, 12337): 167, (257, 12289): 170, (12001, 263): 172, (300, 33000): 191}
    for n1, n2 in mc.MATRIX_CORE_SIZES + mc.SMALL_PATH_SIZES:
        a, b = mh.single_pair(n1, n2)
        for dm, rm, mutual in mc.CONFIGS:
            n = len(_padded(a, b, dm, rm, mutual, n1))
            assert n > 0, (n1, n2, dm, rm, mutual)
            if (dm, rm, mutual) == (0.7, 0.8, True) and (n1, n2) in want:
                assert n == want[n1, n2], (n1, n2, n)
    s1, s2 = mh.straddle_sets()
    for a in (s1[:-1], s1):
        for dm, rm, mutual in mc.CONFIGS:
            assert len(_padded(a, s2, dm, rm, mutual, len(a))) > 0, ("straddle", len(a), dm, rm, mutual)


def test_bank_pairs_still_match():
    """Every ordered pair, every configuration: non-empty, but for the empty set and the all-zero set."""
    sets = mh.bank_sets()
    pads = [mh.pad128(s) for s in sets]
    assert [len(s) for s in sets] == list(mc.BANK_SIZES) + [300] and not sets[mc.BANK_ZERO_SET].any()
    pairs = [tuple(p) for p in mc.bank_all_pairs()]
    for dm, rm, mutual in mc.CONFIGS:
        with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
            res = list(ex.map(lambda p: oracle_match(pads[p[0]], pads[p[1]], distmax=dm, ratiomax=rm, mutual_best=mutual,
                                                     max_match=mc.BANK_MAX_SIFT), pairs))
        for (a, b), r in zip(pairs, res):
            empty = mc.BANK_SIZES.index(0) in (a, b) or mc.BANK_ZERO_SET in (a, b)
            assert (len(r) == 0) == empty, (dm, rm, mutual, a, b, len(r))


@pytest.mark.parametrize("n1,n2,geometry", gc.CASES)
def test_guided_cases_still_match(n1, n2, geometry):
    """Folded descriptors with the case's own locations, H and F: empty exactly where guided_cases.EMPTY says the 128-d case
    is, and not the unguided result (but for the 1 x 1 case).  The gates do not look at descriptors, so nothing about their
    float32 certainty changes; the placed over-clamp rows (norm 700) stay over the clamp: their folded self-product is
    still above 2^18."""
    cs = (n1, n2, geometry)
    c = mh.guided_case(*cs)
    p1, p2 = mh.pad128(c.d1), mh.pad128(c.d2)
    for _, i, ip, ipp, j in c.triples:
        assert int(c.d1[ip].astype(np.int64) @ c.d2[j].astype(np.int64)) > mc.CLAMP
    for k, (h, f) in enumerate(gc.pick_thresholds(*cs)):
        for dm, rm, mutual in gc.CONFIGS:
            kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
            ref = oracle_match(p1, p2, c.loc1, c.loc2, c.H, c.F, hdistmax=h, fdistmax=f, **kw)
            assert (len(ref) == 0) == ((cs, k) in gc.EMPTY), (cs, k, dm, rm, mutual, len(ref))
            if (n1, n2) != (1, 1):
                assert not np.array_equal(ref, oracle_match(p1, p2, **kw)), (cs, k, dm, rm, mutual, "== unguided")


# ---- the ABI without a GPU --------------------------------------------------------------------------------------------

NEW = ["hess_matcher_set_dim", "hess_matcher_dim"]


def test_header_declares_and_library_exports_the_dim_calls():
    import hessgpu_amd
    from hessgpu_amd import _abi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hess_abi.h")).read(), flags=re.S)
    lib = hessgpu_amd.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*hess_matcher\s*\*", text), name
        assert hasattr(lib, name), name
        assert name[len("hess_"):] in _abi.PRODUCT_PROTOTYPES
    assert _abi.HESS_ABI_VERSION == 5
    assert re.search(r"#define\s+HESS_ABI_VERSION\s+5\b", text)
    sift = open(os.path.join(ROOT, "include", "SiftGPU.h")).read()
    for name in ("siftmatch_set_device_param", "siftmatch_set_descriptors_u8"):
        assert re.search(r"\bvoid\s+" + name + r"\s*\(\s*SiftMatchGPU\s*\*", sift), name


def test_null_matcher_is_refused_by_the_dim_calls():
    from hessgpu_amd import _abi
    from hessgpu_amd import matcher as hm

    L = hm._lib()
    for dim in (64, 128, 96):
        assert L.hess_matcher_set_dim(None, dim) == _abi.HESS_ERR_ARG
    assert L.hess_matcher_dim(None) == _abi.HESS_ERR_ARG


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for descriptors of the wrong length")


class _Session:
    """What set_bank_from_session reads of a context before it touches the device."""

    def __init__(self, dim):
        self._dim = dim

    def desc_dim(self):
        return self._dim

    def __getattr__(self, name):
        raise AssertionError(f"the context was asked for {name} although its descriptor length is refused")


def _matcher_without_library(dim):
    from hessgpu_amd import matcher as hm

    m = hm.Matcher.__new__(hm.Matcher)            # no device needed: the checks come first
    m.L, m.h, m._dim = _NoLibrary(), None, dim
    return m


@pytest.mark.parametrize("dim,other", [(64, 128), (128, 64)])
def test_wrong_second_axis_is_rejected_before_the_library(dim, other):
    m = _matcher_without_library(dim)
    assert m.dim == dim
    for dt in (np.uint8, np.float32):
        bad = np.zeros((5, other), dt)
        with pytest.raises(ValueError):
            m.set_descriptors(0, bad)
        with pytest.raises(ValueError):
            m.set_bank([np.zeros((2, dim), dt), bad])
    with pytest.raises(ValueError) as e:
        m.set_bank_from_session(_Session(other))
    assert str(dim) in str(e.value) and str(other) in str(e.value)
    with pytest.raises(ValueError):               # -sd: no descriptors at all
        m.set_bank_from_session(_Session(0))


def test_matcher_dim_argument_is_checked_before_the_library():
    from hessgpu_amd import matcher as hm

    real = hm._lib
    hm._lib = lambda: _NoLibrary()
    try:
        for dim in (0, 32, 96, 256):
            with pytest.raises(ValueError):
                hm.Matcher(0, dim=dim)
    finally:
        hm._lib = real
