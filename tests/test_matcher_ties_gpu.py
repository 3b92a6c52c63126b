"""The HIP matcher against the CPU oracle on inputs that MATCH (tests/matcher_cases.py; tests/test_matcher_cases.py checks
the inputs themselves on the CPU): descriptor-like sets with correspondences and exact ties placed on the tile, super tile,
segment, lane-half, wavefront and row-block boundaries of the matrix-core kernel.  Integer work: every comparison is exact,
and every one asserts first that the expected result is not empty.

With (distmax, ratiomax) = (2, 2), not mutual and max_match = n1 every row with a positive best score is returned: the
column chosen for every row is observed, ties included; the mutual run observes the row chosen for every such column."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import matcher_cases as mc
from oracle_lib import oracle_match

pytestmark = pytest.mark.gpu


def _check_single(m, a, b, label):
    """set 1 = a, set 2 = b through the single-pair entry point: every configuration, and a max_match below the count."""
    m.set_descriptors(0, a)
    m.set_descriptors(1, b)
    n1 = len(a)
    for dm, rm, mutual in mc.CONFIGS:
        ref = oracle_match(a, b, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
        assert len(ref) > 0, (label, dm, rm, mutual)
        got = m.match(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
        assert np.array_equal(got, ref), (label, dm, rm, mutual, mc.first_difference(ref, got))
        cut = len(ref) // 2
        if cut:
            got = m.match(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=cut)
            assert len(got) == cut and np.array_equal(got, ref[:cut]), (label, dm, rm, mutual, cut)


@pytest.mark.parametrize("n1,n2", mc.MATRIX_CORE_SIZES)
def test_single_pair_on_the_matrix_cores(n1, n2):
    """n1 * n2 > 3 Mi: match_mfma_kernel + match_finish_kernel.  matcher_cases.MATRIX_CORE_SIZES says what geometry each
    size yields."""
    from hessgpu_amd.matcher import Matcher

    a, b = mc.single_pair(n1, n2)
    m = Matcher(0, max_sift=max(n1, n2))
    _check_single(m, a, b, (n1, n2))
    m.close()


@pytest.mark.parametrize("n1,n2", mc.SMALL_PATH_SIZES)
def test_single_pair_under_the_threshold(n1, n2):
    """The same kind of input on match_dot_kernel / match_row_kernel / match_col_kernel."""
    from hessgpu_amd.matcher import Matcher

    a, b = mc.single_pair(n1, n2)
    m = Matcher(0, max_sift=4096)
    _check_single(m, a, b, (n1, n2))
    m.close()


def test_single_pair_straddling_the_threshold():
    """The same sets on both paths: 1536 x 2048 is the largest small-path problem, one row more runs on the matrix cores."""
    from hessgpu_amd.matcher import Matcher

    s1, s2 = mc.straddle_sets()
    m = Matcher(0, max_sift=4096)
    for a in (s1[:-1], s1):
        _check_single(m, a, s2, ("straddle", len(a)))
    m.close()


# ---- bank -----------------------------------------------------------------------------------------------------------

BANK_CONFIGS = [dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=mc.BANK_MAX_SIFT) for dm, rm, mutual in mc.CONFIGS]
BANK_CONFIGS += [dict(distmax=2.0, ratiomax=2.0, mutual_best=False, max_match=100),      # max_match below the match count
                 dict(distmax=0.7, ratiomax=0.8, mutual_best=True, max_match=100)]


def _oracle_all(bank, pairs, cfg):
    uniq = sorted({tuple(p) for p in pairs})
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
        res = dict(zip(uniq, ex.map(lambda p: oracle_match(bank[p[0]], bank[p[1]], **cfg), uniq)))
    return [res[tuple(p)] for p in pairs]


def _expect_matches(p, ref, cfg):
    """Every expected result is non-empty, but for the named exceptions: an empty side and the all-zero set."""
    if mc.BANK_SIZES.index(0) in p or mc.BANK_ZERO_SET in p:
        assert len(ref) == 0, (cfg, p)
    else:
        assert len(ref) > 0, (cfg, p)


def _check_bank(m, sets):
    """match_pairs == oracle == single-pair match, pair by pair, over all ordered pairs; then the chunk at the cap."""
    bank = [m.bank(i) for i in range(len(sets))]
    pairs = mc.bank_all_pairs()
    assert len(pairs) > mc.BANK_CHUNK
    for cfg in BANK_CONFIGS:
        got = m.match_pairs(pairs, **cfg)
        ref = _oracle_all(bank, pairs, cfg)
        for k, (a, b) in enumerate(pairs):
            _expect_matches((a, b), ref[k], cfg)
            assert np.array_equal(got[k], ref[k]), (cfg, a, b, mc.first_difference(ref[k], got[k]))
            m.set_descriptors(0, bank[a])
            m.set_descriptors(1, bank[b])
            assert np.array_equal(m.match(**cfg), ref[k]), (cfg, a, b)
        if cfg["max_match"] == 100:
            assert max(len(g) for g in got) == 100
    # one chunk of 64 pairs of the three large sets: segments of up to 15 super tiles (tiles 0..59 of a segment)
    pairs = mc.bank_big_chunk_pairs()
    for cfg in BANK_CONFIGS[3], BANK_CONFIGS[7], BANK_CONFIGS[0], BANK_CONFIGS[8]:
        whole = m.match_pairs(pairs, **cfg)
        again = m.match_pairs(pairs, **cfg)
        ref = _oracle_all(bank, pairs, cfg)
        for k, p in enumerate(pairs):
            assert len(ref[k]) > 0
            assert np.array_equal(whole[k], ref[k]), (cfg, tuple(p), mc.first_difference(ref[k], whole[k]))
            assert np.array_equal(again[k], whole[k]), (cfg, tuple(p))                       # a second call == the first
            assert np.array_equal(m.match_pairs(p[None], **cfg)[0], whole[k]), (cfg, tuple(p))   # one pair per call == the list


def test_bank_all_ordered_pairs_and_a_chunk_at_the_segment_cap():
    from hessgpu_amd.matcher import Matcher

    sets = mc.bank_sets()
    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT)
    m.set_bank(sets)
    for i, s in enumerate(sets):
        assert np.array_equal(m.bank(i), s)
    _check_bank(m, sets)
    m.close()


def test_bank_from_floats_on_the_host_and_on_the_device():
    """The same cases as floats q / 512 (which quantise back to q): set_bank with float input quantises on the host,
    set_bank_device on the device -- the quantisers' output is matched, not only read back."""
    import torch

    from hessgpu_amd.matcher import Matcher

    sets = mc.bank_sets()
    floats = [s.astype(np.float32) / np.float32(512.0) for s in sets]
    pairs = mc.bank_all_pairs()
    cfgs = BANK_CONFIGS[3], BANK_CONFIGS[7], BANK_CONFIGS[0]
    ref = [_oracle_all(sets, pairs, cfg) for cfg in cfgs]
    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT)
    t = torch.from_numpy(np.concatenate(floats)).to("cuda:0")
    torch.cuda.synchronize()
    for load in (lambda: m.set_bank(floats), lambda: m.set_bank_device(t.data_ptr(), [len(s) for s in sets])):
        load()
        for i, s in enumerate(sets):
            assert np.array_equal(m.bank(i), s), i
        for cfg, r in zip(cfgs, ref):
            got = m.match_pairs(pairs, **cfg)
            for k, (a, b) in enumerate(pairs):
                _expect_matches((a, b), r[k], cfg)
                assert np.array_equal(got[k], r[k]), (cfg, a, b, mc.first_difference(r[k], got[k]))
    m.close()


def test_matrix_core_path_is_the_same_every_time_on_inputs_that_match():
    """300 matches of each size, mutual best and not, every one equal to the first, which equals the oracle's and is not
    empty (test_matcher.py keeps the same test on full-range bytes, whose results are empty)."""
    from hessgpu_amd.matcher import Matcher

    for n1, n2 in ((2049, 2081), (300, 33000)):
        a, b = mc.single_pair(n1, n2)
        m = Matcher(0, max_sift=max(n1, n2))
        m.set_descriptors(0, a)
        m.set_descriptors(1, b)
        for dm, rm, mutual in ((0.7, 0.8, True), (2.0, 2.0, False)):
            kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=n1)
            first = m.match(**kw)
            ref = oracle_match(a, b, **kw)
            assert len(ref) > 0 and np.array_equal(first, ref), (n1, n2, mutual, mc.first_difference(ref, first))
            for k in range(300):
                assert np.array_equal(m.match(**kw), first), (n1, n2, mutual, k)
        m.close()
