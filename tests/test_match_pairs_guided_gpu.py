"""Guided matching for bank pairs on the GPU (hess_matcher_match_pairs_guided: match_mfma_kernel<GUIDED>) against the CPU oracle
and against the single-pair guided call (match_dot_kernel), on the banks of tests/guided_pair_cases.py, whose properties
tests/test_guided_pair_cases.py checks on the oracle alone.  Integer results: every comparison is exact."""
import numpy as np
import pytest

import guided_cases as gc
import guided_pair_cases as gp
import matcher_cases as mc
import matcher_cases_half as mh
from oracle_lib import oracle_match

pytestmark = pytest.mark.gpu


def _codes():
    from hessgpu_amd import _abi
    return _abi.HESS_ERR_ARG, _abi.HESS_ERR_STATE, _abi.HESS_ERR_UNSUPPORTED


def _oracle(d1, d2, loc1, loc2, H, F, h, f, dm, rm, mutual, max_match):
    return oracle_match(d1, d2, loc1, loc2, H, F, hdistmax=h, fdistmax=f, distmax=dm, ratiomax=rm, mutual_best=mutual,
                        max_match=max_match)


class _Single:
    """The single-pair guided call on one handle, its slots loaded only when the sets change."""

    def __init__(self, max_sift=4096, dim=128):
        from hessgpu_amd.matcher import Matcher
        self.m = Matcher(0, max_sift=max_sift, dim=dim)
        self.loaded = None

    def __call__(self, key, d1, d2, loc1, loc2, H, F, h, f, dm, rm, mutual, max_match):
        if self.loaded != key:
            self.m.set_descriptors(0, d1)
            self.m.set_descriptors(1, d2)
            self.m.set_locations(0, loc1)
            self.m.set_locations(1, loc2)
            self.loaded = key
        return self.m.match(H=H, F=F, hdistmax=float(h), fdistmax=float(f), distmax=dm, ratiomax=rm, mutual_best=mutual,
                            max_match=max_match)

    def close(self):
        self.m.close()


def _bank(sets, locs, max_sift=4096, dim=128):
    from hessgpu_amd.matcher import Matcher
    m = Matcher(0, max_sift=max_sift, dim=dim)
    m.set_bank(sets)
    m.set_bank_locations(locs)
    return m


def _same(got, ref, what):
    assert np.array_equal(got, ref), (what, len(got), len(ref), mc.first_difference(ref, got))


def test_bank_of_cases_equals_the_oracle_and_the_single_pair_call():
    """Every pair with its own H, F and thresholds in one call: the four threshold kinds x gc.CONFIGS, at full length and cut."""
    sets, locs, pairs, cases = gp.case_bank()
    m, single = _bank(sets, locs), _Single()
    n1max = max(cs[0] for cs in cases)
    differs = 0
    for k in range(len(gc.NOMINAL)):
        H, F, hd, fd = gp.geometry(cases, [k] * len(cases))
        for dm, rm, mutual in gc.CONFIGS:
            kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual)
            got = m.match_pairs_guided(pairs, H, F, hd, fd, max_match=n1max, **kw)
            plain = m.match_pairs(pairs, max_match=n1max, **kw)
            refs = []
            for p, cs in enumerate(cases):
                c = gc.case(*cs)
                ref = _oracle(c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, hd[p], fd[p], dm, rm, mutual, cs[0])
                assert (len(ref) == 0) == ((cs, k) in gc.EMPTY), (cs, k, dm, rm, mutual, len(ref))
                _same(got[p], ref, (cs, k, dm, rm, mutual, "oracle"))
                _same(got[p], single(cs, c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, hd[p], fd[p], dm, rm, mutual, cs[0]),
                      (cs, k, dm, rm, mutual, "single pair"))
                differs += not np.array_equal(got[p], plain[p])
                refs.append(ref)
            cut = max(len(r) for r in refs) // 2
            got = m.match_pairs_guided(pairs, H, F, hd, fd, max_match=cut, **kw)
            for p, cs in enumerate(cases):
                _same(got[p], refs[p][:cut], (cs, k, dm, rm, mutual, "cut", cut))
            assert any(len(r) > cut for r in refs)
    assert differs >= 2 * len(gc.NOMINAL) * len(gc.CONFIGS)      # at least the two 300 x 333 pairs, every time
    m.close()
    single.close()


@pytest.mark.parametrize("n1,n2,geometry", gp.SEAM_CASES)
def test_row_shifted_pair_keeps_the_block_rule_across_the_seams(n1, n2, geometry):
    """224 zero rows in front: the leak triples sit on the 256-row workgroup seam, the 64-row wavefront seam and the ragged
    last block; the expected result is the unshifted one plus (224, 0)."""
    c, s = gc.case(n1, n2, geometry), gp.shifted(n1, n2, geometry)
    m = _bank([s.d1, s.d2], [s.loc1, s.loc2])
    for k, (h, f) in enumerate(gc.pick_thresholds(n1, n2, geometry)):
        for dm, rm, mutual in gc.CONFIGS:
            ref = gp.shift_matches(_oracle(c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, h, f, dm, rm, mutual, n1))
            got, = m.match_pairs_guided([[0, 1]], s.H[None], s.F[None], h, f, max_match=s.n1, distmax=dm, ratiomax=rm,
                                        mutual_best=mutual)
            _same(got, ref, (k, dm, rm, mutual))
            if k == 0 and (dm, rm) == (2.0, 2.0):
                for name, i, ip, ipp, j in s.triples:
                    assert [ip, j] in got.tolist() and ipp not in got[:, 0].tolist(), (name, mutual)
    m.close()


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("n1,n2,geometry", gp.SEAM_CASES)
def test_trailing_row_trap(n1, n2, geometry, last):
    """A ragged last block whose padded rows must read no location: neither the next set's (which would pass and leak
    (289, column)) nor, with the set last in the bank, anything past the end."""
    t = gp.trap(n1, n2, geometry)
    if last:
        sets, locs, pair = [t.d2, t.follower[0], t.d1], [t.loc2, t.follower[1], t.loc1], [[2, 0]]
    else:
        sets, locs, pair = [t.d1, t.follower[0], t.d2], [t.loc1, t.follower[1], t.loc2], [[0, 2]]
    m = _bank(sets, locs)
    for k in (0, 2):
        h, f = gc.pick_thresholds(n1, n2, geometry)[k]
        for mutual in (True, False):
            ref = _oracle(t.d1, t.d2, t.loc1, t.loc2, t.H, t.F, h, f, 2.0, 2.0, mutual, t.n1)
            got, = m.match_pairs_guided(pair, t.H[None], t.F[None], h, f, max_match=t.n1, distmax=2.0, ratiomax=2.0,
                                        mutual_best=mutual)
            assert [t.ipp, t.j] not in got.tolist(), (k, mutual)
            _same(got, ref, (k, mutual))
    m.close()


def test_large_pair():
    """2049 x 2081: 9 row blocks, 17 super tiles, more than one segment."""
    cs = (2049, 2081, "affine")
    c = gc.case(*cs)
    m, single = _bank([c.d1, c.d2], [c.loc1, c.loc2]), _Single()
    th = gc.pick_thresholds(*cs)
    for k in (0, 3):
        h, f = th[k]
        for mutual in (True, False):
            ref = _oracle(c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, h, f, 2.0, 2.0, mutual, cs[0])
            got, = m.match_pairs_guided([[0, 1]], c.H[None], c.F[None], h, f, max_match=cs[0], distmax=2.0, ratiomax=2.0,
                                        mutual_best=mutual)
            assert len(ref)
            _same(got, ref, (k, mutual, "oracle"))
            _same(got, single(cs, c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, h, f, 2.0, 2.0, mutual, cs[0]), (k, mutual, "single pair"))
    m.close()
    single.close()


def test_more_than_one_chunk_with_repeated_reversed_and_self_pairs():
    """72 pairs over the four small cases: the geometry belongs to the position, not to (a, b)."""
    sets, locs, _, cases = gp.case_bank(gp.BANK_CASES[:4])
    m, single = _bank(sets, locs), _Single()
    entries = []                                       # (a, b, case whose geometry is used, threshold entry)
    for pos in range(70):
        q = pos % 4
        entries.append((2 * q, 2 * q + 1, q, (pos // 4 + pos) % 4))
    entries.append((5, 4, 2, 0))                       # reversed
    entries.append((6, 6, 3, 2))                       # (a, a)
    assert len(entries) > 64 and len({e[:2] for e in entries}) < len({(e[0], e[1], e[3]) for e in entries})
    pairs = np.array([e[:2] for e in entries], np.int32)
    H, F, hd, fd = gp.geometry([cases[e[2]] for e in entries], [e[3] for e in entries])
    for dm, rm, mutual in gc.CONFIGS[:2]:
        got = m.match_pairs_guided(pairs, H, F, hd, fd, max_match=129, distmax=dm, ratiomax=rm, mutual_best=mutual)
        memo = {}
        for p, (a, b, q, k) in enumerate(entries):
            if (a, b, q, k) not in memo:
                memo[(a, b, q, k)] = single((a, b), sets[a], sets[b], locs[a], locs[b], H[p], F[p], hd[p], fd[p], dm, rm, mutual, 129)
            _same(got[p], memo[(a, b, q, k)], (p, a, b, q, k, mutual))
        assert sum(len(g) for g in got) > 70
    m.close()
    single.close()


def test_64d_equals_the_single_pair_call_at_64d():
    cs = (300, 333, "affine")
    c = mh.guided_case(*cs)
    m, single = _bank([c.d1, c.d2], [c.loc1, c.loc2], dim=64), _Single(dim=64)
    total = 0
    for k, (h, f) in enumerate(gc.pick_thresholds(*cs)):
        for dm, rm, mutual in gc.CONFIGS:
            got, = m.match_pairs_guided([[0, 1]], c.H[None], c.F[None], h, f, max_match=cs[0], distmax=dm, ratiomax=rm,
                                        mutual_best=mutual)
            _same(got, single(cs, c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, h, f, dm, rm, mutual, cs[0]), (k, dm, rm, mutual))
            total += len(got)
    assert total
    m.close()
    single.close()


def test_states_errors_and_repeats():
    from hessgpu_amd.matcher import Matcher
    from hessgpu_amd.session import HessError

    ARG, STATE, UNSUPPORTED = _codes()
    sets, locs, pairs, cases = gp.case_bank(gp.BANK_CASES[:4])
    H, F, hd, fd = gp.geometry(cases, [0, 2, 0, 2])
    kw = dict(max_match=129, distmax=2.0, ratiomax=2.0, mutual_best=True)
    m = Matcher(0)
    m.set_bank(sets)
    before = m.match_pairs(pairs, **kw)

    def refused(code, call):
        with pytest.raises(HessError) as e:
            call()
        assert e.value.code == code, e.value
        after = m.match_pairs(pairs, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        return str(e.value)

    assert "locations" in refused(STATE, lambda: m.match_pairs_guided(pairs, H, F, hd, fd, **kw))
    m.set_bank_locations(locs)
    m.set_bank_types([np.arange(len(s)) % 3 for s in sets])
    typed = m.match_pairs(pairs, **kw)
    with pytest.raises(HessError) as e:
        m.match_pairs_guided(pairs, H, F, hd, fd, **kw)
    assert e.value.code == UNSUPPORTED and "types" in str(e.value)
    assert all(np.array_equal(x, y) for x, y in zip(typed, m.match_pairs(pairs, **kw)))
    m.set_bank_types(None)
    bad = pairs.copy()
    bad[2, 1] = len(sets)
    assert "pair 2" in refused(ARG, lambda: m.match_pairs_guided(bad, H, F, hd, fd, **kw))
    out, cnt = np.zeros((4, 129, 2), np.int32), np.zeros(4, np.int32)
    rc = m.L.hess_matcher_match_pairs_guided(m.h, 4, pairs.ctypes.data, None, 129, out.ctypes.data, cnt.ctypes.data, 2.0, 2.0, 1)
    assert rc == ARG and b"geo" in m.L.hess_matcher_last_error(m.h)

    good = m.match_pairs_guided(pairs, H, F, hd, fd, **kw)
    assert all(len(g) for g in good[1:])
    for name in ("H", "F"):                            # a zero matrix in the middle of the list
        Z = {"H": H.copy(), "F": F.copy()}
        Z[name][2] = 0
        off = np.float32(gc.OFF)
        got = m.match_pairs_guided(pairs, Z["H"], Z["F"], np.where(np.arange(4) == 2, off, hd), np.where(np.arange(4) == 2, off, fd), **kw)
        assert len(got[2]) == 0 and all(np.array_equal(got[p], good[p]) for p in (0, 1, 3)), name
    Z = H.copy()
    Z[1, 0, 0] = np.inf                                # a non-finite matrix: no match either
    got = m.match_pairs_guided(pairs, Z, F, hd, fd, **kw)
    assert len(got[1]) == 0 and all(np.array_equal(got[p], good[p]) for p in (0, 2, 3))

    first = [g.tobytes() for g in good]
    for _ in range(20):
        assert [g.tobytes() for g in m.match_pairs_guided(pairs, H, F, hd, fd, **kw)] == first

    m.set_bank(sets)                                   # loading the bank again drops the locations
    assert "locations" in refused(STATE, lambda: m.match_pairs_guided(pairs, H, F, hd, fd, **kw))
    m.close()


def _located_bank(nsets, n, seed, size=4096.0):
    """A bank whose pairs fit a homography, made like tools/bench_estimate.py's make_bank."""
    rng = np.random.RandomState(seed)
    pool = (rng.rand(4 * n, 128) * 78).astype(np.int32)
    ref = rng.rand(4 * n, 2) * size
    sets, locs = [], []
    for _ in range(nsets):
        idx = rng.choice(len(pool), n, replace=False)
        sets.append(np.clip(pool[idx] + rng.randint(-4, 5, (n, 128)), 0, 255).astype(np.uint8))
        Hm = np.eye(3) + np.array([[0.1, 0.1, 40.0], [0.1, 0.1, 40.0], [1e-5, 1e-5, 0.0]]) * (rng.rand(3, 3) * 2 - 1)
        x = np.concatenate([ref[idx], np.ones((n, 1))], 1) @ Hm.T
        locs.append((x[:, :2] / x[:, 2:]).astype(np.float32))
    return sets, locs


def test_pipeline_match_estimate_guided_match():
    from hessgpu_amd.matcher import all_pairs

    n, bound = 512, 8.0
    sets, locs = _located_bank(4, n, seed=4)
    m, single = _bank(sets, locs, max_sift=n), _Single(max_sift=n)
    pairs = all_pairs(4)
    matches = m.match_pairs(pairs, max_match=n)
    est = m.estimate_pairs(pairs, matches, "H", bound, seed=1, refit=1)
    Ms = np.stack([e[0] for e in est])
    assert all(e[2] >= 0 for e in est)
    got = m.match_pairs_guided(pairs, H=Ms, hdistmax=bound, max_match=n)
    eye = np.eye(3, dtype=np.float32)
    for p, (a, b) in enumerate(pairs.tolist()):
        assert len(got[p])
        ref = single((a, b), sets[a], sets[b], locs[a], locs[b], Ms[p], eye, bound, gc.OFF, 0.7, 0.8, True, n)
        _same(got[p], ref, (a, b))
    m.close()
    single.close()
