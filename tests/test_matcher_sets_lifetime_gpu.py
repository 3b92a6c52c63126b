"""The life of a matcher's descriptor sets: a bank loaded in each of its four forms, typed, re-typed, located, both single-pair
slots filled, the descriptor length changed and changed back, every pair-list entry point run -- then close(), twelve times in
one process.  Every cycle must give the first cycle's bytes, bank(i) must return the caller's rows in every state, device memory
must not grow from cycle to cycle or from load to load of a live matcher, and a setter that refuses its arguments must leave
the sets as they were.  Only argument and state refusals are tried: no HIP call is made to fail.

The bank: six sets of 300, 0, 1, 255, 256 and 257 rows (the empty set, one row, the 256-row padding from both sides) under
max_sift = 280, so that the FIRST set is cut and every later set's types and locations lie behind rows that were counted but not
kept.  Sets 0, 2 and 4 are the first rows of set 1 of verify_cases.pair_sets("H 300"), sets 3 and 5 those of its set 2, with the
case's locations: pairs across the two sides carry the planted homography, which is what the guided gate and the estimator see.
Float forms are bytes / 512, which the quantisation returns exactly."""
import numpy as np
import pytest

import geom_cases as gcs
import matcher_cases as mc
import matcher_cases_half as mh
import matcher_type_cases as tc
import verify_cases as vc

pytestmark = pytest.mark.gpu

COUNTS = (300, 0, 1, 255, 256, 257)
SIDE = (0, 0, 0, 1, 0, 1)                       # which set of the case a bank set's rows come from
MAX_SIFT = 280
KEPT = tuple(min(n, MAX_SIFT) for n in COUNTS)
PAIRS = np.array([(0, 5), (4, 3), (4, 5), (0, 3), (2, 5), (1, 0), (0, 1), (5, 5), (3, 4)], np.int32)
CASE = "H 300"
TYPE_STRIDE, LOC_HOST_STRIDE, LOC_DEV_STRIDE = 6, 16, 12     # bytes between records: all larger than the packed 2 and 8
# The last bank of a matcher's life: set 0 so many times.  The six sets above are a few hundred KiB on the device, less than one
# 2 MiB step of torch.cuda.mem_get_info, so that alone the footprint can read 0 in a process whose earlier allocations left
# room in a step; 256 sets of 280 kept rows are 16 MiB (8 MiB at 64-d) of padded rows before types and locations.
WIDE = 256
WIDE_PAIRS = np.array([(0, 1), (WIDE - 1, 3), (7, 7)], np.int32)


class Bank:
    """The inputs of one descriptor length, in every form a setter takes."""

    def __init__(self, dim):
        import torch
        d1, d2, l1, l2 = vc.pair_sets(CASE)
        full = [(d1, d2)[s][:n] for s, n in zip(SIDE, COUNTS)]
        self.dim = dim
        self.sets = [mh.fold(s) if dim == 64 else s for s in full]
        self.kept = [s[:k] for s, k in zip(self.sets, KEPT)]
        self.locs = [(l1, l2)[s][:n] for s, n in zip(SIDE, COUNTS)]
        self.counts = np.array(COUNTS, np.int32)
        flat = np.ascontiguousarray(np.concatenate(self.sets))
        self.floats = [s.astype(np.float32) / 512 for s in self.sets]
        self.types = {k: tc.types_for(self.sets, kind) for k, kind in (("a", "random"), ("b", "position"))}
        self.kept_types = {k: [t[:n] for t, n in zip(v, KEPT)] for k, v in self.types.items()}
        # strided records: the value first, then filler that a wrong stride would read
        n = len(flat)
        loc = np.full((n, 4), -7.0, np.float32)
        loc[:, :2] = np.concatenate(self.locs)
        self.loc_host = loc
        typ = np.full((n, 3), 0x5555, np.uint16)
        typ[:, 0] = np.concatenate(self.types["a"])
        self.dev = dict(u8=torch.from_numpy(flat).to("cuda:0"),
                        f32=torch.from_numpy(np.concatenate(self.floats)).to("cuda:0"),
                        types=torch.from_numpy(typ.view(np.int16)).to("cuda:0"),
                        loc=torch.from_numpy(np.ascontiguousarray(loc[:, :3])).to("cuda:0"))
        torch.cuda.synchronize()
        assert typ.strides[0] == TYPE_STRIDE and loc.strides[0] == LOC_HOST_STRIDE and self.dev["loc"].stride(0) * 4 == LOC_DEV_STRIDE
        self.wide = {"sets": [self.sets[0]] * WIDE, "types": [self.types["a"][0]] * WIDE, "locs": [self.locs[0]] * WIDE}
        self.H = np.broadcast_to(gcs.case(CASE).truth.astype(np.float32), (len(PAIRS), 3, 3))

    def load(self, m, form):
        if form == "host u8":
            m.set_bank(self.sets)
        elif form == "host f32":
            m.set_bank(self.floats)
        else:
            m.set_bank_device(self.dev[form[7:]].data_ptr(), self.counts, dtype=np.uint8 if form == "device u8" else np.float32)

    def locations_host(self, m):
        m._check(m.L.hess_matcher_bank_set_locations(m.h, self.loc_host.ctypes.data, LOC_HOST_STRIDE))

    def rows_are_the_callers(self, m, state):
        for i, want in enumerate(self.kept):
            assert np.array_equal(m.bank(i), want), (state, i)


@pytest.fixture(scope="module", params=[128, 64])
def bank(request):
    return Bank(request.param)


def _used():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def _blob(lists):
    return b"".join(np.int32(len(a)).tobytes() + np.ascontiguousarray(a).tobytes() for a in lists)


def _pairs(m):
    return _blob(m.match_pairs(PAIRS, max_match=MAX_SIFT))


def _guided(m, b):
    return _blob(m.match_pairs_guided(PAIRS, H=b.H, hdistmax=8.0, max_match=MAX_SIFT))


def _verify(m):
    from hessgpu_amd.matcher import Matcher
    P = Matcher._verify_params("H", gcs.BOUND["H"], 128, 11, 1, None, True, vc.DISTMAX, vc.RATIOMAX, True)
    out, cnt, res, mask, put = m.verify_pairs_raw(PAIRS, P, MAX_SIFT, inlier=True, putative=True)
    return cnt.tobytes() + res.tobytes() + mask.tobytes() + _blob([out[p, :cnt[p]] for p in range(len(cnt))]) + \
        _blob([put[p, :res["nputative"][p]] for p in range(len(cnt))])


def _refused(code, word, call):
    from hessgpu_amd import HessError
    with pytest.raises(HessError) as e:
        call()
    assert e.value.code == code and word in str(e.value), (code, word, str(e.value))


def _cycle(b, other):
    """One matcher's whole life -> (named results, device bytes it held just before its close())."""
    from hessgpu_amd.matcher import Matcher
    m = Matcher(0, max_sift=MAX_SIFT, dim=b.dim)
    out = {}
    # the bank in its four forms; between them types and locations, which every new bank must end
    b.load(m, "host u8")
    b.rows_are_the_callers(m, "host u8")
    out["plain"] = _pairs(m)
    m.set_bank_types(b.types["a"])
    b.rows_are_the_callers(m, "types a, host")
    out["types a"] = _pairs(m)
    b.load(m, "host f32")                                         # (cnt holds the caller's 300, not the kept 280)
    b.rows_are_the_callers(m, "host f32")
    assert _pairs(m) == out["plain"], "a new bank kept the old one's types"
    m.set_bank_types_device(b.dev["types"].data_ptr(), TYPE_STRIDE)
    b.rows_are_the_callers(m, "types a, device")
    assert _pairs(m) == out["types a"], "types from device records differ from the host form's"
    m.set_bank_types(b.types["b"])                                # typed -> typed: the rows move from the grouped storage
    b.rows_are_the_callers(m, "types b")
    out["types b"] = _pairs(m)
    _refused(-6, "feature types", lambda: _guided(m, b))
    m.set_bank_types(None)
    b.rows_are_the_callers(m, "types off")
    assert _pairs(m) == out["plain"]
    _refused(-5, "no locations", lambda: _guided(m, b))
    b.locations_host(m)
    out["guided"] = _guided(m, b)
    out["verify"] = _verify(m)
    b.load(m, "device f32")
    b.rows_are_the_callers(m, "device f32")
    _refused(-5, "no locations", lambda: _guided(m, b))          # a new bank ends the locations
    assert _pairs(m) == out["plain"]
    m.set_bank_locations_device(b.dev["loc"].data_ptr(), LOC_DEV_STRIDE)
    assert _guided(m, b) == out["guided"], "locations from device records differ from the host form's"
    m.set_bank_types(b.types["a"])                                # types do not move the locations
    m.set_bank_types(None)
    assert _guided(m, b) == out["guided"] and _verify(m) == out["verify"]
    m.set_bank_locations(None)
    _refused(-5, "no locations", lambda: _verify(m))
    b.load(m, "device u8")
    b.rows_are_the_callers(m, "device u8")
    assert _pairs(m) == out["plain"]
    # both slots: descriptors (set 0 is cut to max_sift), types, locations with a gap
    i, j = 0, 5
    m.set_descriptors(0, b.sets[i])
    m.set_descriptors(1, b.floats[j])
    out["single"] = m.match(max_match=MAX_SIFT).tobytes()
    m.set_types(0, b.kept_types["a"][i])
    m.set_types(1, b.types["a"][j])
    out["single typed"] = m.match(max_match=MAX_SIFT).tobytes()
    m.set_types(0, None)
    m.set_types(1, None)
    assert m.match(max_match=MAX_SIFT).tobytes() == out["single"]
    H = b.H[0]
    eye = np.eye(3, dtype=np.float32)
    assert len(m.match(max_match=MAX_SIFT, H=H, F=eye, fdistmax=1e20)) == 0        # no locations yet: SiftMatchCU.cpp:131
    for k, s in ((0, i), (1, j)):
        m.set_locations(k, np.zeros((COUNTS[s], 2), np.float32))
        m.set_locations(k, b.loc_host[sum(COUNTS[:s]):sum(COUNTS[:s + 1])], gap=2)  # (replaces the zeros)
    out["single guided"] = m.match(max_match=MAX_SIFT, H=H, F=eye, hdistmax=8.0, fdistmax=1e20).tobytes()
    m.set_descriptors(1, b.sets[j])                               # new descriptors end the slot's locations
    assert len(m.match(max_match=MAX_SIFT, H=H, F=eye, fdistmax=1e20)) == 0
    # the other descriptor length and back: everything is emptied both times
    m.set_dim(other.dim)
    _refused(-1, "outside the bank", lambda: _pairs(m))
    other.load(m, "host u8")
    other.rows_are_the_callers(m, "other dim")
    out["other dim"] = _pairs(m)
    m.set_dim(b.dim)
    _refused(-5, "bank_set_types", lambda: m.set_bank_types(b.types["a"]))
    b.load(m, "host f32")
    assert _pairs(m) == out["plain"]
    b.locations_host(m)
    m.set_bank_types(b.types["b"])
    # the wide bank, typed and located: what the matcher holds when its footprint is read
    m.set_bank(b.wide["sets"])
    m.set_bank_types(b.wide["types"])
    m.set_bank_locations(b.wide["locs"])
    assert np.array_equal(m.bank(WIDE - 1), b.kept[0])
    out["wide"] = _blob(m.match_pairs(WIDE_PAIRS, max_match=MAX_SIFT))
    before = _used()
    m.close()
    return out, before - _used()


@pytest.fixture(scope="module")
def other(bank):
    return Bank(64 if bank.dim == 128 else 128)


@pytest.fixture(scope="module")
def first_cycle(bank, other):
    return _cycle(bank, other)[0]


def test_first_cycle_is_what_the_models_say(bank, first_cycle):
    """The bytes the other tests compare with are not trivially equal: the pairs across the case's sides match, types change
    the answer, the guided and verified lists are not empty, and plain and typed lists are the NumPy model's."""
    from hessgpu_amd.matcher import Matcher
    m = Matcher(0, max_sift=MAX_SIFT, dim=bank.dim)
    bank.load(m, "host u8")
    plain = m.match_pairs(PAIRS, max_match=MAX_SIFT)
    assert _blob(plain) == first_cycle["plain"]
    m.set_bank_types(bank.types["a"])
    typed = m.match_pairs(PAIRS, max_match=MAX_SIFT)
    m.close()
    for q, (a, c) in enumerate(PAIRS):
        want = mc.model_match(bank.kept[a], bank.kept[c], max_match=MAX_SIFT)
        assert np.array_equal(plain[q], want), (q, mc.first_difference(want, plain[q]))
        want = tc.gated(mc.model_match, bank.kept[a], bank.kept[c], bank.kept_types["a"][a], bank.kept_types["a"][c], max_match=MAX_SIFT)
        assert np.array_equal(typed[q], want), (q, mc.first_difference(want, typed[q]))
    assert [len(p) > 100 for p in plain[:4]] == [True] * 4 and len(plain[5]) == len(plain[6]) == 0
    assert len({first_cycle[k] for k in ("plain", "types a", "types b", "guided")}) == 4
    assert len({first_cycle[k] for k in ("single", "single typed", "single guided")}) == 3
    assert all(len(first_cycle[k]) > 8 * 50 for k in ("guided", "single", "single typed", "single guided"))


def test_twelve_cycles_give_the_same_bytes_and_no_growth(bank, other, first_cycle):
    used, footprints = [], []
    for k in range(12):
        got, footprint = _cycle(bank, other)
        assert got == first_cycle, f"cycle {k} differs from the first in {[n for n in got if got[n] != first_cycle[n]]}"
        used.append(_used())
        footprints.append(footprint)
    growth = used[-1] - used[1]
    print(f"dim {bank.dim}: footprint of one live matcher {footprints[-1]} bytes (all cycles: {sorted(set(footprints))}); "
          f"in use after close() 2: {used[1]}, after close() 12: {used[-1]}, growth {growth}")
    assert footprints[-1] >= WIDE * 512 * bank.dim, "the wide bank's padded rows alone are more"
    assert growth < footprints[-1] / 4, (growth, footprints[-1])


def test_a_live_matcher_reloads_without_growth(bank, first_cycle):
    from hessgpu_amd.matcher import Matcher
    m = Matcher(0, max_sift=MAX_SIFT, dim=bank.dim)
    sets_b = [s[::-1].copy() for s in bank.sets[::-1]]            # another bank: other counts per index, other rows

    def load_a():
        bank.load(m, "host u8")
        bank.locations_host(m)
        return _pairs(m), _guided(m, bank), _verify(m)

    assert load_a() == (first_cycle["plain"], first_cycle["guided"], first_cycle["verify"])
    m.set_bank(sets_b)
    m.set_bank_types([t[::-1].copy() for t in bank.types["b"][::-1]])
    assert [len(m.bank(i)) for i in range(6)] == list(KEPT[::-1])
    assert _pairs(m) != first_cycle["plain"]
    assert load_a() == (first_cycle["plain"], first_cycle["guided"], first_cycle["verify"])
    bank.rows_are_the_callers(m, "A again")
    used = []
    for k in range(20):
        bank.load(m, "host u8")
        m.set_bank_types(bank.types["ab"[k % 2]])
        bank.locations_host(m)
        used.append(_used())
    print(f"dim {bank.dim}: in use after load 2: {used[1]}, after load 20: {used[-1]}")
    assert used[-1] == used[1], used
    m.set_bank_types(None)
    assert (_pairs(m), _guided(m, bank)) == (first_cycle["plain"], first_cycle["guided"])
    m.close()


def test_refused_setters_change_nothing(bank, first_cycle):
    from hessgpu_amd.matcher import Matcher
    m = Matcher(0, max_sift=MAX_SIFT, dim=bank.dim)
    L, h = m.L, m.h
    bank.load(m, "device u8")
    m.set_bank_locations_device(bank.dev["loc"].data_ptr(), LOC_DEV_STRIDE)
    m.set_descriptors(1, bank.sets[5])
    flat_types = np.ascontiguousarray(np.concatenate(bank.types["a"]))
    host_rows, host_floats = np.ascontiguousarray(np.concatenate(bank.sets)), np.concatenate(bank.floats)
    counts = bank.counts.ctypes.data
    refusals = [
        ("odd types stride, bank", -1, "stride_bytes", lambda: L.hess_matcher_bank_set_types(h, flat_types.ctypes.data, 3)),
        ("odd types stride, device form", -1, "stride_bytes",
         lambda: L.hess_matcher_bank_set_types_device(h, bank.dev["types"].data_ptr(), 7)),
        ("odd types stride, slot", -1, "stride_bytes", lambda: L.hess_matcher_set_types(h, 1, flat_types.ctypes.data, 5)),
        ("host pointer as device bytes", -1, "not device memory",
         lambda: L.hess_matcher_bank_set_device_u8(h, 6, counts, host_rows.ctypes.data)),
        ("host pointer as device floats", -1, "not device memory",
         lambda: L.hess_matcher_bank_set_device(h, 6, counts, host_floats.ctypes.data)),
        ("misaligned device floats", -1, "aligned", lambda: L.hess_matcher_bank_set_device(h, 6, counts, bank.dev["f32"].data_ptr() + 4)),
        ("misaligned device locations", -1, "4-byte aligned",
         lambda: L.hess_matcher_bank_set_locations_device(h, bank.dev["loc"].data_ptr() + 2, LOC_DEV_STRIDE)),
        ("host pointer as device locations", -1, "not device memory",
         lambda: L.hess_matcher_bank_set_locations_device(h, bank.loc_host.ctypes.data, LOC_HOST_STRIDE)),
        ("locations stride below a pair", -1, "stride_bytes", lambda: L.hess_matcher_bank_set_locations(h, bank.loc_host.ctypes.data, 4)),
        ("types before descriptors, slot 0", -5, "load the descriptors", lambda: L.hess_matcher_set_types(h, 0, flat_types.ctypes.data, 2)),
    ]
    for what, code, word, call in refusals:
        assert call() == code, what
        assert word in (L.hess_matcher_last_error(h) or b"").decode(), (what, L.hess_matcher_last_error(h))
        assert _pairs(m) == first_cycle["plain"], what             # (a typed bank would answer with "types a")
        assert _guided(m, bank) == first_cycle["guided"], what     # (and refuse this; so would a bank without locations)
        bank.rows_are_the_callers(m, what)
    m.close()
    fresh = Matcher(0, max_sift=MAX_SIFT, dim=bank.dim)            # types and locations before any bank
    for fn, args, word in ((fresh.L.hess_matcher_bank_set_types, (flat_types.ctypes.data, 2), "load the descriptors"),
                           (fresh.L.hess_matcher_bank_set_types_device, (bank.dev["types"].data_ptr(), TYPE_STRIDE), "load the descriptors"),
                           (fresh.L.hess_matcher_bank_set_locations, (bank.loc_host.ctypes.data, LOC_HOST_STRIDE), "load the bank's descriptors")):
        assert fn(fresh.h, *args) == -5 and word in fresh.L.hess_matcher_last_error(fresh.h).decode()
    bank.load(fresh, "host u8")
    assert _pairs(fresh) == first_cycle["plain"]
    fresh.close()
