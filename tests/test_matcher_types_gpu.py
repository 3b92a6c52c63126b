"""The feature-type gate of the matcher on the GPU (hess_matcher_set_types / _bank_set_types / _bank_set_types_device):
every result equals the gated reference of tests/matcher_type_cases.py -- the CPU oracle per class, indices mapped back,
merged in row order, truncated -- bit for bit.  tests/test_matcher_type_cases.py shows on the CPU that these inputs tell
the gate from a filter applied after an ungated match."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
import matcher_cases as mc
import matcher_cases_half as mh
import matcher_type_cases as tc
from oracle_lib import oracle_match, oracle_quantize

pytestmark = pytest.mark.gpu

# the eight configurations without a limit, a limit of 3 and, per pair, of n1 (None)
BANK_CONFIGS = [dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=mc.BANK_MAX_SIFT) for dm, rm, mutual in mc.CONFIGS]
BANK_CONFIGS += [dict(distmax=2.0, ratiomax=2.0, mutual_best=False, max_match=3),
                 dict(distmax=0.7, ratiomax=0.8, mutual_best=True, max_match=3)]


def _reference_all(sets, types, pairs, cfg, match=tc.gated_reference):
    uniq = sorted({tuple(p) for p in pairs})
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
        res = dict(zip(uniq, ex.map(lambda p: match(sets[p[0]], sets[p[1]], types[p[0]], types[p[1]], **cfg), uniq)))
    return [res[tuple(p)] for p in pairs]


@functools.lru_cache(maxsize=None)
def _bank_reference(kind, k):
    """The references of all ordered pairs of the bank for BANK_CONFIGS[k].  "highbits" is "random" by definition
    (type & 3: test_matcher_type_cases.py checks that gated_reference agrees), so the two share one."""
    kind = "random" if kind == "highbits" else kind
    return _reference_all(mc.bank_sets(), tc.bank_types(kind), mc.bank_all_pairs(), BANK_CONFIGS[k])


@pytest.mark.parametrize("kind", tc.KINDS)
def test_bank_all_ordered_pairs(kind):
    from hessgpu_amd.matcher import Matcher

    sets, types = mc.bank_sets(), tc.bank_types(kind)
    pairs = mc.bank_all_pairs()
    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT)
    m.set_bank(sets)
    m.set_bank_types(types)
    for i, s in enumerate(sets):
        assert np.array_equal(m.bank(i), s), i                     # the caller's order, whatever the storage order
    total = 0
    for k, cfg in enumerate(BANK_CONFIGS):
        got = m.match_pairs(pairs, **cfg)
        ref = _bank_reference(kind, k)
        for q, (a, b) in enumerate(pairs):
            assert np.array_equal(got[q], ref[q]), (kind, cfg, a, b, mc.first_difference(ref[q], got[q]))
        total += sum(len(r) for r in ref)
        if cfg["max_match"] == 3:
            assert max(len(g) for g in got) == 3
    assert total > 0
    # max_match = n1 of each pair: one pair per call
    cfg = dict(distmax=2.0, ratiomax=2.0, mutual_best=False)
    big = [(a, b) for a in mc.BANK_BIG for b in mc.BANK_BIG]
    for a, b in big:
        ref = tc.gated_reference(sets[a], sets[b], types[a], types[b], max_match=len(sets[a]), **cfg)
        got = m.match_pairs([(a, b)], max_match=len(sets[a]), **cfg)[0]
        assert len(ref) > 0 and np.array_equal(got, ref), (kind, a, b, mc.first_difference(ref, got))
    if kind == "saddle":    # one class: the gated result is the ungated one, every placed tie on its seam
        for k in (0, 3, 7):
            ref = _bank_reference(kind, k)
            for q in (66, 67, 68, 76, 77, 78, 86, 87, 88):
                a, b = pairs[q]
                assert np.array_equal(ref[q], oracle_match(sets[a], sets[b], **BANK_CONFIGS[k])), (k, a, b)
    # types removed: the ungated oracle again
    m.set_bank_types(None)
    for i, s in enumerate(sets):
        assert np.array_equal(m.bank(i), s), i
    for cfg in (BANK_CONFIGS[0], BANK_CONFIGS[7]):
        got = m.match_pairs(big, **cfg)
        for q, (a, b) in enumerate(big):
            assert np.array_equal(got[q], oracle_match(sets[a], sets[b], **cfg)), (kind, "ungated", a, b)
    m.close()


def test_bank_chunk_of_more_than_64_jobs_at_the_segment_cap():
    """64 pairs of the three large sets in one chunk: up to 256 class jobs in one launch."""
    from hessgpu_amd.matcher import Matcher

    sets = mc.bank_sets()
    pairs = mc.bank_big_chunk_pairs()
    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT)
    m.set_bank(sets)
    for kind in ("random", "position"):
        types = tc.bank_types(kind)
        m.set_bank_types(types)                                    # (the second time: retyping a typed bank)
        for cfg in (BANK_CONFIGS[3], BANK_CONFIGS[0]):
            whole = m.match_pairs(pairs, **cfg)
            ref = _reference_all(sets, types, pairs, cfg)
            for q, p in enumerate(pairs):
                assert len(ref[q]) > 0
                assert np.array_equal(whole[q], ref[q]), (kind, cfg, tuple(p), mc.first_difference(ref[q], whole[q]))
            assert np.array_equal(m.match_pairs(pairs[5][None], **cfg)[0], whole[5])      # one pair per call == the list
    assert m.last_ms() > 0.0
    m.close()


def _check_single(m, a, b, ta, tb, label):
    n1 = len(a)
    for dm, rm, mutual in mc.CONFIGS:
        kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual)
        ref = tc.gated_reference(a, b, ta, tb, max_match=n1, **kw)
        assert len(ref) > 0, (label, dm, rm, mutual)
        got = m.match(max_match=n1, **kw)
        assert np.array_equal(got, ref), (label, dm, rm, mutual, mc.first_difference(ref, got))
        got = m.match(max_match=3, **kw)
        assert np.array_equal(got, ref[:3]), (label, dm, rm, mutual, "max_match 3")


@pytest.mark.parametrize("n1,n2", ((600, 700), (2100, 2050)))
def test_single_pair_with_types(n1, n2):
    from hessgpu_amd import HessError, _abi
    from hessgpu_amd.matcher import Matcher

    a, b = mc.single_pair(n1, n2)
    m = Matcher(0, max_sift=4096)
    m.set_descriptors(0, a)
    m.set_descriptors(1, b)
    for kind in tc.KINDS if n1 == 600 else ("random", "position"):
        ta, tb = tc.single_types(n1, n2, kind)
        m.set_types(0, ta)                                         # (from the second kind on: retyping a slot)
        m.set_types(1, tb)
        _check_single(m, a, b, ta, tb, (n1, n2, kind))
    # types through a key array's field, stride 24
    keys = np.zeros(n1, _abi.KEYPOINT_DTYPE)
    keys["type"] = ta
    m.set_types(0, keys)
    _check_single(m, a, b, ta, tb, (n1, n2, "keys"))
    # set_descriptors clears the slot's types: one slot typed is refused, both untyped is the ungated match
    m.set_descriptors(0, a)
    with pytest.raises(HessError) as e:
        m.match()
    assert e.value.code == -5
    m.set_descriptors(1, b)
    for mutual in (True, False):
        assert np.array_equal(m.match(mutual_best=mutual, max_match=n1), oracle_match(a, b, mutual_best=mutual, max_match=n1))
    m.close()


def test_single_pair_straddling_the_threshold_with_types():
    """Typed slots take the job tables at any size: the same sets just under and over the ungated path's 3 Mi switch."""
    from hessgpu_amd.matcher import Matcher

    s1, s2 = mc.straddle_sets()
    m = Matcher(0, max_sift=4096)
    for kind in ("random", "position"):
        t1, t2 = tc.straddle_types(kind)
        for n in (len(s1) - 1, len(s1)):
            m.set_descriptors(0, s1[:n])
            m.set_descriptors(1, s2)
            m.set_types(0, t1[:n])
            m.set_types(1, t2)
            _check_single(m, s1[:n], s2, t1[:n], t2, ("straddle", kind, n))
    m.close()


def test_bank_of_64d_sets():
    """dim = 64: the reference is the oracle on the zero-padded class subsets (matcher_cases_half.pad128)."""
    from hessgpu_amd.matcher import Matcher

    sets = mh.bank_sets()
    pairs = mc.bank_all_pairs()

    def match64(a, b, ta, tb, **cfg):
        return tc.gated(lambda x, y, **kw: oracle_match(mh.pad128(x), mh.pad128(y), **kw), a, b, ta, tb, **cfg)

    m = Matcher(0, max_sift=mc.BANK_MAX_SIFT, dim=64)
    m.set_bank(sets)
    for kind in ("random", "position"):
        types = tc.bank_types(kind)
        m.set_bank_types(types)
        for i, s in enumerate(sets):
            assert np.array_equal(m.bank(i), s), i
        for cfg in (BANK_CONFIGS[0], BANK_CONFIGS[3], BANK_CONFIGS[7]):
            got = m.match_pairs(pairs, **cfg)
            ref = _reference_all(sets, types, pairs, cfg, match=match64)
            for q, (a, b) in enumerate(pairs):
                assert np.array_equal(got[q], ref[q]), (kind, cfg, a, b, mc.first_difference(ref[q], got[q]))
            assert sum(len(r) for r in ref) > 0
    # the other length removes everything, types included
    m.set_dim(128)
    from hessgpu_amd import HessError
    with pytest.raises(HessError) as e:
        m.set_bank_types(tc.bank_types("random"))
    assert e.value.code == -5
    m.close()


@pytest.mark.parametrize("fmt", ("f32", "u8"))
def test_types_from_a_context_on_the_device(fmt):
    """set_bank_from_session(types=True) reads the type field of the device key records (stride 24): the same results as
    the host route from the fetched keys, and as the gated reference."""
    import hessgpu_amd
    from hessgpu_amd.matcher import Matcher, all_pairs

    imgs = np.stack([fixtures.load_rgb(f"640-{i}.jpg") for i in range(1, 4)])
    g = hessgpu_amd.HessContext(0)
    if fmt == "u8":
        g.set_descriptor_format("u8")
    counts = g.run(imgs)
    fetched = [g.fetch(i) for i in range(len(imgs))]
    keys = [k for k, _ in fetched]
    desc = [d if fmt == "u8" else oracle_quantize(d) for _, d in fetched]
    for i, k in enumerate(keys):
        assert len(k) == counts[i] > 100
        assert len(set((k["type"] & 3).tolist())) >= 2, (i, np.bincount(k["type"] & 3))
    types = [k["type"] for k in keys]
    pairs = np.concatenate([all_pairs(len(imgs)), all_pairs(len(imgs))[:, ::-1]])
    dev = Matcher(0, max_sift=8192)
    dev.set_bank_from_session(g, types=True)
    host = Matcher(0, max_sift=8192)
    host.set_bank(desc)
    host.set_bank_types(keys)                                      # the key arrays themselves: their "type" field
    cut = Matcher(0, max_sift=500)                                 # truncation first, descriptors and types alike
    cut.set_bank_from_session(g, types=True)
    for i in range(len(imgs)):
        assert np.array_equal(dev.bank(i), desc[i]) and np.array_equal(cut.bank(i), desc[i][:500]), i
    total = differs = 0
    for cfg in (dict(mutual_best=True), dict(mutual_best=False, distmax=2.0, ratiomax=2.0), dict(mutual_best=True, max_match=3)):
        a, b = dev.match_pairs(pairs, **cfg), host.match_pairs(pairs, **cfg)
        c = cut.match_pairs(pairs, **cfg)
        kw = dict(cfg)
        kw.setdefault("max_match", 4096)
        for q, (p0, p1) in enumerate(pairs):
            ref = tc.gated_reference(desc[p0], desc[p1], types[p0], types[p1], **kw)
            assert np.array_equal(a[q], ref), (fmt, cfg, p0, p1, mc.first_difference(ref, a[q]))
            assert np.array_equal(b[q], ref), (fmt, cfg, p0, p1)
            ref = tc.gated_reference(desc[p0][:500], desc[p1][:500], types[p0][:500], types[p1][:500], **kw)
            assert np.array_equal(c[q], ref), (fmt, cfg, p0, p1, "max_sift 500")
            total += len(a[q])
            u = oracle_match(desc[p0], desc[p1], **kw)
            u = u[(types[p0][u[:, 0]] & 3) == (types[p1][u[:, 1]] & 3)]
            differs += not np.array_equal(u[:len(a[q])], a[q])
    assert total > 0
    assert differs > 0          # filtering the ungated result afterwards is not this result
    # the types live in the matcher: the context's next run does not touch them
    g.run(imgs[::-1])
    again = dev.match_pairs(pairs)
    for q in range(len(pairs)):
        assert np.array_equal(again[q], host.match_pairs(pairs)[q])
    for x in (dev, host, cut):
        x.close()
    g.close()


def test_errors_leave_the_matcher_usable():
    import torch

    from hessgpu_amd import HessError
    from hessgpu_amd.matcher import Matcher

    a, b = mc.single_pair(600, 700)
    ta, tb = tc.single_types(600, 700, "random")
    sets, types = mc.bank_sets()[3:6], tc.bank_types("random")[3:6]
    flat = np.concatenate(types)
    m = Matcher(0, max_sift=4096)
    L, h = m.L, m.h

    def refused(code, word, fn, *args):
        assert fn(h, *args) == code, (fn.__name__, args)
        assert word in (L.hess_matcher_last_error(h) or b"").decode(), (word, L.hess_matcher_last_error(h))

    # types before the descriptors they belong to
    refused(-5, "set_types", L.hess_matcher_set_types, 0, ta.ctypes.data, 2)
    refused(-5, "bank_set_types", L.hess_matcher_bank_set_types, flat.ctypes.data, 2)
    refused(-5, "bank_set_types_device", L.hess_matcher_bank_set_types_device, flat.ctypes.data, 2)
    m.set_descriptors(0, a)
    m.set_descriptors(1, b)
    m.set_bank(sets)
    pairs = [(0, 1), (1, 2), (2, 0)]
    # a stride below 2 or odd; an index that is no slot
    for stride in (0, 1, 3, 23):
        refused(-1, "stride_bytes", L.hess_matcher_set_types, 0, ta.ctypes.data, stride)
        refused(-1, "stride_bytes", L.hess_matcher_bank_set_types, flat.ctypes.data, stride)
        refused(-1, "stride_bytes", L.hess_matcher_bank_set_types_device, flat.ctypes.data, stride)
    refused(-1, "index", L.hess_matcher_set_types, 2, ta.ctypes.data, 2)
    # the device form: host memory, an odd address, a range past the allocation
    refused(-1, "device memory", L.hess_matcher_bank_set_types_device, flat.ctypes.data, 2)
    dt = torch.from_numpy(flat.view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    refused(-1, "aligned", L.hess_matcher_bank_set_types_device, dt.data_ptr() + 1, 2)
    refused(-1, "allocation", L.hess_matcher_bank_set_types_device, dt.data_ptr(), 1 << 26)
    # nothing changed: both are still the ungated matcher
    assert np.array_equal(m.match(max_match=600), oracle_match(a, b, max_match=600))
    for q, (p0, p1) in enumerate(pairs):
        assert np.array_equal(m.match_pairs(pairs)[q], oracle_match(sets[p0], sets[p1]))
    # exactly one slot typed
    m.set_types(1, tb)
    buf = np.zeros((600, 2), np.int32)
    refused(-5, "slot", L.hess_matcher_match, 600, buf.ctypes.data, None, None, 0.7, 0.8, 32.0, 16.0, 1)
    # guided with types on either slot, or both: refused, never ignored
    eye = np.eye(3, dtype=np.float32)
    m.set_locations(0, np.zeros((600, 2), np.float32))
    m.set_locations(1, np.zeros((700, 2), np.float32))
    refused(-6, "guided", L.hess_matcher_match, 600, buf.ctypes.data, eye.ctypes.data, eye.ctypes.data, 0.7, 0.8, 32.0, 16.0, 1)
    m.set_types(0, ta)
    refused(-6, "guided", L.hess_matcher_match, 600, buf.ctypes.data, eye.ctypes.data, eye.ctypes.data, 0.7, 0.8, 32.0, 16.0, 1)
    with pytest.raises(HessError):
        m.match(H=eye, F=eye)
    # ... and the typed match works, the device form works with a good pointer, removing the types works
    assert np.array_equal(m.match(max_match=600), tc.gated_reference(a, b, ta, tb, max_match=600))
    m.set_bank_types_device(dt.data_ptr(), 2)
    for q, (p0, p1) in enumerate(pairs):
        assert np.array_equal(m.match_pairs(pairs)[q], tc.gated_reference(sets[p0], sets[p1], types[p0], types[p1]))
    m.set_types(0, None)
    m.set_types(1, None)
    assert np.array_equal(m.match(max_match=600), oracle_match(a, b, max_match=600))
    guided = m.match(H=eye, F=eye, hdistmax=1e9, fdistmax=1e9, max_match=600)     # guided is available again
    assert guided.shape[1] == 2
    # loading a bank removes its types
    m.set_bank(sets)
    for q, (p0, p1) in enumerate(pairs):
        assert np.array_equal(m.match_pairs(pairs)[q], oracle_match(sets[p0], sets[p1]))
    m.close()


def test_siftgpu_api_set_feature_types():
    """SiftMatchGPU::SetFeatureTypes through its flat mirror: siftmatch_set_types with the keys' stride is what
    SetFeatureTypes(index, keys) passes on."""
    from hessgpu_amd import _abi
    from siftgpu_lib import lib

    L = lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    for name, res, args in [("siftmatch_create", vp, [i32]), ("siftmatch_destroy", None, [vp]),
                            ("siftmatch_set_descriptors_u8", None, [vp, i32, i32, vp]),
                            ("siftmatch_set_types", i32, [vp, i32, vp, i32]),
                            ("siftmatch_get_match", i32, [vp, i32, vp, f32, f32, i32]),
                            ("siftmatch_get_guided_match", i32, [vp, i32, vp, vp, vp, f32, f32, f32, f32, i32])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    a, b = mc.single_pair(600, 700)
    ta, tb = tc.single_types(600, 700, "random")
    ka, kb = np.zeros(600, _abi.KEYPOINT_DTYPE), np.zeros(700, _abi.KEYPOINT_DTYPE)
    ka["type"], kb["type"] = ta, tb
    hnd = L.siftmatch_create(4096)
    assert L.siftmatch_set_types(hnd, 0, ta.ctypes.data, 2) == -5              # before the descriptors
    L.siftmatch_set_descriptors_u8(hnd, 0, 600, a.ctypes.data)
    L.siftmatch_set_descriptors_u8(hnd, 1, 700, b.ctypes.data)
    buf = np.zeros((600, 2), np.int32)
    for mutual in (True, False):
        n = L.siftmatch_get_match(hnd, 600, buf.ctypes.data, 0.7, 0.8, int(mutual))
        assert np.array_equal(buf[:n], oracle_match(a, b, mutual_best=mutual, max_match=600))
    assert L.siftmatch_set_types(hnd, 0, ka.ctypes.data + 22, 24) == 0          # &keys[0].type, sizeof(SiftKeypoint)
    assert L.siftmatch_set_types(hnd, 1, tb.ctypes.data, 2) == 0
    for mutual in (True, False):
        n = L.siftmatch_get_match(hnd, 600, buf.ctypes.data, 0.7, 0.8, int(mutual))
        ref = tc.gated_reference(a, b, ta, tb, mutual_best=mutual, max_match=600)
        assert len(ref) > 0 and np.array_equal(buf[:n], ref), mutual
    eye = np.eye(3, dtype=np.float32)
    assert L.siftmatch_get_guided_match(hnd, 600, buf.ctypes.data, eye.ctypes.data, eye.ctypes.data, 0.7, 0.8, 32, 16, 1) == 0
    assert L.siftmatch_set_types(hnd, 0, None, 24) == 0 and L.siftmatch_set_types(hnd, 1, None, 2) == 0
    n = L.siftmatch_get_match(hnd, 600, buf.ctypes.data, 0.7, 0.8, 1)
    assert np.array_equal(buf[:n], oracle_match(a, b, max_match=600))
    L.siftmatch_destroy(hnd)
