"""Batched matching on the GPU: a bank of descriptor sets on the device and many (a, b) pairs per call
(hess_matcher_bank_* / hess_matcher_match_pairs).  Every pair must equal the CPU oracle and the single-pair matcher bit
for bit -- integer work, the reference's tie order and truncation."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
from oracle_lib import oracle_match, oracle_quantize

pytestmark = pytest.mark.gpu

CONFIGS = [dict(mutual_best=True),
           dict(mutual_best=False, distmax=0.9, ratiomax=0.95),
           dict(mutual_best=True, distmax=1.2, ratiomax=0.9, max_match=300),
           dict(mutual_best=False, distmax=2.0, ratiomax=2.0, max_match=100)]   # max_match below the match count


def _oracle_all(bank, pairs, cfg):
    kw = dict(cfg)
    kw.setdefault("max_match", 4096)
    with ThreadPoolExecutor(8) as ex:   # (the oracle's C code runs without the GIL)
        return list(ex.map(lambda p: oracle_match(bank[p[0]], bank[p[1]], **kw), [tuple(p) for p in pairs]))


def _single_all(m, bank, pairs, cfg):
    kw = dict(cfg)
    kw.setdefault("max_match", 4096)
    out = []
    for a, b in pairs:
        m.set_descriptors(0, bank[a])
        m.set_descriptors(1, bank[b])
        out.append(m.match(**kw))
    return out


def _synthetic_sets(sizes, seed):
    """Full byte range; sets drawn from one pool with noise; duplicated rows inside and across sets.  Uniformly random bytes
    put every dot product far above the clamp of the score, so NO pair of these sets has a match in any configuration: they
    check sizes, chunking and that nothing overflows into a false match.  The bank cases that match, ties included, are in
    test_matcher_ties_gpu.py."""
    rng = np.random.RandomState(seed)
    pool = rng.randint(0, 256, size=(6000, 128)).astype(np.int32)
    out = []
    for n in sizes:
        idx = rng.choice(len(pool), size=n, replace=False) if n else np.zeros(0, int)
        s = pool[idx] + rng.randint(-12, 13, size=(n, 128))
        s = np.clip(s, 0, 255).astype(np.uint8)
        if n > 8:
            s[n // 2] = s[3]; s[n - 1] = s[3]; s[(n // 2) ^ 1] = s[5]   # duplicates far apart
            s[7] = np.clip(pool[0], 0, 255)                            # the same row in every set above 8
        out.append(s)
    return out


def _real_sets():
    from hessgpu_amd import HessContext

    g = HessContext(0)
    out = []
    for name in ("640-1.jpg", "640-2.jpg"):
        g.run(fixtures.load_rgb(name)[None])
        out.append(oracle_quantize(g.fetch(0)[1]))
    g.close()
    return out


def test_bank_of_real_and_synthetic_sets_all_ordered_pairs():
    from hessgpu_amd.matcher import Matcher

    max_sift = 3200
    sets = _real_sets() + _synthetic_sets([0, 1, 31, 255, 256, 257, 1500, 3100, max_sift + 100], seed=3)
    m = Matcher(0, max_sift=max_sift)
    m.set_bank(sets)
    bank = [m.bank(i) for i in range(len(sets))]
    for s, b in zip(sets, bank):
        assert np.array_equal(b, s[:max_sift])                # stored as given, truncated to max_sift
    assert len(bank[-1]) == max_sift and len(bank[2]) == 0
    pairs = np.array([(a, b) for a in range(len(sets)) for b in range(len(sets))], np.int32)  # (a, a) included
    assert len(pairs) > 64                                   # more than one chunk
    for cfg in CONFIGS:
        got = m.match_pairs(pairs, **cfg)
        ref = _oracle_all(bank, pairs, cfg)
        single = _single_all(m, bank, pairs, cfg)
        for k, (a, b) in enumerate(pairs):
            assert np.array_equal(got[k], ref[k]), (cfg, a, b, len(got[k]), len(ref[k]))
            assert np.array_equal(got[k], single[k]), (cfg, a, b)
        if cfg.get("max_match") == 100:
            assert max(len(g) for g in got) == 100
        assert sum(len(g) for g in got) > 0
    m.match_pairs(pairs[:5])
    assert m.last_ms() > 0.0
    # float input on the host: quantised like set_descriptors_f32
    rng = np.random.RandomState(5)
    f = [rng.rand(n, 128).astype(np.float32) * 0.6 - 0.05 for n in (10, 300, max_sift + 1)]
    m.set_bank(f)
    for i, x in enumerate(f):
        assert np.array_equal(m.bank(i), oracle_quantize(x[:max_sift]))
    m.close()


def test_bank_from_a_context_on_the_device():
    import hessgpu_amd
    from hessgpu_amd import HessError
    from hessgpu_amd.matcher import Matcher, all_pairs

    imgs = np.stack([fixtures.load_rgb(f"640-{i}.jpg") for i in range(1, 6)])
    g = hessgpu_amd.HessContext(0)
    counts = g.run(imgs)
    m = Matcher(0, max_sift=8192)
    m.set_bank_from_session(g)
    bank = []
    for i in range(len(imgs)):
        b = m.bank(i)
        assert len(b) == counts[i] > 100
        assert np.array_equal(b, oracle_quantize(g.fetch(i)[1])), i
        bank.append(b)
    pairs = np.concatenate([all_pairs(len(imgs)), all_pairs(len(imgs))[:, ::-1]])
    for cfg in CONFIGS[:2]:
        got = m.match_pairs(pairs, **cfg)
        ref = _oracle_all(bank, pairs, cfg)
        for k in range(len(pairs)):
            assert np.array_equal(got[k], ref[k]), (cfg, pairs[k])
        assert sum(len(x) for x in got) > 0
    # host memory is not device memory
    host = np.zeros((10, 128), np.float32)
    with pytest.raises(HessError) as e:
        m.set_bank_device(host.ctypes.data, [10])
    assert e.value.code == -1 and "device memory" in str(e.value)
    # -half (64-d) and -sd (no descriptors) contexts are refused
    for kw in (dict(half_sift=1), dict(compute_descriptors=0)):
        h = hessgpu_amd.HessContext(0, **kw)
        h.run(imgs[:1])
        with pytest.raises(ValueError):
            m.set_bank_from_session(h)
        h.close()
    # the bank survives the context's next run (built and copied before the call returned)
    g.run(imgs[::-1])
    assert np.array_equal(m.bank(0), bank[0])
    g.close()
    m.close()


def _quantiser_edges():
    v = []
    for k in range(-8, 300):
        b = np.float32((k + 0.5) / 512.0)
        v += [b, np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))]
    v += [0.0, -0.0, 0.5, 0.49999997, 0.50000006, 0.75, 1.0, 1.5, 3.0, 100.0, 1e6, -1e-7, -0.5 / 512, -0.001,
          -0.25, -0.49, -3.0, np.float32(1e-30), np.float32(-1e-30)]
    v = np.array(v, dtype=np.float32)
    v = np.concatenate([v, np.zeros((-len(v)) % 128, np.float32)])
    return v.reshape(-1, 128)


def test_device_quantiser_edges():
    import torch

    from hessgpu_amd.matcher import Matcher

    edges = _quantiser_edges()
    rng = np.random.RandomState(9)
    more = (rng.rand(300, 128).astype(np.float32) * 1.2 - 0.1)
    host = np.concatenate([edges, more])
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    m = Matcher(0, max_sift=4096)
    counts = [len(edges), 0, len(more)]
    m.set_bank_device(t.data_ptr(), counts)
    assert np.array_equal(m.bank(0), oracle_quantize(edges))
    assert len(m.bank(1)) == 0
    assert np.array_equal(m.bank(2), oracle_quantize(more))
    # max_sift truncation of a device set
    m2 = Matcher(0, max_sift=100)
    m2.set_bank_device(t.data_ptr(), counts)
    assert np.array_equal(m2.bank(2), oracle_quantize(more[:100]))
    m.close()
    m2.close()


def test_chunks_do_not_change_results():
    from hessgpu_amd import HessError
    from hessgpu_amd.matcher import Matcher

    rng = np.random.RandomState(21)
    sizes = list(rng.randint(0, 400, size=18)) + [0, 1]
    sets = _synthetic_sets(sizes, seed=4)
    m = Matcher(0, max_sift=4096)
    m.set_bank(sets)
    n = len(sets)
    pairs = np.array([(a, b) for a in range(n) for b in range(n)], np.int32)
    pairs = np.concatenate([pairs, pairs[rng.permutation(len(pairs))[:50]]])   # repeats, shuffled
    assert len(pairs) > 3 * 64
    for cfg in (dict(mutual_best=True), dict(mutual_best=False, distmax=2.0, ratiomax=2.0, max_match=40)):
        whole = m.match_pairs(pairs, **cfg)
        again = m.match_pairs(pairs, **cfg)
        for k, p in enumerate(pairs):
            one = m.match_pairs(p[None], **cfg)[0]
            assert np.array_equal(whole[k], one), (cfg, p)
            assert np.array_equal(whole[k], again[k]), (cfg, p)
        bank = [m.bank(i) for i in range(n)]
        ref = _oracle_all(bank, pairs[:120], cfg)
        for k in range(120):
            assert np.array_equal(whole[k], ref[k]), (cfg, pairs[k])
    assert m.match_pairs(np.zeros((0, 2), np.int32)) == []
    for bad in ([[0, n]], [[n + 5, 0]]):
        with pytest.raises(HessError) as e:
            m.match_pairs(bad)
        assert e.value.code == -1
    m.close()


def test_bank_and_single_pair_slots_are_independent():
    from hessgpu_amd.matcher import Matcher

    rng = np.random.RandomState(2)
    x, y = _synthetic_sets([900, 1200], seed=8)
    sets = _synthetic_sets([700, 2500, 1300], seed=9)
    m = Matcher(0, max_sift=4096)
    m.set_descriptors(0, x)
    m.set_descriptors(1, y)
    m.set_bank(sets)
    pairs = np.array([[0, 1], [1, 2], [2, 0], [1, 1]], np.int32)
    first = m.match_pairs(pairs)
    for mutual in (True, False):                               # the single-pair slots still hold x and y
        assert np.array_equal(m.match(mutual_best=mutual), oracle_match(x, y, mutual_best=mutual))
    m.set_descriptors(0, rng.randint(0, 256, size=(3000, 128)).astype(np.uint8))
    m.set_descriptors(1, rng.randint(0, 256, size=(3000, 128)).astype(np.uint8))
    m.match()
    again = m.match_pairs(pairs)                               # ... and the bank still holds its sets
    for k, (a, b) in enumerate(pairs):
        assert np.array_equal(again[k], first[k])
        assert np.array_equal(again[k], oracle_match(sets[a], sets[b]))
    m.close()
