"""hess_matcher_verify_pairs on the GPU.  The reference in every comparison is the chain of the three existing entry points on
the SAME matcher (steps 1-5 of the rule in include/hess_abi.h: match_pairs, estimate_pairs, the one-matrix geometry,
match_pairs_guided, estimate_pairs), compared byte for byte: matches, counts, every field of both results, masks and putative
lists.  The banks are those of tests/verify_cases.py, whose properties tests/test_verify_cases.py holds on the CPU."""
import numpy as np
import pytest

import matcher_cases as mc
import verify_cases as vc

pytestmark = pytest.mark.gpu


def _hm():
    from hessgpu_amd import matcher as hm
    return hm


def _matcher(sets, locs, **kw):
    m = _hm().Matcher(0, **kw)
    m.set_bank(sets)
    m.set_bank_locations(locs)
    return m


def _params(model, bound=None, T=300, seed=11, refit=0, gb=None, fin=True, dm=vc.DISTMAX, rm=vc.RATIOMAX, mutual=True):
    import geom_cases as gcs
    return _hm().Matcher._verify_params(model, gcs.BOUND[model] if bound is None else bound, T, seed, refit, gb, fin, dm, rm, mutual)


def chain(m, pairs, P, max_match):
    """Steps 1-5 through hess_matcher_match_pairs, _estimate_pairs and _match_pairs_guided, with the raw arrays."""
    hm = _hm()
    L, h = m.L, m.h
    ab = hm.check_pairs(pairs)
    n, w = len(ab), max(max_match, 1)
    g = P["geom"].copy()
    dm, rm, mutual = float(P["distmax"][0]), float(P["ratiomax"][0]), int(P["mutual_best"][0])
    put, nput = np.zeros((n, w, 2), np.int32), np.zeros(n, np.int32)
    assert L.hess_matcher_match_pairs(h, n, ab.ctypes.data, max_match, put.ctypes.data, nput.ctypes.data, dm, rm, mutual) == 0
    res1 = np.zeros(n, hm.GEOM_RESULT_DTYPE)
    assert L.hess_matcher_estimate_pairs(h, n, ab.ctypes.data, max_match, put.ctypes.data, nput.ctypes.data, g.ctypes.data,
                                         res1.ctypes.data, None) == 0
    gb = P["guided_bound"][0] if P["guided_bound"][0] != 0 else g["bound"][0]
    M = res1["M"].reshape(n, 3, 3)
    geo = hm.guided_pairs(n, H=M, hdistmax=gb) if int(g["model"][0]) == 1 else hm.guided_pairs(n, F=M, fdistmax=gb)
    out, cnt = np.zeros((n, w, 2), np.int32), np.zeros(n, np.int32)
    assert L.hess_matcher_match_pairs_guided(h, n, ab.ctypes.data, geo.ctypes.data, max_match, out.ctypes.data, cnt.ctypes.data,
                                             dm, rm, mutual) == 0
    res2 = np.zeros(n, hm.GEOM_RESULT_DTYPE)
    res2["hypothesis"] = -1
    mask = np.zeros((n, w), np.uint8)
    if int(P["final_estimate"][0]):
        assert L.hess_matcher_estimate_pairs(h, n, ab.ctypes.data, max_match, out.ctypes.data, cnt.ctypes.data, g.ctypes.data,
                                             res2.ctypes.data, mask.ctypes.data) == 0
    return dict(out=out, cnt=cnt, put=put, nput=nput, res1=res1, res2=res2, mask=mask)


def _blob(out, cnt, res, mask, put):
    """Everything a call returned, as bytes: lists up to their counts."""
    parts = [cnt.tobytes(), res.tobytes()]
    for p in range(len(cnt)):
        parts.append(out[p, :cnt[p]].tobytes())
        if put is not None:
            parts.append(put[p, :res["nputative"][p]].tobytes())
    if mask is not None:
        parts.append(mask.tobytes())
    return b"".join(parts)


def same(m, pairs, P, max_match, ref=None, inlier=True, putative=True, what=None):
    """verify_pairs equals the chain in every byte -> (the reference, the call's blob)."""
    ref = chain(m, pairs, P, max_match) if ref is None else ref
    out, cnt, res, mask, put = m.verify_pairs_raw(pairs, P, max_match, inlier=inlier, putative=putative)
    assert np.array_equal(cnt, ref["cnt"]), (what, cnt.tolist(), ref["cnt"].tolist())
    assert np.array_equal(res["nguided"], ref["cnt"]) and np.array_equal(res["nputative"], ref["nput"]), what
    assert not res["reserved"].any()
    for p in range(len(cnt)):
        assert np.array_equal(out[p, :cnt[p]], ref["out"][p, :cnt[p]]), (what, p, mc.first_difference(ref["out"][p, :cnt[p]], out[p, :cnt[p]]))
        if putative:
            k = ref["nput"][p]
            assert np.array_equal(put[p, :k], ref["put"][p, :k]), (what, p, "putative")
        for name, want in (("putative", ref["res1"]), ("final", ref["res2"])):
            assert res[name][p].tobytes() == want[p].tobytes(), (what, p, name, res[name][p], want[p])
    assert res["putative"].tobytes() == ref["res1"].tobytes() and res["final"].tobytes() == ref["res2"].tobytes(), what
    if inlier:
        assert mask.tobytes() == ref["mask"].tobytes(), (what, "mask")
    return ref, _blob(out, cnt, res, mask, put)


def _has_model(r):
    return r["hypothesis"] >= 0


@pytest.fixture(scope="module")
def bank():
    m = _matcher(*vc.bank())
    yield m
    m.close()


@pytest.mark.parametrize("refit", [0, 2])
@pytest.mark.parametrize("model", ["H", "F"])
def test_bank_pairs_equal_the_chain(bank, model, refit):
    pairs, names = vc.bank_pairs()
    n1max = max(len(s) for s in vc.bank()[0])
    seen_refit = False
    for mutual in (True, False):
        for fin in (True, False):
            for gb in (None, 2.5):
                P = _params(model, refit=refit, gb=gb, fin=fin, mutual=mutual)
                ref, _ = same(bank, pairs, P, n1max, what=(model, refit, mutual, fin, gb))
                has = _has_model(ref["res1"])
                # non-vacuity, on the reference chain's output
                assert (has & (ref["cnt"] > 0)).any() and (~has).any(), (model, has.tolist(), ref["cnt"].tolist())
                below = ("H below k",) if model == "H" else vc.BELOW + ("H n = k",)     # 3, 7 and 4 matches: k is 4 or 8
                for name in below + ("empty first", "empty second"):
                    p = names.index(name)
                    assert not has[p] and ref["cnt"][p] == 0 and not ref["res1"]["M"][p].any(), name
                assert ref["nput"][names.index("H 1031")] > 768 and ref["nput"][names.index("H n = k")] == 4
                assert fin or (not _has_model(ref["res2"]).any() and not ref["mask"].any())
                seen_refit |= bool((ref["res1"]["reserved"][:, 0] > 0).any() or (ref["res2"]["reserved"][:, 0] > 0).any())
    assert seen_refit == (refit > 0)
    own = names.index(f"{model} 300")
    assert _has_model(ref["res1"])[own] and ref["res1"]["inliers"][own] >= 100


def test_more_than_2048_putative_matches_cross_the_estimators_lds_chunk():
    m = _matcher(*vc.big(), max_sift=vc.BIG_MAX_SIFT)
    for refit, fin in ((2, True), (0, False)):
        P = _params("H", T=256, refit=refit, fin=fin)
        ref, _ = same(m, [[0, 1]], P, vc.BIG_MAX_SIFT, what=("big", refit, fin))
        assert ref["nput"][0] > 2048 and _has_model(ref["res1"])[0] and ref["cnt"][0] > 2048
    m.close()


def test_max_match_40_truncates_both_lists_and_strides_the_compacted_buffers(bank):
    pairs = np.array([vc.pair_of("H 300"), vc.pair_of("F 300"), (vc.pair_of("H 300")[0],) * 2, vc.pair_of("H below k")], np.int32)
    for model in ("H", "F"):
        for mutual in (True, False):
            ref, _ = same(bank, pairs, _params(model, refit=2, mutual=mutual), 40, what=("cut", model, mutual))
            assert ref["nput"][:3].tolist() == [40, 40, 40] and ref["cnt"].max() == 40      # both lists are cut somewhere
    ref, _ = same(bank, pairs, _params("H"), 0, what="max_match 0")
    assert not ref["cnt"].any() and not _has_model(ref["res1"]).any()


@pytest.mark.parametrize("model", ["H", "F"])
def test_300_pairs_cross_both_chunks_and_take_seed_plus_list_position(bank, model):
    pairs = vc.many_pairs(300)
    P = _params(model, T=64, seed=0xfffffff0, refit=2)             # (seed + p wraps mod 2^32 within the list)
    ref, _ = same(bank, pairs, P, 80, what=("many", model))
    hyp = ref["res1"]["hypothesis"]
    where = {}
    for p, ab in enumerate(map(tuple, pairs.tolist())):
        where.setdefault(ab, []).append(p)
    # the same (a, b) at positions with the same offset in a 64-pair chunk returns different hypotheses somewhere: a
    # chunk-local p could not reproduce the chain
    differs = 0
    for ab, ps in where.items():
        by_offset = {}
        for p in ps:
            by_offset.setdefault(p % 64, []).append(p)
        for group in by_offset.values():
            differs += len(group) > 1 and len({int(hyp[p]) for p in group}) > 1
    assert differs > 0
    assert (hyp >= 0).any() and (hyp < 0).any()


def test_600_pairs_reuse_both_pinned_slots(bank):
    """Three groups of chunks (256 + 256 + 88 pairs): the third is delivered through the slot the first one used."""
    for fin in (True, False):
        same(bank, vc.many_pairs(600), _params("H", T=64, refit=2, fin=fin), 80, what=("600", fin))


def test_64_d_bank():
    m = _matcher(*vc.bank(half=True), dim=64)
    pairs, names = vc.bank_pairs()
    for model in ("H", "F"):
        ref, _ = same(m, pairs, _params(model, refit=2), 1100, what=("half", model))
        assert (_has_model(ref["res1"]) & (ref["cnt"] > 0)).any()
    m.close()


def test_outputs_passed_as_null_change_nothing_else(bank):
    pairs, _ = vc.bank_pairs()
    for fin in (True, False):
        P = _params("H", refit=2, fin=fin)
        ref = chain(bank, pairs, P, 1100)
        for inlier in (True, False):
            for putative in (True, False):
                same(bank, pairs, P, 1100, ref=ref, inlier=inlier, putative=putative, what=("null", fin, inlier, putative))


def test_twenty_repeats_give_the_same_bytes(bank):
    pairs, _ = vc.bank_pairs()
    P = _params("F", T=64, refit=2)
    _, first = same(bank, pairs, P, 1100)
    for _ in range(20):
        assert _blob(*bank.verify_pairs_raw(pairs, P, 1100, inlier=True, putative=True)) == first


def test_buffers_grown_and_reused_by_the_other_calls_and_back():
    m = _matcher(*vc.bank())
    pairs, _ = vc.bank_pairs()
    P = _params("H", refit=2)
    _, first = same(m, pairs, P, 1100)
    # the three calls on other lists, larger and smaller; then the same bytes again
    other = vc.many_pairs(130)
    before = chain(m, other, _params("F", T=512), 70)
    a = m.match_pairs(pairs[::-1], max_match=5)
    assert _blob(*m.verify_pairs_raw(pairs, P, 1100, inlier=True, putative=True)) == first
    # and those three calls after a verify_pairs give what they gave before
    after = chain(m, other, _params("F", T=512), 70)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    b = m.match_pairs(pairs[::-1], max_match=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    m.close()


def test_the_wrapper_returns_the_chain_as_dicts(bank):
    pairs, names = vc.bank_pairs()
    P = _params("H", T=300, seed=3, refit=2, gb=6.0)
    ref = chain(bank, pairs, P, 1100)
    got = bank.verify_pairs(pairs, "H", 8.0, hypotheses=300, seed=3, refit=2, guided_bound=6.0, max_match=1100, putative=True)
    assert len(got) == len(pairs)
    for p, d in enumerate(got):
        k = ref["cnt"][p]
        assert np.array_equal(d["matches"], ref["out"][p, :k]) and np.array_equal(d["putative"], ref["put"][p, :ref["nput"][p]])
        assert d["M"].tobytes() == ref["res1"]["M"][p].tobytes() and d["M_final"].tobytes() == ref["res2"]["M"][p].tobytes()
        assert d["hypothesis"] == ref["res1"]["hypothesis"][p] and d["inliers"] == ref["res1"]["inliers"][p]
        assert d["mask"].dtype == bool and np.array_equal(d["mask"], ref["mask"][p, :k].astype(bool))
        assert d["info"] == {"inliers": int(ref["res2"]["inliers"][p]), "refits": int(ref["res2"]["reserved"][p, 0]),
                             "ransac_inliers": int(ref["res2"]["reserved"][p, 1])}
    plain = bank.verify_pairs(pairs, "H", 8.0, hypotheses=300, seed=3, refit=2, guided_bound=6.0, max_match=1100, final_estimate=False)
    assert all(set(d) == {"matches", "M", "hypothesis", "inliers"} for d in plain)
    assert all(np.array_equal(d["matches"], e["matches"]) for d, e in zip(plain, got))
    assert bank.verify_pairs(np.zeros((0, 2), np.int32), "H", 8.0) == []


# ---- errors: nothing is launched, the matcher is as it was ---------------------------------------------------------------

def _raw(m, pairs, P, max_match=100, null=()):
    """The C call with chosen arguments NULL -> (return code, error text)."""
    hm = _hm()
    ab = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(ab)
    out, cnt = np.zeros((max(n, 1), max(max_match, 1), 2), np.int32), np.zeros(max(n, 1), np.int32)
    res = np.zeros(max(n, 1), hm.VERIFY_RESULT_DTYPE)
    arg = {"pairs_ab": ab.ctypes.data, "params": P.ctypes.data if P is not None else None, "out_pairs": out.ctypes.data,
           "out_counts": cnt.ctypes.data, "out": res.ctypes.data}
    for k in null:
        arg[k] = None
    rc = m.L.hess_matcher_verify_pairs(m.h, n, arg["pairs_ab"], arg["params"], max_match, arg["out_pairs"], arg["out_counts"],
                                       arg["out"], None, None)
    return rc, (m.L.hess_matcher_last_error(m.h) or b"").decode()


def _edit(P, path, value):
    Q = P.copy()
    if path[0] == "geom":
        g = Q["geom"]
        if path[1] == "reserved":
            g["reserved"][0, path[2]] = value
        else:
            g[path[1]] = value
        Q["geom"] = g
    elif path[0] == "reserved":
        Q["reserved"][0, path[1]] = value
    else:
        Q[path[0]] = value
    return Q


BAD_PARAMS = [
    (("geom", "model"), 3, "model"), (("geom", "model"), 0, "model"),
    (("geom", "hypotheses"), -1, "hypotheses"), (("geom", "hypotheses"), 65537, "hypotheses"),
    (("geom", "reserved", 0), 9, "refit"), (("geom", "reserved", 0), -1, "refit"),
    (("geom", "reserved", 1), 1, "reserved"), (("geom", "reserved", 3), 1, "reserved"),
    (("geom", "bound"), 0.0, "bound"), (("geom", "bound"), -1.0, "bound"), (("geom", "bound"), np.nan, "bound"),
    (("geom", "bound"), np.inf, "bound"),
    (("guided_bound",), -1.0, "guided_bound"), (("guided_bound",), np.nan, "guided_bound"), (("guided_bound",), np.inf, "guided_bound"),
    (("final_estimate",), 2, "final_estimate"), (("final_estimate",), -1, "final_estimate"),
    (("reserved", 0), 1, "reserved"), (("reserved", 2), 7, "reserved"),
]


def test_every_refusal_names_its_argument_and_leaves_the_matcher_as_it_was():
    from hessgpu_amd import _abi
    ARG, STATE, UNSUPPORTED = _abi.HESS_ERR_ARG, _abi.HESS_ERR_STATE, _abi.HESS_ERR_UNSUPPORTED
    sets, locs = vc.bank()
    m = _hm().Matcher(0)
    m.set_bank(sets)
    pairs, _ = vc.bank_pairs()
    P = _params("H")
    before = m.match_pairs(pairs)

    def unchanged():
        after = m.match_pairs(pairs)
        assert len(after) == len(before) and all(np.array_equal(x, y) for x, y in zip(before, after))

    rc, text = _raw(m, pairs, P)                                   # no locations
    assert rc == STATE and "verify_pairs" in text and "locations" in text
    unchanged()
    m.set_bank_locations(locs)
    good, _ = same(m, pairs, P, 100)
    m.set_bank_types([np.zeros(len(s), np.uint16) for s in sets])  # feature types: the guided call's refusal
    rc, text = _raw(m, pairs, P)
    assert rc == UNSUPPORTED and "guided matching with feature types is not built" in text
    m.set_bank_types(None)
    unchanged()
    for name in ("params", "out", "out_pairs", "out_counts", "pairs_ab"):
        rc, text = _raw(m, pairs, P, null=(name,))
        assert rc == ARG and name in text and "NULL" in text, (name, rc, text)
    for path, value, word in BAD_PARAMS:
        rc, text = _raw(m, pairs, _edit(P, path, value))
        assert rc == ARG and word in text, (path, value, rc, text)
    for bad in ([[0, len(sets)]], [[-1, 0]], [[0, 1], [len(sets) + 3, 1]]):
        rc, text = _raw(m, bad, P)
        assert rc == ARG and "outside the bank" in text, (bad, rc, text)
    rc, text = _raw(m, pairs, P, max_match=-1)
    assert rc == ARG and "max_match" in text
    rc, text = m.L.hess_matcher_verify_pairs(m.h, -1, None, None, 4, None, None, None, None, None), m.L.hess_matcher_last_error(m.h).decode()
    assert rc == ARG and "npairs" in text
    assert m.L.hess_matcher_verify_pairs(m.h, 0, None, None, 4, None, None, None, None, None) == 0      # npairs == 0 returns 0
    assert m.L.hess_matcher_verify_pairs(m.h, 0, None, P.ctypes.data, 4, None, None, None, None, None) == 0
    unchanged()
    same(m, pairs, P, 100, ref=good)                               # and the call itself answers as before
    m.close()


def test_scratch_overflow_of_one_pair_is_too_big_as_in_match_pairs():
    """One set of 800 000 zero rows against itself with mutual best: 3125 row blocks x 800 000 column partials exceed what a
    launch can address (2^31 - 1 entries).  Refused by the plan, before any allocation or launch."""
    from hessgpu_amd import _abi
    from hessgpu_amd.session import HessError
    n = 800000
    m = _hm().Matcher(0, max_sift=n)
    m.set_bank([np.zeros((n, 128), np.uint8), mc.descriptor_rows(3, np.random.RandomState(1))])
    m.set_bank_locations([np.zeros((n, 2), np.float32), np.zeros((3, 2), np.float32)])
    with pytest.raises(HessError) as e:
        m.match_pairs([[0, 0]], max_match=8)
    assert e.value.code == _abi.HESS_ERR_TOO_BIG
    rc, text = _raw(m, [[0, 0]], _params("H"), max_match=8)
    assert rc == _abi.HESS_ERR_TOO_BIG and "verify_pairs" in text and "scratch" in text
    assert len(m.match_pairs([[1, 1]], max_match=8)[0]) == 3      # the matcher still answers
    m.close()
