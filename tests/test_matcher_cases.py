"""The matcher tests' inputs, checked on the CPU (tests/matcher_cases.py): for every case and configuration of the GPU tests
the oracle equals an independent NumPy model, its result is not empty, the inputs tell the reference's tie rules from the
plausible wrong ones, and the bytes cover what the signed-byte matrix-core path has to correct.  A GPU test that compares
with the oracle on these inputs therefore compares something."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import matcher_cases as mc
from oracle_lib import oracle_match

SINGLE = mc.MATRIX_CORE_SIZES + mc.SMALL_PATH_SIZES

# the wrong rules: name -> switches of the model
WRONG_RULES = {"lowest class": dict(row_rule="class"), "lowest column": dict(row_rule="col"),
               "second ignores duplicates": dict(second_counts_duplicates=False), "highest row": dict(col_rule="high")}


def _oracle(a, b, dm, rm, mutual, max_match):
    return oracle_match(a, b, distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=max_match)


def _check_pair(a, b, label, floor=True):
    """oracle == model in every configuration (and truncated); the match floor; -> {wrong rule: configurations in which it
    differs from the oracle}."""
    n1 = max(len(a), 1)
    M = mc.Model(a, b)
    assert M.dot.size == 0 or M.dot.max() < mc.CLAMP, (label, "a dot product reaches the clamp")
    differs = {name: [] for name in WRONG_RULES}
    for dm, rm, mutual in mc.CONFIGS:
        ref = _oracle(a, b, dm, rm, mutual, n1)
        got = M.match(dm, rm, mutual, n1)
        assert np.array_equal(ref, got), (label, dm, rm, mutual, mc.first_difference(ref, got))
        if floor and (dm, rm) == (0.7, 0.8):
            # a condition on the inputs, against the oracle alone: at least a quarter of the smaller set matches
            assert 4 * len(ref) >= min(len(a), len(b)), (label, mutual, len(ref))
        if len(ref) > 1:
            cut = len(ref) // 2                                  # a max_match below the match count
            assert np.array_equal(_oracle(a, b, dm, rm, mutual, cut), M.match(dm, rm, mutual, cut)), (label, dm, rm, mutual)
            assert np.array_equal(ref[:cut], M.match(dm, rm, mutual, cut))
        for name, kw in WRONG_RULES.items():
            if not np.array_equal(ref, M.match(dm, rm, mutual, n1, **kw)):
                differs[name].append((dm, rm, mutual))
    return differs


@pytest.mark.parametrize("n1,n2", SINGLE)
def test_single_pair_inputs_oracle_equals_model_and_tell_the_rules_apart(n1, n2):
    a, b = mc.single_pair(n1, n2)
    differs = _check_pair(a, b, (n1, n2))
    for name, where in differs.items():
        print(f"{n1} x {n2}: wrong rule '{name}' differs from the oracle at (distmax, ratiomax, mutual) = {where}")
        assert where, f"{n1} x {n2}: the inputs do not tell '{name}' from the reference's rule in any configuration"
    # the row rules can only show where tied rows pass: ratiomax > 1
    assert all(rm > 1 for _, rm, _ in differs["lowest class"] + differs["lowest column"])


def test_threshold_straddling_pair():
    s1, s2 = mc.straddle_sets()
    assert (len(s1) - 1) * len(s2) == mc.MATRIX_CORE_ABOVE and len(s1) * len(s2) > mc.MATRIX_CORE_ABOVE
    for a in (s1[:-1], s1):
        differs = _check_pair(a, s2, ("straddle", len(a)))
        assert all(differs.values()), differs


def test_bank_inputs_every_ordered_pair():
    sets = mc.bank_sets()
    assert [len(s) for s in sets] == list(mc.BANK_SIZES) + [300] and not sets[mc.BANK_ZERO_SET].any()
    pairs = mc.bank_all_pairs()
    assert len(pairs) > mc.BANK_CHUNK                                      # more than one chunk
    assert {tuple(p) for p in mc.bank_big_chunk_pairs()} <= {tuple(p) for p in pairs}

    def one(p):
        a, b = sets[p[0]], sets[p[1]]
        if len(a) == 0 or len(b) == 0 or mc.BANK_ZERO_SET in p:
            # the named exceptions: an empty side or the all-zero set gives exactly no match, in every configuration
            for dm, rm, mutual in mc.CONFIGS:
                assert len(_oracle(a, b, dm, rm, mutual, 4096)) == 0 and len(mc.model_match(a, b, distmax=dm, ratiomax=rm, mutual=mutual)) == 0
            return None
        return _check_pair(a, b, ("bank", tuple(p)))

    with ThreadPoolExecutor(4) as ex:
        results = list(ex.map(one, [tuple(p) for p in pairs]))
    total = {name: 0 for name in WRONG_RULES}
    for p, differs in zip(pairs, results):
        if differs is None:
            continue
        for name, where in differs.items():
            total[name] += len(where)
            if min(len(sets[p[0]]), len(sets[p[1]])) >= 1500:      # every pair of the large sets tells every rule apart
                assert where, (tuple(p), name)
    print("bank: configurations (over all pairs) in which each wrong rule differs from the oracle:", total)
    assert all(total.values())


def test_geometry_of_the_cases():
    """What the sizes were chosen for, from the host's plan restated in matcher_cases (hess_match.hip: hess_matcher_match,
    pair_seg, chunk_sps)."""
    assert mc.single_plan(2049, 2081) == (9, 17, 17, 1)
    assert mc.single_plan(255, 12337) == (1, 97, 97, 1) and mc.single_plan(257, 12289) == (2, 97, 97, 1)
    assert mc.single_plan(12001, 263) == (47, 3, 3, 1)
    assert mc.single_plan(300, 33000) == (2, 258, 86, 3)                  # several super tiles per segment
    for n1, n2 in mc.MATRIX_CORE_SIZES:
        assert n1 * n2 > mc.MATRIX_CORE_ABOVE
    for n1, n2 in mc.SMALL_PATH_SIZES:
        assert n1 * n2 <= mc.MATRIX_CORE_ABOVE
    # the bank's large chunk reaches the cap; 25 super tiles -> 2 segments of 13 (tiles 0..51), 30 -> 2 of 15 (tiles 0..59)
    sizes = [(mc.BANK_SIZES[a], mc.BANK_SIZES[b]) for a, b in mc.bank_big_chunk_pairs()]
    assert len(sizes) == mc.BANK_CHUNK and mc.chunk_sps(sizes) == mc.MAX_SPS
    assert mc.pair_seg(25, 15) == (2, 13) and mc.pair_seg(30, 15) == (2, 15) and mc.pair_seg(12, 15) == (1, 12)
    # ... and the sets hold ties in the first and the last tile of a segment of that geometry, tile 59 included
    g3100, g3825 = (mc.tie_groups(n, (1, 2, 6, mc.MAX_SPS)) for n in (3100, 3825))
    assert g3100["segment_first_last_tile_sps13"] == (17, 13 * 128 - 32 + 18)
    assert g3100["last_segment_first_last_tile_sps13"] == (13 * 128 + 1, 3072 + 2)
    assert g3825["segment_first_last_tile_sps15"] == (17, 59 * 32 + 18)
    assert g3825["last_segment_first_last_tile_sps15"] == (1920 + 1, 1920 + 59 * 32 + 2)
    # the all-pairs call: which caps its chunks get (the ties for 1, 2, 6 super tiles per segment cover them)
    allp = [(len(mc.bank_sets()[a]), len(mc.bank_sets()[b])) for a, b in mc.bank_all_pairs()]
    caps = {mc.chunk_sps(allp[k:k + mc.BANK_CHUNK]) for k in range(0, len(allp), mc.BANK_CHUNK)}
    print("all-pairs chunks: super tiles per segment at most", sorted(caps))
    assert caps <= {1, 2, 6}
    # the tie groups every case of at least 300 rows carries
    for n in (300, 1500, 2081, 12289, 33000):
        g = mc.tie_groups(n, (1,))
        for name in ("tile_classes_1_2", "tile_classes_3_16", "class_5_tiles_1_3", "first_last_column", "rows_16_apart",
                     "rows_32_apart", "rows_64_apart", "rows_256_apart", "last_row_early_row", "class_6_two_segments_sps1",
                     "classes_9_10_two_segments_sps1", "three_copies_sps1"):
            assert name in g, (n, name)
        pos = [p for v in g.values() for p in v]
        assert len(pos) == len(set(pos))


def test_bytes_cover_the_signed_byte_correction():
    """Every generated set of 255 rows or more has a byte of 255 and at least 2 % of its bytes >= 128: the matrix-core path
    multiplies bytes biased by -128 and corrects the sum (rfix / cfix in hess_match.hip)."""
    sets = [s for n1, n2 in SINGLE for s in mc.single_pair(n1, n2)] + list(mc.straddle_sets())
    sets += [s for k, s in enumerate(mc.bank_sets()) if k != mc.BANK_ZERO_SET]
    checked = 0
    for s in sets:
        if len(s) >= 255:
            assert s.max() == 255 and (s >= 128).mean() >= 0.02, (len(s), s.max(), (s >= 128).mean())
            assert (s.astype(np.int64) ** 2).sum(1).max() < 512 * 512
            checked += 1
    assert checked >= 20
