"""The feature-type cases of the matcher tests, checked on the CPU (tests/matcher_type_cases.py): the gated reference
(the oracle per class) equals the NumPy model per class in every configuration, and the inputs are such that a GPU test
passing on them means something -- gating changes results in a way that filtering the ungated result cannot reproduce,
placed ties are split across classes, and no expected result is empty."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import matcher_cases as mc
import matcher_type_cases as tc
from oracle_lib import oracle_match


def _model(a, b, max_match, distmax, ratiomax, mutual_best):
    return mc.model_match(a, b, distmax=distmax, ratiomax=ratiomax, mutual=mutual_best, max_match=max_match)


def _check(a, b, ta, tb, label):
    """gated_reference == the model per class, every configuration, whole and truncated -> the match counts."""
    n1 = max(len(a), 1)
    counts = []
    for dm, rm, mutual in mc.CONFIGS:
        kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual)
        ref = tc.gated_reference(a, b, ta, tb, max_match=n1, **kw)
        got = tc.gated(_model, a, b, ta, tb, max_match=n1, **kw)
        assert np.array_equal(ref, got), (label, dm, rm, mutual, mc.first_difference(ref, got))
        assert np.all(tc.classes(ta)[ref[:, 0]] == tc.classes(tb)[ref[:, 1]])
        assert np.all(np.diff(ref[:, 0]) > 0)
        if len(ref) > 1:
            cut = len(ref) // 2
            assert np.array_equal(tc.gated_reference(a, b, ta, tb, max_match=cut, **kw), ref[:cut]), (label, dm, rm, mutual)
        counts.append(len(ref))
    return counts


def _common_class(ta, tb):
    return bool(set(tc.classes(ta).tolist()) & set(tc.classes(tb).tolist()))


@pytest.mark.parametrize("kind", ("random", "position"))
def test_bank_gated_reference_equals_the_model_per_class(kind):
    sets, types = mc.bank_sets(), tc.bank_types(kind)
    pairs = [tuple(p) for p in mc.bank_all_pairs()]
    with ThreadPoolExecutor(4) as ex:
        counts = list(ex.map(lambda p: _check(sets[p[0]], sets[p[1]], types[p[0]], types[p[1]], (kind, p)), pairs))
    for p, c in zip(pairs, counts):
        if mc.BANK_ZERO_SET in p or not _common_class(types[p[0]], types[p[1]]):
            assert not any(c), (kind, p, c)              # an empty side (of every class) or the all-zero set: no match
        elif min(len(sets[p[0]]), len(sets[p[1]])) >= 255:
            # sets of a block or more share hundreds of correspondences per class: no configuration is empty
            assert all(c), (kind, p, c)
    for k in range(len(mc.CONFIGS)):
        assert sum(c[k] for c in counts) > 0


def test_saddle_assignment_is_the_ungated_match_and_highbits_is_random():
    sets = mc.bank_sets()
    sad, rnd, high = (tc.bank_types(k) for k in ("saddle", "random", "highbits"))
    for t, h in zip(rnd, high):
        assert np.array_equal(tc.classes(t), tc.classes(h)) and (len(h) == 0 or h.min() >= 0xfffc)
    for a, b in ((6, 7), (8, 6), (5, 3), (7, 7)):
        for dm, rm, mutual in mc.CONFIGS:
            kw = dict(distmax=dm, ratiomax=rm, mutual_best=mutual, max_match=len(sets[a]))
            ref = oracle_match(sets[a], sets[b], **kw)
            assert len(ref) > 0 and np.array_equal(tc.gated_reference(sets[a], sets[b], sad[a], sad[b], **kw), ref)
            assert np.array_equal(tc.gated_reference(sets[a], sets[b], high[a], high[b], **kw),
                                  tc.gated_reference(sets[a], sets[b], rnd[a], rnd[b], **kw))


def test_single_pair_cases_are_not_empty():
    cases = [(mc.single_pair(600, 700), tc.single_types(600, 700, k), (600, 700, k)) for k in tc.KINDS]
    cases += [(mc.single_pair(2100, 2050), tc.single_types(2100, 2050, k), (2100, 2050, k)) for k in ("random", "position")]
    cases += [(mc.straddle_sets(), tc.straddle_types(k), ("straddle", k)) for k in ("random", "position")]
    for (a, b), (ta, tb), label in cases:
        assert all(_check(a, b, ta, tb, label)), label


def test_gating_is_not_filtering_the_ungated_result():
    """Assignment "random", default thresholds, mutual best, the 90 ordered pairs of different sets: matches of the gated
    reference that the ungated result, filtered to same-class pairs, does not hold.  (348 when the cases were written.)"""
    sets, types = mc.bank_sets(), tc.bank_types("random")
    pairs = [(a, b) for a in range(len(sets)) for b in range(len(sets)) if a != b]
    assert len(pairs) == 90

    def one(p):
        a, b = p
        g = tc.gated_reference(sets[a], sets[b], types[a], types[b], max_match=max(len(sets[a]), 1))
        u = oracle_match(sets[a], sets[b], max_match=max(len(sets[a]), 1))
        u = u[tc.classes(types[a])[u[:, 0]] == tc.classes(types[b])[u[:, 1]]]
        return len(set(map(tuple, g)) - set(map(tuple, u)))

    with ThreadPoolExecutor(4) as ex:
        extra = list(ex.map(one, pairs))
    print("matches only gating finds:", sum(extra), "in", sum(1 for e in extra if e), "of 90 pairs")
    assert sum(extra) >= 300


def test_placed_ties_are_split_and_the_position_groups_sit_on_the_block():
    sets = mc.bank_sets()
    split = {k: tc.split_tie_groups(len(s), t) for k, (s, t) in enumerate(zip(sets, tc.bank_types("random")))}
    assert any(split.values()), split
    assert not any(tc.split_tie_groups(len(s), t) for s, t in zip(sets, tc.bank_types("saddle")))
    pos = [np.bincount(tc.classes(t), minlength=4).tolist() for t in tc.bank_types("position")]
    sizes = {n for c in pos for n in c}
    assert {255, 256, 257} <= sizes, pos
    assert sum(1 for c, s in zip(pos, sets) if len(s) >= 768 and c[0] == 0) == 1          # class 0 absent from one large set
    assert sum(1 for c in pos if c[3] > 0) == 1                                            # class 3 in one set only
    for kind in ("random", "highbits"):
        assert all(c > 0 for c in np.bincount(np.concatenate([tc.classes(t) for t in tc.bank_types(kind)]), minlength=4))
