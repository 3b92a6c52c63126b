"""Banks for the tests of hess_matcher_verify_pairs (a plain helper module, no tests in it): descriptor sets whose UNGUIDED
matches carry the planted geometry of a geom_cases case, built from the existing builders.

  pair_sets(name)  for geom_cases.case(name): set 1 = matcher_cases.descriptor_rows(len(loc1)), set 2 = fresh rows with
                   d2[j] = noisy(d1)[i] for every (i, j) of the case's matches; the locations are the case's loc1 / loc2.  The
                   match of set 1 against set 2 (distmax 0.7, ratiomax 0.8) then returns nearly all of the case's matches and
                   nothing else (tests/test_verify_cases.py holds that against matcher_cases.Model), so the estimator sees the
                   planted inliers and outliers.
  bank()           the sets of BANK_CASES back to back (case q: sets 2 q and 2 q + 1), then one EMPTY set
  bank_pairs()     every case's pair, a pair with the empty set on either side, and a pair (a, a)
  many_pairs(n)    n pairs cycling over the small cases of the same bank, forwards and reversed: positions of the same (a, b)
                   recur, so only seed + POSITION IN THE LIST can reproduce the chain
  big()            the sets of "H 5000" (more than 2048 matches: the estimator's LDS chunk seam), for Matcher(max_sift=5120)
"""
import functools

import numpy as np

import geom_cases as gcs
import matcher_cases as mc
import matcher_cases_half as mh

DISTMAX, RATIOMAX = 0.7, 0.8
MIN_SHARE = 0.95            # of a case's matches that the unguided match must return
SEED = 0                    # case q of geom_cases.CASES draws its rows from RandomState(SEED + q)

BANK_CASES = ("H 65", "H 300", "F 300", "H 1031", "H below k", "F below k", "H n = k", "F 65")
SMALL_CASES = ("H 65", "F 65", "H below k", "F below k")          # the 300-pair list cycles over these
BELOW = ("H below k", "F below k")
BIG_CASE = "H 5000"
BIG_MAX_SIFT = 5120


@functools.lru_cache(maxsize=None)
def pair_sets(name):
    """-> (d1 [rows of loc1, 128] u8, d2 [rows of loc2, 128] u8, loc1, loc2) of geom_cases.case(name)."""
    c = gcs.case(name)
    rng = np.random.RandomState(SEED + list(gcs.CASES).index(name))
    d1 = mc.descriptor_rows(len(c.loc1), rng)
    d2 = mc.descriptor_rows(len(c.loc2), rng)
    d2[c.matches[:, 1]] = mc.noisy(d1, rng)[c.matches[:, 0]]
    return d1, d2, c.loc1, c.loc2


def case_set(name):
    """The case's matches as a set of (i, j)."""
    return set(map(tuple, gcs.case(name).matches.tolist()))


@functools.lru_cache(maxsize=None)
def bank(half=False):
    """-> (sets, locs): case q of BANK_CASES is sets 2 q and 2 q + 1, the last set is empty.  half: folded to 64-d as
    matcher_cases_half does."""
    sets, locs = [], []
    for name in BANK_CASES:
        d1, d2, l1, l2 = pair_sets(name)
        sets += [d1, d2]
        locs += [l1, l2]
    sets.append(np.zeros((0, 128), np.uint8))
    locs.append(np.zeros((0, 2), np.float32))
    if half:
        sets = [mh.fold(s) for s in sets]
    return sets, locs


EMPTY_SET = 2 * len(BANK_CASES)


def pair_of(name):
    q = BANK_CASES.index(name)
    return (2 * q, 2 * q + 1)


def bank_pairs():
    """-> (pairs int32 [n, 2], names): the case pairs in BANK_CASES' order, then (empty, a set), (a set, empty) and (a, a)."""
    pairs = [pair_of(n) for n in BANK_CASES]
    names = list(BANK_CASES)
    a = pair_of("H 300")[0]
    pairs += [(EMPTY_SET, a), (a, EMPTY_SET), (a, a)]
    names += ["empty first", "empty second", "same set"]
    return np.array(pairs, np.int32), names


def many_pairs(n=300):
    """n pairs over SMALL_CASES: position p takes case p mod 4, reversed when (p // 4) is odd -- every (a, b) recurs."""
    out = []
    for p in range(n):
        a, b = pair_of(SMALL_CASES[p % len(SMALL_CASES)])
        out.append((b, a) if (p // len(SMALL_CASES)) % 2 else (a, b))
    return np.array(out, np.int32)


def big():
    """-> (sets, locs) of BIG_CASE alone: the pair is (0, 1)."""
    d1, d2, l1, l2 = pair_sets(BIG_CASE)
    return [d1, d2], [l1, l2]
