"""Feature types for the matcher tests (a plain helper module, no tests in it): the definition of the gated match and
the type assignments for the sets of tests/matcher_cases.py.

The gated match G(A, B, tA, tB) -- hess_matcher_set_types / _bank_set_types in include/hess_abi.h -- is BY DEFINITION the
existing matcher on derived inputs, so the CPU oracle checks it bit for bit as it stands:

  1. class of a feature = type & 3; per class c, A_c = the rows of A of class c in ascending original index, B_c
     likewise; M_c = the ungated match of (A_c, B_c), same thresholds, no limit (nothing for an empty side);
  2. every M_c mapped back to original indices; the union in ascending original row of A;
  3. the first max_match.

gated_reference does exactly that on oracle_match; gated(match, ...) does it on any ungated matcher (the NumPy model of
matcher_cases, the oracle on zero-padded 64-d rows).

Assignments (types_for(sets, kind) -> one u16 array per set):
  "random"    RandomState(3).choice(4, p=[.3, .3, .35, .05]), set after set: tie groups and correspondences are split
  "saddle"    every row class 2: G must equal the ungated result, so every placed tie of matcher_cases stays on its seam
  "position"  class by position: groups of exactly 255, 256 and 257 rows (one below, on and above the 256-row block a group
              is padded to); class 0 absent from one set, class 3 present in one set only
  "highbits"  the random assignment | 0xfffc: must behave as its low two bits
"""
import functools

import numpy as np

import matcher_cases as mc
from oracle_lib import oracle_match

KINDS = ("random", "saddle", "position", "highbits")
P_RANDOM = (.3, .3, .35, .05)


def classes(t):
    return np.asarray(t).astype(np.int64) & 3


def gated(match, a, b, ta, tb, max_match=4096, **kw):
    """The three steps of the definition on `match(a_c, b_c, max_match=rows of a_c, **kw)` -> [k, 2] int32."""
    ca, cb = classes(ta), classes(tb)
    assert len(ca) == len(a) and len(cb) == len(b)
    parts = []
    for c in range(4):
        ia, ib = np.flatnonzero(ca == c), np.flatnonzero(cb == c)
        if len(ia) == 0 or len(ib) == 0:
            continue
        m = np.asarray(match(np.ascontiguousarray(a[ia]), np.ascontiguousarray(b[ib]), max_match=len(ia), **kw))
        if len(m):
            parts.append(np.stack([ia[m[:, 0]], ib[m[:, 1]]], 1))
    if not parts:
        return np.zeros((0, 2), np.int32)
    out = np.concatenate(parts)
    out = out[np.argsort(out[:, 0], kind="stable")]
    assert len(np.unique(out[:, 0])) == len(out)          # a row has one class
    return out[:max_match].astype(np.int32)


def gated_reference(a, b, ta, tb, distmax=0.7, ratiomax=0.8, mutual_best=True, max_match=4096):
    return gated(oracle_match, a, b, ta, tb, max_match=max_match, distmax=distmax, ratiomax=ratiomax, mutual_best=mutual_best)


def _by_position(n, k):
    i = np.arange(n)
    if n < 768:
        return (i + k) % 3
    t = np.full(n, 2)
    v = k % 3
    if v == 0:        # class 1: 255 rows, class 0: 256 rows, class 2: the rest
        t[:255], t[255:511] = 1, 0
    elif v == 1:      # class 2: 257 rows, class 1: the rest; class 0 absent
        t[257:] = 1
    else:             # class 3: 255 rows (this variant only), class 0: 256, class 1: 257, class 2: the rest
        t[:255], t[255:511], t[511:768] = 3, 0, 1
    return t


def types_for(sets, kind):
    """One u16 array of types per set of `sets`."""
    assert kind in KINDS
    if kind == "saddle":
        out = [np.full(len(s), 2) for s in sets]
    elif kind == "position":
        out = [_by_position(len(s), k) for k, s in enumerate(sets)]
    else:
        rng = np.random.RandomState(3)
        out = [rng.choice(4, size=len(s), p=P_RANDOM) for s in sets]
        if kind == "highbits":
            out = [t | 0xfffc for t in out]
    return [np.asarray(t).astype(np.uint16) for t in out]


@functools.lru_cache(maxsize=None)
def bank_types(kind):
    return types_for(mc.bank_sets(), kind)


@functools.lru_cache(maxsize=None)
def single_types(n1, n2, kind):
    return types_for(mc.single_pair(n1, n2), kind)


@functools.lru_cache(maxsize=None)
def straddle_types(kind):
    return types_for(mc.straddle_sets(), kind)


def split_tie_groups(n, types, sps_list=(1, 2, 6, mc.MAX_SPS)):
    """The placed tie groups of a set of n rows whose members do not all have one class."""
    c = classes(types)
    return [name for name, pos in mc.tie_groups(n, sps_list).items() if len({int(c[p]) for p in pos}) > 1]
