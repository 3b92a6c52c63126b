"""64-d inputs for the matcher tests (a plain helper module, no tests in it): the cases of tests/matcher_cases.py and
tests/guided_cases.py folded to the shape of -half descriptors, and the definition of what a 64-d match IS.

  fold(s)    [n, 128] u8 -> [n, 64] u8: min(floor(hypot(s[:, 0::2], s[:, 1::2])), 255).  Equal rows stay equal (the placed
             ties stay ties, at the same positions: the plan does not depend on the descriptor length), an all-zero row
             stays all zero, and a row's L2 norm only falls (floor), so dot products stay under the 2^18 clamp.
  pad128(h)  h with 64 zero columns appended.  Dot products of unsigned bytes are unchanged by zero columns, so the result
             for 64-d sets is BY DEFINITION what the 128-d matcher and the CPU oracle return for pad128 of them: the same
             clamp, acos, ratio rule, tie order by column and row index, truncation.

tests/test_matcher_half_cases.py checks on the CPU that these inputs still match; tests/test_matcher_half_gpu.py runs them."""
import functools
from types import SimpleNamespace

import numpy as np

import guided_cases as gc
import matcher_cases as mc

DIM = 64


def fold(s):
    s = np.asarray(s)
    assert s.dtype == np.uint8 and s.ndim == 2 and s.shape[1] == 128
    h = np.hypot(s[:, 0::2].astype(np.float64), s[:, 1::2].astype(np.float64))
    return np.minimum(np.floor(h), 255).astype(np.uint8)


def pad128(h):
    h = np.asarray(h)
    assert h.dtype == np.uint8 and h.ndim == 2 and h.shape[1] == DIM
    return np.ascontiguousarray(np.concatenate([h, np.zeros_like(h)], 1))


@functools.lru_cache(maxsize=None)
def single_pair(n1, n2):
    a, b = mc.single_pair(n1, n2)
    return fold(a), fold(b)


@functools.lru_cache(maxsize=None)
def straddle_sets():
    a, b = mc.straddle_sets()
    return fold(a), fold(b)


@functools.lru_cache(maxsize=None)
def bank_sets():
    return [fold(s) for s in mc.bank_sets()]


@functools.lru_cache(maxsize=None)
def guided_case(n1, n2, geometry):
    """guided_cases.case with folded descriptors; locations, H, F, triples as they are."""
    c = gc.case(n1, n2, geometry)
    return SimpleNamespace(**dict(vars(c), d1=fold(c.d1), d2=fold(c.d2)))


def norms(s):
    return np.sqrt((s.astype(np.float64) ** 2).sum(1))


def distinct_rows(s):
    return len(np.unique(s, axis=0))
