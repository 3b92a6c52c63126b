"""Banks for the guided pair-list tests (hess_matcher_match_pairs_guided), built from guided_cases.case without changing it
(a plain helper module, no tests in it; tests/test_guided_pair_cases.py checks on the CPU oracle what the GPU tests rely on).

  case bank      the sets [d1, d2] of BANK_CASES back to back, pair k = (2k, 2k + 1), each with its own H, F and thresholds
  shifted        set 1 of a 300 x 333 case with SHIFT = 224 rows put in front: zero descriptors (score 0 never matches),
                 locations copied from rows k mod 300 (no new gate value arises).  Every match moves by (224, 0), and the leak
                 triples land on the seams of match_mfma_kernel: A on rows (251, 252, 260) -- the 8-row block that leaks ends
                 at row 255 and its silent copy sits in the next 256-row workgroup; B on (283, 284, 292); C on the ragged last
                 block of 524 rows
  trap           set 1 cut to its first TRAP_ROWS = 292 rows: its ragged last block 288..291 holds the over-clamp copy
                 i'' = 289 of triple C's column, and no row of that block passes.  The set that FOLLOWS it in the bank
                 starts with four locations equal to loc1[296], the row that passes with that column: a kernel that read the
                 locations of padded rows 292..295 from the next set would switch the block rule on and report (289, column)
"""
import functools
from types import SimpleNamespace

import numpy as np

import guided_cases as gc

BANK_CASES = ((1, 1, "identity"), (9, 65, "identity"), (63, 129, "projective"), (65, 63, "affine"), (300, 333, "affine"),
              (300, 333, "projective"))
assert set(BANK_CASES) <= set(gc.CASES)
SEAM_CASES = ((300, 333, "affine"), (300, 333, "projective"))
SHIFT = 224
TRAP_ROWS = 292


def case_bank(cases=BANK_CASES):
    """-> (descriptor sets, location sets, pairs [k, 2], cases): pair k is case k."""
    sets, locs = [], []
    for cs in cases:
        c = gc.case(*cs)
        sets += [c.d1, c.d2]
        locs += [c.loc1, c.loc2]
    pairs = np.array([(2 * k, 2 * k + 1) for k in range(len(cases))], np.int32)
    return sets, locs, pairs, cases


def geometry(cases, which):
    """-> H, F [n, 3, 3] and hdistmax, fdistmax [n] float32: case k at entry which[k] of its pick_thresholds."""
    H = np.stack([gc.case(*cs).H for cs in cases]).astype(np.float32)
    F = np.stack([gc.case(*cs).F for cs in cases]).astype(np.float32)
    t = [gc.pick_thresholds(*cs)[w] for cs, w in zip(cases, which)]
    return H, F, np.array([a for a, _ in t], np.float32), np.array([b for _, b in t], np.float32)


@functools.lru_cache(maxsize=None)
def shifted(n1, n2, geometry):
    c = gc.case(n1, n2, geometry)
    front = np.arange(SHIFT) % n1
    d1 = np.concatenate([np.zeros((SHIFT, 128), np.uint8), c.d1])
    loc1 = np.concatenate([c.loc1[front], c.loc1]).astype(np.float32)
    triples = [(name, i + SHIFT, ip + SHIFT, ipp + SHIFT, j) for name, i, ip, ipp, j in c.triples]
    return SimpleNamespace(**dict(vars(c), n1=n1 + SHIFT, d1=d1, loc1=loc1, triples=triples))


def shift_matches(ref):
    return (np.asarray(ref, np.int32).reshape(-1, 2) + np.array([SHIFT, 0], np.int32)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def trap(n1, n2, geometry):
    """-> namespace of the cut case (d1, loc1 of TRAP_ROWS rows), with follower (descriptors, locations: the set to put
    behind set 1 in the bank), appended (d1, loc1 of the cut set with the follower's first four rows appended as zero
    descriptors: what a kernel that reads on would see), and ipp, j: the over-clamp copy and its column."""
    c = gc.case(n1, n2, geometry)
    (name, i, ip, ipp, j), = [t for t in c.triples if t[0] == "C"]
    assert (i, ipp) == (296, 289) and TRAP_ROWS // 8 * 8 <= ipp < TRAP_ROWS <= i
    fd = c.d2[:16].copy()
    floc = c.loc2[:16].copy()
    floc[:4] = c.loc1[i]
    ad1 = np.concatenate([c.d1[:TRAP_ROWS], np.zeros((4, 128), np.uint8)])
    aloc1 = np.concatenate([c.loc1[:TRAP_ROWS], floc[:4]]).astype(np.float32)
    return SimpleNamespace(**dict(vars(c), n1=TRAP_ROWS, d1=c.d1[:TRAP_ROWS].copy(), loc1=c.loc1[:TRAP_ROWS].copy(),
                                  follower=(fd, floc), appended=(ad1, aloc1), ipp=ipp, j=j))
