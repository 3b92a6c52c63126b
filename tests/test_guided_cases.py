"""The guided-matching tests' inputs, checked on the CPU (tests/guided_cases.py): for every case, threshold pair and
configuration of the GPU test no pair's gate decision is within float32 rounding of its threshold, the oracle equals an
independent float64 model, the result is not empty (named exceptions apart), and from 300 rows on it differs from the
unguided result, gates out true correspondences, holds matches that exist only through the 8-row-block leak, and tells
the reference's rules from the plausible wrong ones.  A GPU test that compares with the oracle on these inputs therefore
compares something."""
import numpy as np
import pytest

import guided_cases as gc
import matcher_cases as mc
from oracle_lib import oracle_match


def _oracle(c, h, f, dm, rm, mutual, max_match):
    return oracle_match(c.d1, c.d2, c.loc1, c.loc2, c.H, c.F, distmax=dm, ratiomax=rm, hdistmax=h, fdistmax=f,
                        mutual_best=mutual, max_match=max_match)


@pytest.mark.parametrize("n1,n2,geometry", gc.CASES)
def test_guided_inputs_oracle_equals_model_and_tell_the_rules_apart(n1, n2, geometry):
    cs = (n1, n2, geometry)
    label = f"{n1} x {n2} {geometry}"
    c = gc.case(*cs)
    big = cs in gc.BIG
    base = mc.Model(c.d1, c.d2)
    differs = {name: [] for name in gc.WRONG_RULES}
    largest = [0.0, 0.0]
    for k, (h, f) in enumerate(gc.pick_thresholds(*cs)):
        # a condition on the inputs, not a share to be tolerated
        pairs, mh, mf = gc.uncertain(c, h, f)
        largest = [max(largest[0], mh), max(largest[1], mf)]
        assert len(pairs) == 0, (label, h, f, "pairs within the rounding margin of a threshold", pairs[:5])
        # the finite thresholds are float32 numbers off the location grid
        for t in (h, f):
            assert t >= gc.OFF or (t == float(np.float32(t)) and t * 64 != round(t * 64)), (label, t)
        M = gc.GuidedModel(c, h, f, dot=base.dot)
        true_pass = M.passed[c.corr[:, 0], c.corr[:, 1]]
        leaks = (M.raw > 0) & ~M.passed
        print(f"{label} (hdistmax, fdistmax) = ({h:.7g}, {f:.7g}): {int(M.passed.sum())} pairs pass, true correspondences "
              f"{int(true_pass.sum())} pass / {int((~true_pass).sum())} fail, {int(leaks.sum())} gated-out pairs leak")
        if big:
            assert (~true_pass).any() and true_pass.any(), (label, h, f)
        for dm, rm, mutual in gc.CONFIGS:
            ref = _oracle(c, h, f, dm, rm, mutual, n1)
            got = M.match(dm, rm, mutual, n1)
            assert np.array_equal(ref, got), (label, h, f, dm, rm, mutual, mc.first_difference(ref, got))
            assert (len(ref) == 0) == ((cs, k) in gc.EMPTY), (label, k, dm, rm, mutual, len(ref))
            if len(ref) > 1:
                cut = len(ref) // 2                                  # a max_match below the match count
                assert np.array_equal(_oracle(c, h, f, dm, rm, mutual, cut), ref[:cut]), (label, h, f, dm, rm, mutual)
                assert np.array_equal(M.match(dm, rm, mutual, cut), ref[:cut])
            if big:
                assert not np.array_equal(ref, base.match(dm, rm, mutual, n1)), (label, h, f, dm, rm, mutual, "== unguided")
            if (dm, rm, mutual) == (2.0, 2.0, False) and h < gc.OFF:
                # every row with a candidate is returned: i' matches j through the leak alone, its copy i'' gets nothing
                rows = dict(map(tuple, ref))
                for name, i, ip, ipp, j in c.triples:
                    assert M.passed[i, j] and not M.passed[ip].any() and not M.passed[ipp].any(), (label, name)
                    assert base.dot[ip, j] > mc.CLAMP and leaks[ip, j], (label, name)
                    assert rows.get(ip) == j and ipp not in rows, (label, name, rows.get(ip), rows.get(ipp))
                if big:
                    assert len(c.triples) >= 2
        # the wrong rules; the largest case stops at a rule's first difference (a model of 4 Mi pairs takes a second)
        for name, kw in gc.WRONG_RULES.items():
            if n1 * n2 > mc.MATRIX_CORE_ABOVE and differs[name]:
                continue
            W = gc.GuidedModel(c, h, f, dot=base.dot, **kw)
            for dm, rm, mutual in (gc.CONFIGS[1], gc.CONFIGS[0], gc.CONFIGS[2]):
                if not np.array_equal(_oracle(c, h, f, dm, rm, mutual, n1), W.match(dm, rm, mutual, n1)):
                    differs[name].append((k, dm, rm, mutual))
                    if n1 * n2 > mc.MATRIX_CORE_ABOVE:
                        break
    print(f"{label}: largest rounding margin H {largest[0]:.1e}  F {largest[1]:.1e}; no uncertain pair")
    for name, where in differs.items():
        print(f"{label}: wrong rule '{name}' differs from the oracle at (threshold pair, distmax, ratiomax, mutual) = {where}")
        if big:
            assert where, f"{label}: the inputs do not tell '{name}' from the reference's rule in any configuration"


def test_leak_placements():
    """Where the triples sit: i | i' across a 4-row boundary inside one 8-row block; the copy in the next block, once in the
    same 64-row tile and once across the tile boundary; one triple in a ragged last block."""
    for n1, n2, geometry in gc.BIG:
        t = {name: (i, ip, ipp) for name, i, ip, ipp, j in gc.case(n1, n2, geometry).triples}
        for i, ip, ipp in t.values():
            assert i // 8 == ip // 8 != ipp // 8
        for name in "AB":
            i, ip, ipp = t[name]
            assert i // 4 != ip // 4 and ipp // 8 == ip // 8 + 1
        assert t["A"][2] // 64 == t["A"][1] // 64 and t["B"][2] // 64 == t["B"][1] // 64 + 1
    i, ip, ipp = next((i, ip, ipp) for name, i, ip, ipp, j in gc.case(300, 333, "affine").triples if name == "C")
    assert 300 % 8 and i // 8 == ip // 8 == 299 // 8 and ipp // 8 == 299 // 8 - 1
    i, ip, ipp = next((i, ip, ipp) for name, i, ip, ipp, j in gc.case(63, 129, "projective").triples if name == "C")
    assert 63 % 8 and i // 8 == ip // 8 == 62 // 8 and i // 4 != ip // 4


def test_the_vanishing_line_row_never_passes():
    for cs in gc.CASES:
        if cs[2] != "projective":
            continue
        c = gc.case(*cs)
        x2 = np.float32(c.H[2, 0]) * c.loc1[c.vanish, 0] + np.float32(c.H[2, 1]) * c.loc1[c.vanish, 1] + np.float32(c.H[2, 2])
        assert x2 == 0
        for h, f in ((gc.OFF, gc.OFF),) + gc.pick_thresholds(*cs):
            assert not gc.GuidedModel(c, h, f).passed[c.vanish].any()


@pytest.mark.parametrize("n1,n2,geometry", [c for c in gc.CASES if c[2] == "affine"])
def test_affine_h_gate_is_exact_in_float32(n1, n2, geometry):
    """Dyadic H, grid locations: the float32 H-gate quantities EQUAL the float64 ones, in either association."""
    c = gc.case(n1, n2, geometry)
    d0, d1, _ = gc.gates(c.loc1, c.loc2, c.H, c.F)
    H, x, y = c.H, c.loc1[:, 0], c.loc1[:, 1]
    assert H.dtype == x.dtype == np.float32
    for order in (lambda a, b, t: (a + b) + t, lambda a, b, t: a + (b + t)):
        q = [order(H[r, 0] * x, H[r, 1] * y, H[r, 2]) for r in range(3)]
        for k, d in enumerate((d0, d1)):
            d32 = np.abs((q[k] / q[2])[:, None] - c.loc2[None, :, k])
            assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d)


def test_one_matrix_alone_is_certain_too():
    """SiftMatchGPU::GetGuidedSiftMatch replaces a missing matrix by the identity with a bound of 1e20 (SiftMatch.cpp:663-676);
    the GPU test does that on these two cases with the case's H-only and F-only bounds: no pair is uncertain there either
    (under an identity H the vanishing-line row passes the H gate and meets the F bound)."""
    eye = np.eye(3, dtype=np.float32)
    for cs in ((300, 333, "projective"), (300, 333, "affine")):
        c, th = gc.case(*cs), gc.pick_thresholds(*cs)
        for H, F, h, f in ((c.H, eye, th[2][0], gc.OFF), (eye, c.F, gc.OFF, th[1][1])):
            v = dict(vars(c), H=H, F=F)
            pairs, _, _ = gc.uncertain(gc.SimpleNamespace(**v), h, f)
            assert len(pairs) == 0, (cs, h, f, pairs[:5])
