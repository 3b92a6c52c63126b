"""Inputs and an independent float64 model for the guided-matching tests (a plain helper module, no tests in it).

Guided matching (hess_matcher_match with H and F; MultiplyDescriptorG_Kernel, ProgramCU.cu:3565-3700) gates every pair
(i, j) by a homography box test and a Sampson error, and then adds the dot product to EVERY row of an 8-row block for
a column in which any row of the block passed (`good_count`, ProgramCU.cu:3648-3674).  A gated-out pair therefore holds
dot - 2^18, which is positive -- a candidate of its row and its column, a "leak" -- only for a dot product above the clamp.
Real descriptors and matcher_cases' rows (norm 490) never reach it, so the block rule is invisible on them: the rows
that show it are PLACED here.

  descriptors   matcher_cases.single_pair (correspondences, exact ties) plus placed over-clamp rows (norm 700)
  locations     set 1 random on a quarter-pixel grid in [0, 1000)^2; set 2 the true map of the corresponding row plus
                integer noise (a third within 1, a third within 24, a third within 64 pixels), snapped to the grid; the rest
                random
  geometries    "affine": H dyadic with third row (0, 0, 2), F = [t]x H with t = (1, 1/2, 0), dyadic as well: on grid
                locations every quantity of both gates up to the last division is exact in float32, whatever the order;
                "projective": third row (-2^-12, -2^-13, 1), F = [t]x H with a finite epipole, all nine entries non-zero,
                and one location of set 1 on the vanishing line (x2 == 0 exactly: nothing finite, the row never passes);
                "identity": H = I and F from a small rotation and a translation (the true map does not satisfy it exactly).
                No F is antisymmetric.
  leak triples  (i, i', i'', j): row i passes with column j; row i' of the same 8-row block sits far outside the image
                (it fails the H gate with every column), and holds the over-clamp descriptor of column j: its one
                candidate is the leak; i'' is a copy of i' in a neighbouring 8-row block, which gets nothing.
                A: (27, 28, 36)  i | i' straddle a 4-row boundary (the kernel's per-thread rows), all in one 64-row tile
                B: (59, 60, 68)  the same, the next block lies across the 64-row tile boundary
                C: the ragged last block of a set whose size is no multiple of 8, the copy in the block before
  thresholds    per case, next to the nominal (32, 16), (1e20, 16), (32, 1e20) and the tight (2.5, 1): each finite one is
                a float32 in a gap of the case's own gate values wide enough for the rounding margins, see pick_thresholds
  GuidedModel   matcher_cases.Model on max(raw, 0); the gates in float64 from the formulas; switches for WRONG rules
  uncertain     the pairs whose pass / fail could depend on float32 rounding; the tests assert there are none

Rounding margin: 8 x a first-order forward bound of the float32 evaluation (u = 2^-24 per operation, any association,
fused or not; `margins`).  The bound knows nothing of exactness, so it is applied to the affine cases as well, whose gate
values lie on a grid.  The projective geometry stops at 300 x 333: with the H gate off every one of the n1 n2 pairs
meets the F bound, and from some 10^5 pairs of a general F on no bound near 16 is clear of all their margins.

Largest margin per case (H gate: of d0 or d1 below 64 where the other axis may pass; F gate: of se below 32 among the
pairs that pass the H gate), as test_guided_cases.py prints it; no case has an uncertain pair:
  1 x 1 identity        H 2.9e-03  F 3.9e-02        65 x 63 affine          H 4.7e-03  F 6.1e-02
  7 x 70 projective     H 8.3e-03  F 1.5e-02        300 x 333 affine        H 5.0e-03  F 1.4e-01
  8 x 64 affine         H 4.5e-03  F 3.5e-02        300 x 333 projective    H 1.1e-02  F 5.0e-02
  9 x 65 identity       H 3.4e-03  F 3.7e-02        1000 x 877 affine       H 5.0e-03  F 6.3e-02
  63 x 129 projective   H 1.2e-02  F 5.9e-02        2049 x 2081 affine      H 5.1e-03  F 6.4e-02
"""
import functools
from types import SimpleNamespace

import numpy as np

import matcher_cases as mc

OFF = 1.0e20                      # a gate with this bound is switched off (SiftMatch.cpp:663-676)
GATED = -(1 << 18)                # what a gated-out pair starts from (ProgramCU.cu:3639-3646)
GRID = 4                          # locations are multiples of 1 / GRID
OVER_NORM = 700.0                 # placed rows: |v|^2 = 490 000 > 2^18 by far more than flooring to bytes takes away
U = 2.0 ** -24

# (n1, n2, geometry): sizes around the 4-row thread, 8-row block and 64 x 64 tile edges of match_dot_kernel, and one
# above 3 Mi products, where the guided call needs a larger score matrix than any unguided one on the same handle
CASES = ((1, 1, "identity"), (7, 70, "projective"), (8, 64, "affine"), (9, 65, "identity"), (63, 129, "projective"),
         (65, 63, "affine"), (300, 333, "affine"), (300, 333, "projective"), (1000, 877, "affine"), (2049, 2081, "affine"))
BIG = tuple(c for c in CASES if c[0] >= 300)
NOMINAL = ((32.0, 16.0), (OFF, 16.0), (32.0, OFF), (2.5, 1.0))       # both, F only, H only, tight
CONFIGS = (mc.CONFIGS[3], mc.CONFIGS[7], mc.CONFIGS[0])             # (2, 2) mutual and not, the defaults
assert CONFIGS == ((2.0, 2.0, True), (2.0, 2.0, False), (0.7, 0.8, True))
# the expected result is empty: (case, index into NOMINAL) -- the tight pair on two of the smallest sizes, and the 1 x 1
# case wherever the F gate is on (its one pair has a Sampson error of several hundred under the "identity" F)
EMPTY = {((1, 1, "identity"), 0), ((1, 1, "identity"), 1), ((1, 1, "identity"), 3), ((8, 64, "affine"), 3)}

VANISH = (3072.0, 2048.0)        # on the vanishing line of the projective H: -3072 / 4096 - 2048 / 8192 + 1 == 0


def _cross(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


@functools.lru_cache(maxsize=None)
def matrices(geometry):
    """-> (H, F) float32 [3, 3]; F = [t]x H, so a pair (x, H x) has Sampson error 0 (not for "identity", see above)."""
    if geometry == "affine":
        H = np.array([[2.5, 0.5, 49.0], [-0.25, 2.0, 33.0], [0.0, 0.0, 2.0]])
        F = _cross((1.0, 0.5, 0.0)) @ H          # [[0, 0, 1], [0, 0, -2], [-1.5, 1.75, 8.5]]
    elif geometry == "projective":
        H = np.array([[1.25, 0.25, 24.5], [-0.125, 1.0, 16.5], [-2.0 ** -12, -2.0 ** -13, 1.0]])
        F = _cross((300.0, -200.0, 1.0)) @ H / 256.0
    else:
        H = np.eye(3)
        c, s = np.cos(0.01), np.sin(0.01)
        F = _cross((1.0, 0.5, 0.002)) @ np.array([[c, -s, 3.0], [s, c, -2.0], [0.0, 0.0, 1.0]])
    H, F = H.astype(np.float32), F.astype(np.float32)
    assert not np.allclose(F, -F.T) and not np.array_equal(F, F.T)
    return H, F


def project(H, loc):
    """The map of H in float64: [n, 2] -> [n, 2]."""
    x = np.concatenate([loc, np.ones((len(loc), 1))], 1) @ H.astype(np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return x[:, :2] / x[:, 2:]


def _snap(v):
    return np.rint(v * GRID) / GRID


def _pool_index(s, pool):
    """For every row of s the pool row it is a noisy copy of (+-6 per byte), or -1."""
    a, p = s.astype(np.float64), pool.astype(np.float64)
    d2 = (a * a).sum(1)[:, None] + (p * p).sum(1)[None, :] - 2.0 * a @ p.T
    k = d2.argmin(1)
    return np.where(d2[np.arange(len(s)), k] <= 128 * 36, k, -1)


def _free(s, n):
    """Rows of a generated set that hold neither a placed tie nor the all-zero row."""
    groups = mc.tie_groups(n, tuple(range(1, mc.MAX_SPS + 1)))
    taken = {p for pos in groups.values() for p in pos} | set(np.flatnonzero(~s.any(1)).tolist())
    return [r for r in range(n) if r not in taken]


def leak_rows(n1):
    """-> [(name, i, i', i'')] for a set 1 of n1 rows (see the module docstring)."""
    out = []
    if n1 > 36:
        out.append(("A", 27, 28, 36))
    if n1 > 68:
        out.append(("B", 59, 60, 68))
    base = (n1 - 1) // 8 * 8
    if n1 % 8 >= 4 and base >= 80:      # rows base .. base + 3 at least; the last two hold ties: i, i' = base, base + 1
        out.append(("C", base, base + 1, base - 7))
    elif n1 % 8 >= 7 and base >= 48:    # 63 rows: 59 | 60 straddle the 4-row boundary, the copy in the block before
        out.append(("C", base + 3, base + 4, base - 4))
    return out


@functools.lru_cache(maxsize=None)
def case(n1, n2, geometry, seed=5):
    """-> namespace d1, d2 (u8 [n, 128]), loc1, loc2 (float32 [n, 2]), H, F, corr ([k, 2]: true correspondences (i, j)),
    triples ([(name, i, i', i'', j)]), vanish (row of set 1 on the vanishing line, or -1)."""
    a, b = mc.single_pair(n1, n2, seed)
    d1, d2 = a.copy(), b.copy()
    _, pool, _ = mc._case_material(seed, max(n1, n2))
    rng = np.random.RandomState(1000 * seed + n1 + n2)
    H, F = matrices(geometry)
    loc1 = rng.randint(0, 1000 * GRID, size=(n1, 2)) / GRID
    loc2 = rng.randint(0, 1000 * GRID, size=(n2, 2)) / GRID
    free1, free2 = _free(d1, n1), _free(d2, n2)
    # leak triples: descriptors and the far-away locations of i', i''
    triples = []
    over = mc.descriptor_rows(4, rng, norm=OVER_NORM)
    for k, (name, i, ip, ipp) in enumerate(leak_rows(n1)):
        assert {i, ip, ipp} <= set(free1), (n1, name)
        j = free2[len(free2) // 2 + 5 * k]
        d1[ip] = d1[ipp] = d2[j] = over[k]
        loc1[ip] = (6000.0 + 500 * k, 7000.0)
        loc1[ipp] = (6250.0 + 500 * k, 7000.0)
        triples.append((name, i, ip, ipp, j))
    vanish = -1
    if geometry == "projective":
        vanish = free1[2]
        loc1[vanish] = VANISH
    # true correspondences: rows that copy the same pool row; set 2 = the map of set 1 + noise
    k1, k2 = _pool_index(d1, pool), _pool_index(d2, pool)
    where1 = {int(k): i for i, k in enumerate(k1) if k >= 0}
    corr = np.array([(where1[int(k)], j) for j, k in enumerate(k2) if k >= 0 and int(k) in where1], np.int64).reshape(-1, 2)
    corr = corr[corr[:, 0] != vanish]
    amp = np.array([1, 24, 64])[rng.randint(0, 3, size=len(corr))]
    noise = np.rint((rng.rand(len(corr), 2) * 2 - 1) * amp[:, None])
    loc2[corr[:, 1]] = _snap(project(H, loc1[corr[:, 0]])) + noise
    for _, i, _, _, j in triples:
        loc2[j] = _snap(project(H, loc1[i:i + 1]))[0]
    loc1, loc2 = loc1.astype(np.float32), loc2.astype(np.float32)
    assert np.array_equal(loc1 * GRID, np.rint(loc1 * GRID)) and np.array_equal(loc2 * GRID, np.rint(loc2 * GRID))
    return SimpleNamespace(n1=n1, n2=n2, geometry=geometry, d1=d1, d2=d2, loc1=loc1, loc2=loc2, H=H, F=F, corr=corr,
                           triples=triples, vanish=vanish)


# ---- the gates in float64 -------------------------------------------------------------------------------------------

def _h1(loc):
    return np.concatenate([loc.astype(np.float64), np.ones((len(loc), 1))], 1)


def gates(loc1, loc2, H, F, h_on_set2=False, divide=True, f_transposed=False, sampson_terms=4):
    """-> d0, d1, se [n1, n2] float64 from the formulas (ProgramCU.cu:3618-3638): x = H x1, d = |x[:2] / x[2] - x2|;
    se = (x2^T F x1)^2 / ((F x1)_0^2 + (F x1)_1^2 + (F^T x2)_0^2 + (F^T x2)_1^2).  The switches state WRONG formulas."""
    Hm, Fm = H.astype(np.float64).reshape(3, 3), F.astype(np.float64).reshape(3, 3)
    if f_transposed:
        Fm = Fm.T
    p1, p2 = _h1(loc1), _h1(loc2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if h_on_set2:
            x = p2 @ Hm.T
            q = x[:, :2] / x[:, 2:] if divide else x[:, :2]
            d0, d1 = np.abs(q[None, :, 0] - p1[:, None, 0]), np.abs(q[None, :, 1] - p1[:, None, 1])
        else:
            x = p1 @ Hm.T
            q = x[:, :2] / x[:, 2:] if divide else x[:, :2]
            d0, d1 = np.abs(q[:, None, 0] - p2[None, :, 0]), np.abs(q[:, None, 1] - p2[None, :, 1])
        fx, ft = p1 @ Fm.T, p2 @ Fm
        s = fx[:, None, 0] * p2[None, :, 0] + fx[:, None, 1] * p2[None, :, 1] + fx[:, None, 2]
        den = (fx[:, 0] ** 2 + fx[:, 1] ** 2)[:, None] + (ft[:, 0] ** 2 + (ft[:, 1] ** 2 if sampson_terms == 4 else 0.0))[None, :]
        se = s * s / den
    return d0, d1, se


def margins(loc1, loc2, H, F):
    """-> m_d0, m_d1, m_se [n1, n2]: 8 x a first-order bound of |float32 result - exact result|.  Every sum of three terms
    a + b + c (products included, fused or not, any association) is within 3 u (|a| + |b| + |c|) of the exact one; a
    quotient, a difference and a square add u times their own size; errors of operands propagate with the derivative."""
    Hm, Fm = np.abs(H.astype(np.float64).reshape(3, 3)), np.abs(F.astype(np.float64).reshape(3, 3))
    H64, F64 = H.astype(np.float64).reshape(3, 3), F.astype(np.float64).reshape(3, 3)
    p1, p2 = _h1(loc1), _h1(loc2)
    a1, a2 = np.abs(p1), np.abs(p2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, ex = p1 @ H64.T, 3 * U * (a1 @ Hm.T)                              # [n1, 3] and its error
        q = x[:, :2] / x[:, 2:]
        eq = U * np.abs(q) + ex[:, :2] / np.abs(x[:, 2:]) + np.abs(q) * ex[:, 2:] / np.abs(x[:, 2:])
        d = [np.abs(q[:, None, k] - p2[None, :, k]) for k in (0, 1)]
        md = [8 * (eq[:, None, k] + U * d[k]) for k in (0, 1)]
        fx, efx = p1 @ F64.T, 3 * U * (a1 @ Fm.T)                            # [n1, 3]
        ft, eft = p2 @ F64, 3 * U * (a2 @ Fm)                                # [n2, 3]
        terms = np.abs(fx[:, None, 0]) * a2[None, :, 0] + np.abs(fx[:, None, 1]) * a2[None, :, 1] + np.abs(fx[:, None, 2])
        s = fx[:, None, 0] * p2[None, :, 0] + fx[:, None, 1] * p2[None, :, 1] + fx[:, None, 2]
        es = 3 * U * terms + efx[:, None, 0] * a2[None, :, 0] + efx[:, None, 1] * a2[None, :, 1] + efx[:, None, 2]
        num, enum = s * s, 2 * np.abs(s) * es + U * s * s
        den = (fx[:, 0] ** 2 + fx[:, 1] ** 2)[:, None] + (ft[:, 0] ** 2 + ft[:, 1] ** 2)[None, :]
        eden = 4 * U * den + (2 * np.abs(fx[:, 0]) * efx[:, 0] + 2 * np.abs(fx[:, 1]) * efx[:, 1])[:, None] \
            + (2 * np.abs(ft[:, 0]) * eft[:, 0] + 2 * np.abs(ft[:, 1]) * eft[:, 1])[None, :]
        se = num / den
        mse = 8 * (enum / den + se * eden / den + U * se)
    return md[0], md[1], mse


def _f32(t):
    return float(np.float32(t))


def uncertain(c, hdistmax, fdistmax):
    """-> (pairs [k, 2] whose pass / fail may depend on float32 rounding, largest H margin, largest F margin among the
    pairs looked at).  d0 (d1) counts where it is within its margin of hdistmax and the other axis may pass; se where it is
    within its margin of fdistmax and the pair passes the H gate.  A non-finite quantity fails on both sides and has no
    margin: x2 == 0 is exact on the grid (the third rows are dyadic), and nothing else is near a division by zero."""
    h, f = _f32(hdistmax), _f32(fdistmax)
    d0, d1, se = gates(c.loc1, c.loc2, c.H, c.F)
    m0, m1, ms = margins(c.loc1, c.loc2, c.H, c.F)
    fin = np.isfinite(d0) & np.isfinite(d1)
    with np.errstate(invalid="ignore"):
        may0, may1 = fin & (d0 < h + m0), fin & (d1 < h + m1)
        bad_h = (may1 & (np.abs(d0 - h) <= m0)) | (may0 & (np.abs(d1 - h) <= m1))
        pass_h = fin & (d0 < h) & (d1 < h)
        bad_f = pass_h & np.isfinite(se) & (np.abs(se - f) <= ms)
        near = pass_h & np.isfinite(se) & (se < 2 * min(f, 32.0))
    mh = max(float(m0[may1 & (d0 < 2 * min(h, 64.0))].max(initial=0)), float(m1[may0 & (d1 < 2 * min(h, 64.0))].max(initial=0)))
    return np.argwhere(bad_h | bad_f), mh, float(ms[near].max(initial=0))


def _pick(values, margin, nominal):
    """A float32 threshold near `nominal` that no value is within its margin of: the middle of the widest clear gap whose
    middle lies within 10 % of nominal."""
    lo, hi = 0.9 * nominal, 1.1 * nominal
    keep = (values + margin > 0.8 * nominal) & (values - margin < 1.2 * nominal)
    v, m = values[keep], margin[keep]
    order = np.argsort(v - m)
    a, b = np.concatenate([[0.8 * nominal], (v + m)[order]]), np.concatenate([(v - m)[order], [1.2 * nominal]])
    top = np.maximum.accumulate(a)                      # the end of everything that starts before gap k
    mid, width = (top + b) / 2, b - top
    width = np.where((mid >= lo) & (mid <= hi), width, -1.0)
    k = int(width.argmax())
    assert width[k] > 16 * U * nominal, ("no clear gap near", nominal)
    t = _f32(mid[k])
    if t * 64 == round(t * 64):                         # off the grid of the exact cases as well
        t = _f32(mid[k] + 0.15 * width[k])
    return t


@functools.lru_cache(maxsize=None)
def pick_thresholds(n1, n2, geometry):
    """-> ((hdistmax, fdistmax), ...) for NOMINAL: each finite bound moved into a gap of the case's gate values.  The H bound
    looks at d0 where d1 may pass and at d1 where d0 may pass; the F bound at the pairs that pass the chosen H bound."""
    c = case(n1, n2, geometry)
    d0, d1, se = gates(c.loc1, c.loc2, c.H, c.F)
    m0, m1, ms = margins(c.loc1, c.loc2, c.H, c.F)
    fin = np.isfinite(d0) & np.isfinite(d1)
    out = []
    for hn, fn in NOMINAL:
        h = hn
        if hn < OFF:
            with np.errstate(invalid="ignore"):
                s0, s1 = fin & (d1 < 1.3 * hn), fin & (d0 < 1.3 * hn)
            h = _pick(np.concatenate([d0[s0], d1[s1]]), np.concatenate([m0[s0], m1[s1]]), hn)
        f = fn
        if fn < OFF:
            with np.errstate(invalid="ignore"):
                ph = fin & (d0 < _f32(h)) & (d1 < _f32(h)) & np.isfinite(se)
            f = _pick(se[ph], ms[ph], fn)
        out.append((h, f))
    return tuple(out)


# ---- the model ------------------------------------------------------------------------------------------------------

WRONG_RULES = {
    "block of 4 rows": dict(block=4), "block of 64 rows": dict(block=64), "no leak": dict(leak=False),
    "Euclidean H gate": dict(euclid=True), "F transposed": dict(f_transposed=True), "H applied to set 2": dict(h_on_set2=True),
    "projection without the division": dict(divide=False), "three-term Sampson denominator": dict(sampson_terms=3),
}


class GuidedModel(mc.Model):
    """matcher_cases.Model with the dot matrix replaced by what the guided multiply stores: pass = (d0 < h) & (d1 < h) &
    (se < f), anything non-finite fails; blockgood[i // 8, j] = any pass in the block; raw = (0 where pass else -2^18) +
    (dot where blockgood else 0); rows and columns then work on max(raw, 0) (ProgramCU.cu:3684-3687: the column partials
    start from 0 and replace on '>').  block, leak, euclid and the switches of `gates` state WRONG rules with the same
    code.  dot: the integer products, to share them among several models of one case."""

    def __init__(self, c, hdistmax, fdistmax, dot=None, block=8, leak=True, euclid=False, **gate_switches):
        if dot is None:
            super().__init__(c.d1, c.d2)
            dot = self.dot
        self.n1, self.n2 = dot.shape
        h, f = _f32(hdistmax), _f32(fdistmax)
        d0, d1, se = gates(c.loc1, c.loc2, c.H, c.F, **gate_switches)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = np.isfinite(d0) & np.isfinite(d1) & np.isfinite(se)
            ok &= (np.sqrt(d0 * d0 + d1 * d1) < h) if euclid else ((d0 < h) & (d1 < h))
            ok &= se < f
        self.passed = ok
        if leak:
            nb = -(-self.n1 // block)
            pad = np.zeros((nb * block, self.n2), bool)
            pad[:self.n1] = ok
            good = np.repeat(pad.reshape(nb, block, self.n2).any(1), block, axis=0)[:self.n1]
            self.raw = np.where(ok, 0, GATED) + np.where(good, dot, 0)
        else:
            self.raw = np.where(ok, dot, GATED)
        self.plain = dot
        self.dot = np.maximum(self.raw, 0)
