"""Inputs and a float64 model for the tests of the estimator's refit (include/hess_abi.h, step 6; a plain helper module, no
tests in it), built from the pieces of geom_cases.

  normal64      the normalisation and the 9 x 9 normal matrix N of a set of correspondences, with its eigenvalues
  moments       the moment sums that hessgpu_amd/csrc/hess_geom_refit.h takes, in its layout (for tests/geom_refit_main.cpp)
  candidate64   step 6 b-d: geom_cases.solve in float64 on the inliers (on more than k points it is the least-squares DLT: the
                same normalisation, the right singular vector of the smallest singular value of the design matrix), back in
                pixel coordinates, then finish64 (rank 2 for F there, as the rule says, and unit norm), with the rule's sign
  step64        one iteration from a mask and a matrix: the candidate, kappa = lambda_9 / (lambda_2 - lambda_1), the interval
                [lo, hi] that holds the float32 gate's count on the candidate (decide64 and its rounding band) and the verdict
                "accept", "reject" or "undecided" (the interval straddles the count before); or the reason to stop
  chain64       the whole rule from the float64 model of steps 1-5
  noisy         geom_cases.scene with N(0, sigma) on the planted inliers' second points; NOISY names the chosen (model, n,
                sigma, seed), QUALITY those whose refit at least halves the error, REJECTED the one whose chain ends in a
                discarded candidate (test_refit_cases.py checks the conditions on the CPU)
  rms           the RMS gate value of a matrix on the noise-free planted inliers
"""
import functools
from types import SimpleNamespace

import numpy as np

import geom_cases as g

T_NOISY = 256
MAX_KAPPA = 1.0e6
TOL = 8 * 2.0 ** -24          # 2^-24: one float32 rounding of a unit-norm matrix; 8: the factor of the estimator's own tests


def _sym(i, j):
    a, b = min(i, j), max(i, j)
    return b if a == 0 else (2 + b if a == 1 else 5)


def _rows(model, a, b):
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    z, o = np.zeros_like(x), np.ones_like(x)
    if model == "H":
        return np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], 1)])
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, o], 1)


def normal64(model, p1, p2):
    """-> namespace c1, s1, c2, s2 (centroids, scales), a, b (normalised points), N [9, 9], lam (ascending eigenvalues), x (the
    unit eigenvector of lam[0]), kappa = lam[8] / (lam[1] - lam[0]); ok False: a mean distance is zero or not finite."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1, c2 = p1.mean(0), p2.mean(0)
    d1, d2 = np.sqrt(((p1 - c1) ** 2).sum(1)).mean(), np.sqrt(((p2 - c2) ** 2).sum(1)).mean()
    if not (np.isfinite(d1) and np.isfinite(d2) and d1 > 0 and d2 > 0):
        return SimpleNamespace(ok=False)
    s1, s2 = np.sqrt(2) / d1, np.sqrt(2) / d2
    a, b = (p1 - c1) * s1, (p2 - c2) * s2
    A = _rows(model, a, b)
    N = A.T @ A
    lam, vec = np.linalg.eigh(N)
    with np.errstate(divide="ignore"):
        kappa = lam[8] / (lam[1] - lam[0])
    return SimpleNamespace(ok=True, c1=c1, s1=s1, c2=c2, s2=s2, a=a, b=b, N=N, lam=lam, x=vec[:, 0], kappa=float(kappa))


def moments(model, a, b):
    """The moment sums of normalised points a -> b in the layout of hess_geom_refit.h: H 24 (P, U, V, W), F 36."""
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    o = np.ones_like(x)
    pp = np.stack([x * x, x * y, x, y * y, y, o], 1)
    if model == "H":
        return np.concatenate([pp.sum(0), (u[:, None] * pp).sum(0), (v[:, None] * pp).sum(0), ((u * u + v * v)[:, None] * pp).sum(0)])
    qq = np.stack([u * u, u * v, u, v * v, v, o], 1)
    return (qq[:, :, None] * pp[:, None, :]).sum(0).reshape(36)


def denormalise64(model, x, nm):
    """The eigenvector x (normalised coordinates) as the returned matrix: pixel coordinates, rank 2 for F, unit norm."""
    T1 = np.array([[nm.s1, 0, -nm.s1 * nm.c1[0]], [0, nm.s1, -nm.s1 * nm.c1[1]], [0, 0, 1]])
    T2 = np.array([[nm.s2, 0, -nm.s2 * nm.c2[0]], [0, nm.s2, -nm.s2 * nm.c2[1]], [0, 0, 1]])
    X = np.asarray(x, np.float64).reshape(3, 3)
    return g.finish64(model, np.linalg.inv(T2) @ X @ T1 if model == "H" else T2.T @ X @ T1)


def candidate64(model, p1, p2, mask, prev):
    """-> the float64 candidate of the correspondences in `mask`, with the sign for which sum C prev >= 0."""
    C = g.finish64(model, g.solve(model, p1[mask], p2[mask], np.float64, rank2=False))
    return C if (C * np.asarray(prev, np.float64)).sum() >= 0 else -C


def step64(model, p1, p2, mask, prev, bound):
    """One iteration of the rule from (prev, mask) -> namespace stop (None, "few", "degenerate" or "not finite"), and without a
    stop: C (float64), C32, kappa, lo, hi, before (= |mask|), verdict, ok and band (decide64 on C32)."""
    mask = np.asarray(mask, bool)
    before = int(mask.sum())
    if before < g.K[model]:
        return SimpleNamespace(stop="few", before=before)
    nm = normal64(model, p1[mask], p2[mask])
    if not nm.ok:
        return SimpleNamespace(stop="degenerate", before=before)
    C = candidate64(model, p1, p2, mask, prev)
    C32 = C.astype(np.float32)
    if not np.isfinite(C32).all():
        return SimpleNamespace(stop="not finite", before=before)
    ok, band = g.decide64(model, C32, p1, p2, bound)
    lo, hi = int((ok & ~band).sum()), int((ok | band).sum())
    verdict = "accept" if lo >= before else ("reject" if hi < before else "undecided")
    return SimpleNamespace(stop=None, C=C, C32=C32, kappa=nm.kappa, lo=lo, hi=hi, before=before, verdict=verdict, ok=ok, band=band)


def ransac64(c):
    """The float64 model of steps 1-5 on case c -> (M0 as float32, its mask by the float64 gate, t): the largest exact score,
    the lowest t among equals."""
    h = g.hypotheses(c.model, c.p1, c.p2, c.seed, c.T, c.bound)
    score = (g.gates_many(c.model, h.M0, c.p1, c.p2) < c.bound).sum(1)
    score[h.bad] = 0
    t = int(np.argmax(score))
    M = h.M[t].astype(np.float32)
    return M, g.decide64(c.model, M, c.p1, c.p2, c.bound)[0], t


def chain64(c, refit=4):
    """The rule on case c in float64 -> namespace M0, S0, t, steps (step64 records, the last one may be a stop or a reject), M,
    S (the last accepted), refits.  An undecided step is taken as its float64 count decides."""
    M, S, t = ransac64(c)
    out = SimpleNamespace(M0=M, S0=S, t=t, steps=[], refits=0)
    for _ in range(refit):
        st = step64(c.model, c.p1, c.p2, S, M, c.bound)
        out.steps.append(st)
        if st.stop is not None or int(st.ok.sum()) < st.before:
            break
        same = np.array_equal(st.ok, S)
        M, S = st.C32, st.ok
        out.refits += 1
        if same:
            break
    out.M, out.S = M, S
    return out


# ---- noisy scenes ---------------------------------------------------------------------------------------------------------

SIZE = {65: 1000, 300: 4096, 1031: 4096}
# (model, n, sigma) -> the RANSAC seed: the first seed >= 1 whose chain (chain64, refit = 4) has kappa <= MAX_KAPPA at every
# step, no undecided step, no rejected step, and at least halves rms() -- the conditions test_refit_cases.py checks
NOISY = {("H", 65, 0.5): 1, ("H", 65, 1.0): 1, ("H", 300, 0.5): 1, ("H", 300, 1.0): 1, ("H", 1031, 0.5): 1, ("H", 1031, 1.0): 1,
         ("F", 65, 0.5): 1, ("F", 65, 1.0): 3, ("F", 300, 0.5): 1, ("F", 300, 1.0): 2, ("F", 1031, 0.5): 1, ("F", 1031, 1.0): 1}
QUALITY = tuple(NOISY)
# a chain that ends in a discarded candidate (decided: hi < the count before)
REJECTED = ("F", 1031, 1.0, 2)


@functools.lru_cache(maxsize=None)
def noisy(model, n, sigma, seed):
    """-> namespace as geom_cases.case() and clean2 (the second points before the noise), sigma."""
    size = SIZE[n]
    sc = g.scene(model, n, size)
    rng = np.random.default_rng(7000 + 10 * n + int(round(10 * sigma)) + (0 if model == "H" else 5))
    p2 = sc.p2.copy()
    p2[sc.planted] = (sc.p2[sc.planted].astype(np.float64) + rng.normal(0, sigma, (int(sc.planted.sum()), 2))).astype(np.float32)
    loc1, loc2, matches = g._layout(sc.p1, p2, size)
    return SimpleNamespace(name=f"{model} {n} sigma {sigma} seed {seed}", model=model, n=n, T=T_NOISY, bound=g.BOUND[model], seed=seed,
                           loc1=loc1, loc2=loc2, matches=matches, p1=sc.p1, p2=p2, clean2=sc.p2, planted=sc.planted, truth=sc.truth,
                           sigma=sigma)


def rms(c, M):
    """The RMS gate value of M on the noise-free planted inliers of noisy case c."""
    v = g.gate_many(c.model, M, c.p1[c.planted], c.clean2[c.planted])
    return float(np.sqrt(np.mean(v ** 2)))


def chain_is_sound(ch):
    """kappa <= MAX_KAPPA at every step and no step undecided."""
    return all(st.stop is not None or (st.kappa <= MAX_KAPPA and st.verdict != "undecided") for st in ch.steps)


def sublist(name, n):
    """The first n correspondences of a planted case of geom_cases as a case of its own (same locations, seed and T)."""
    c = g.case(name)
    return SimpleNamespace(name=f"{name}[:{n}]", model=c.model, n=n, T=c.T, bound=c.bound, seed=c.seed, loc1=c.loc1, loc2=c.loc2,
                           matches=np.ascontiguousarray(c.matches[:n]), p1=c.p1[:n], p2=c.p2[:n], planted=c.planted[:n], truth=c.truth)


SEAMS = (None, 255, 256, 257, 2048, 2049)       # None: k
