"""Inputs and an independent float64 model for the geometry-estimation tests (hess_matcher_estimate / _estimate_pairs; a plain
helper module, no tests in it).

  sample        the sampling rule of include/hess_abi.h restated in Python integers
  scenes        "H": a projective homography with nine non-zero entries; "F": a 3-D point cloud seen by two cameras that
                differ by a rotation and a translation, F from the cameras.  Inliers are the exact images rounded to float32;
                an outlier's second point is redrawn until its gate value under the truth (float64) is at least 4 x bound.
                Rows are shuffled, and the correspondences index two location sets with a few rows nobody refers to.
                "clean": every correspondence an inlier of guided_cases' dyadic affine H on a quarter-pixel grid
  bounds        H 8.0 (both axes of the box test), F 4.0 (Sampson, squared pixels); inlier share H 0.5, F 0.7
  seed          per case the first seed >= 1 with at least 8 all-inlier hypotheses among the T (T = 1: hypothesis 0 draws only
                inliers and a float32 SVD solve on it puts every inlier within a quarter of the bound); the clean case: the first
                seed whose sample 0 has no three points spanning a triangle below 1000 square pixels
  solve64       the hypothesis of a sample in float64 (Hartley normalisation, SVD null vector, rank 2 for F)
  gate64 / band the gate values of guided_cases.gates and the rounding margins of guided_cases.margins per correspondence
  alone         the seed under which hypothesis 0 is hypothesis t of another seed (mix is a bijection: unmix inverts it)
  hypotheses    all T hypotheses of a case at once in float64 (samples, solve_many, gates_many) with the interval [lo, hi] that
                holds the kernel's float32 score of each: the counts of gate values below bound / 2 and below 2 x bound
  separated     scenes on which `winner` names the index the rule must return whatever float32 does inside those intervals, one
                per place where the rule is implemented (lanes, wavefronts, blocks, the finish kernel's entries, dead lanes);
                WRONG_WINNER_RULES: the arg-max bugs these cases are chosen to tell from the rule
  solo          256 single hypotheses per case for the comparison with the float64 solve, with their conditioning
  noisy         inliers with a pixel of noise: a near-continuous range of scores
  degenerate    coincident, collinear, repeated and non-finite points
"""
import functools
from types import SimpleNamespace

import numpy as np

import guided_cases as gc

M32 = 0xFFFFFFFF
K = {"H": 4, "F": 8}
MODEL_ID = {"H": 1, "F": 2}          # HESS_GEOM_HOMOGRAPHY, HESS_GEOM_FUNDAMENTAL
BOUND = {"H": 8.0, "F": 4.0}
SHARE = {"H": 0.5, "F": 0.7}
MIN_ALL_INLIER = 8

# name -> (model, n, T, image size)
CASES = {}
for _m in ("H", "F"):
    CASES[f"{_m} below k"] = (_m, K[_m] - 1, 64, 4096)
    CASES[f"{_m} n = k"] = (_m, K[_m], 64, 4096)
    CASES[f"{_m} 65"] = (_m, 65, 256, 1000)
    CASES[f"{_m} 300"] = (_m, 300, 257, 4096)
    CASES[f"{_m} 1031"] = (_m, 1031, 512, 4096)
    CASES[f"{_m} 5000"] = (_m, 5000, 2048, 4096)
    CASES[f"{_m} 65 T = 1"] = (_m, 65, 1, 1000)
CASES["clean"] = ("H", 64, 64, 1000)
PLANTED = tuple(k for k, v in CASES.items() if v[1] >= K[v[0]] and k != "clean")   # cases with a model to find
BELOW = tuple(k for k, v in CASES.items() if v[1] < K[v[0]])


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def sample(seed, t, k, n):
    """-> the k distinct indices below n of hypothesis t, in draw order."""
    h = mix((mix((seed ^ 0x9E3779B9) & M32) + t) & M32)
    chosen = []
    for j in range(k):
        c = (mix((h + j) & M32) * (n - j)) >> 32
        for s in sorted(chosen):
            if s <= c:
                c += 1
        chosen.append(c)
    return chosen


def _h1(p):
    return np.concatenate([p, np.ones((len(p), 1), p.dtype)], 1)


def _cross(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def _norm_T(p):
    c = p.mean(0)
    s = np.sqrt(2) / np.sqrt(((p - c) ** 2).sum(1)).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]], p.dtype)


def solve(model, p1, p2, dtype=np.float64, rank2=True):
    """-> the unit-norm [3, 3] hypothesis of k correspondences p1 -> p2 ([k, 2]), computed in `dtype`.  rank2=False: F as the
    null vector gives it, back in pixel coordinates (what the kernel scores; `finish64` makes it the returned matrix)."""
    p1, p2 = p1.astype(dtype), p2.astype(dtype)
    T1, T2 = _norm_T(p1), _norm_T(p2)
    a, b = _h1(p1) @ T1.T, _h1(p2) @ T2.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a, b):
        if model == "H":
            rows.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
            rows.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
        else:
            rows.append([u * x, u * y, u, v * x, v * y, v, x, y, 1])
    A = np.array(rows, dtype)
    if len(A) < 9:                                       # a ninth row of zeros: full V^T from the SVD
        A = np.concatenate([A, np.zeros((9 - len(A), 9), dtype)])
    m = np.linalg.svd(A)[2][-1].reshape(3, 3).astype(dtype)
    if model == "H":
        M = np.linalg.inv(T2).astype(dtype) @ m @ T1
    elif rank2:
        U, S, Vt = np.linalg.svd(m)
        S[2] = 0
        M = T2.T @ ((U * S) @ Vt).astype(dtype) @ T1
    else:
        M = T2.T @ m @ T1
    return M / np.linalg.norm(M)


def solve64(model, p1, p2):
    return solve(model, p1, p2, np.float64)


def _diag(fn, M, p1, p2, step=512):
    """guided_cases works on all pairs of two sets: the correspondences are the diagonal, taken block by block."""
    M = np.asarray(M)
    out = None
    for s in range(0, len(p1), step):
        r = fn(p1[s:s + step], p2[s:s + step], M, M)
        r = [np.diagonal(a).copy() for a in r]
        out = r if out is None else [np.concatenate(z) for z in zip(out, r)]
    if out is None:
        out = [np.zeros(0)] * 3
    return out


def gate64(model, M, p1, p2):
    """-> the gate value per correspondence in float64: H max(d0, d1), F the Sampson error (inf where not finite)."""
    d0, d1, se = _diag(gc.gates, M, p1, p2)
    with np.errstate(invalid="ignore"):
        v = np.maximum(d0, d1) if model == "H" else se
    return np.where(np.isfinite(v), v, np.inf)


def gate_many(model, M, p1, p2):
    """gate64 written out per correspondence, for the thousands of hypotheses the CPU test walks (guided_cases.gates builds
    all pairs of two sets).  test_geom_cases.py holds it against gate64."""
    M = np.asarray(M, np.float64)
    a, b = _h1(p1.astype(np.float64)), _h1(p2.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fx = a @ M.T
        if model == "H":
            v = np.abs(fx[:, :2] / fx[:, 2:] - b[:, :2]).max(1)
        else:
            ft = b @ M
            s = (b * fx).sum(1)
            v = s * s / (fx[:, 0] ** 2 + fx[:, 1] ** 2 + ft[:, 0] ** 2 + ft[:, 1] ** 2)
    return np.where(np.isfinite(v), v, np.inf)


def decide64(model, M, p1, p2, bound):
    """-> (passes the gate in float64, lies in the float32 rounding band of the bound) per correspondence."""
    b = float(np.float32(bound))
    d0, d1, se = _diag(gc.gates, M, p1, p2)
    m0, m1, ms = _diag(gc.margins, M, p1, p2)
    with np.errstate(invalid="ignore"):
        if model == "H":
            ok = np.isfinite(d0) & np.isfinite(d1) & (d0 < b) & (d1 < b)
            band = ((np.abs(d0 - b) <= m0) & (d1 < b + m1)) | ((np.abs(d1 - b) <= m1) & (d0 < b + m0))
        else:
            ok = np.isfinite(se) & (se < b)
            band = np.abs(se - b) <= ms
    return ok, band


H_TRUE = np.array([[1.1, 0.08, 30.0], [-0.06, 0.95, -20.0], [2e-5, -1e-5, 1.0]])


@functools.lru_cache(maxsize=None)
def scene(model, n, size):
    """-> namespace p1, p2 (float32 [n, 2] correspondences), planted (bool [n]), truth ([3, 3] float64); n = k: all inliers."""
    rng = np.random.default_rng(1000 * n + size + (0 if model == "H" else 500))
    bound = BOUND[model]
    nin = n if n <= K[model] else int(round(n * SHARE[model]))
    if model == "H":
        truth = H_TRUE
        p1 = rng.uniform(0, size, (n, 2))
        p2 = gc.project(truth, p1)
    else:
        X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)
        f = size * 1.2
        Kc = np.array([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1]])
        c, s = np.cos(0.15), np.sin(0.15)
        R, tt = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([-1.0, 0.1, 0.3])
        x1, x2 = X @ Kc.T, (X @ R.T + tt) @ Kc.T
        p1, p2 = x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]
        truth = np.linalg.inv(Kc).T @ _cross(tt) @ R @ np.linalg.inv(Kc)
        truth = truth / np.linalg.norm(truth)
    p1, p2 = p1.astype(np.float32), p2.astype(np.float32)
    for i in range(nin, n):
        while True:
            p2[i] = rng.uniform(0, size, 2).astype(np.float32)
            if gate64(model, truth, p1[i:i + 1], p2[i:i + 1])[0] >= 4 * bound:
                break
    perm = rng.permutation(n)
    planted = np.zeros(n, bool)
    planted[:nin] = True
    return SimpleNamespace(p1=p1[perm], p2=p2[perm], planted=planted[perm], truth=truth)


def all_inlier(model, n, T, seed, planted):
    return [t for t in range(T) if planted[sample(seed, t, K[model], n)].all()]


def _triangles_ok(p, least=1000.0):
    for a in range(len(p)):
        for b in range(a + 1, len(p)):
            for c in range(b + 1, len(p)):
                u, v = p[b] - p[a], p[c] - p[a]
                if abs(u[0] * v[1] - u[1] * v[0]) / 2 < least:
                    return False
    return True


def _layout(p1, p2, size):
    """The correspondences as rows of two location sets, in shuffled order, with rows that no match names."""
    n = len(p1)
    rng = np.random.default_rng(n + 17)
    r1, r2 = rng.permutation(n + 7)[:n], rng.permutation(n + 3)[:n]
    loc1 = rng.uniform(0, size, (n + 7, 2)).astype(np.float32)
    loc2 = rng.uniform(0, size, (n + 3, 2)).astype(np.float32)
    loc1[r1], loc2[r2] = p1, p2
    return loc1, loc2, np.ascontiguousarray(np.stack([r1, r2], 1), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace model, n, T, bound, seed, loc1, loc2 (float32 [rows, 2]), matches (int32 [n, 2]), p1, p2 (the located
    correspondences), planted, allin (the all-inlier hypotheses), truth."""
    model, n, T, size = CASES[name]
    k, bound = K[model], BOUND[model]
    if name == "clean":
        rng = np.random.default_rng(64)
        p1 = (rng.integers(0, 1000 * gc.GRID, size=(n, 2)) / gc.GRID)
        truth = gc.matrices("affine")[0].astype(np.float64)
        p2 = gc.project(truth, p1)
        p1, p2 = p1.astype(np.float32), p2.astype(np.float32)
        assert np.array_equal(p2.astype(np.float64), gc.project(truth, p1.astype(np.float64)))     # exact images
        planted = np.ones(n, bool)
        seed = next(s for s in range(1, 1000) if _triangles_ok(p1[sample(s, 0, k, n)].astype(np.float64))
                    and _triangles_ok(p2[sample(s, 0, k, n)].astype(np.float64)))
    else:
        sc = scene(model, n, size)
        p1, p2, planted, truth = sc.p1, sc.p2, sc.planted, sc.truth
        seed = 0
        if n >= k:
            for seed in range(1, 100000):
                if T > 1:
                    if len(all_inlier(model, n, T, seed, planted)) >= min(MIN_ALL_INLIER, T):
                        break
                else:
                    s = sample(seed, 0, k, n)
                    if planted[s].all():
                        g = gate64(model, solve(model, p1[s], p2[s], np.float32).astype(np.float32), p1, p2)
                        if g[planted].max() < bound / 4 and g[~planted].min() >= 2 * bound:
                            break
    allin = all_inlier(model, n, T, seed, planted) if n >= k else []
    loc1, loc2, matches = _layout(p1, p2, size)
    return SimpleNamespace(name=name, model=model, n=n, T=T, bound=bound, seed=seed, loc1=loc1, loc2=loc2, matches=matches,
                           p1=p1, p2=p2, planted=planted, allin=allin, truth=truth)


# ---- one hypothesis alone ----------------------------------------------------------------------------------------------

def unmix(x):
    """The inverse of mix (mix is a bijection on uint32)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7ED1B41D) & M32
    x ^= (x >> 13) ^ (x >> 26)
    x = (x * 0xA5CB9243) & M32
    x ^= x >> 16
    return x


def alone(seed, t):
    """-> the seed whose hypothesis 0 is hypothesis t of `seed`: a call with hypotheses = 1 and this seed returns what
    hypothesis t yields on its own (its finished matrix and mask, or no model when it scores below k)."""
    return unmix((mix((seed ^ 0x9E3779B9) & M32) + t) & M32) ^ 0x9E3779B9


# ---- all hypotheses of a case in float64 -------------------------------------------------------------------------------

def _mix_many(x):
    m = np.uint64(M32)
    x = x & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & m
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & m
    return x ^ (x >> np.uint64(16))


def samples(seed, T, k, n):
    """-> int64 [T, k]: sample(seed, t, k, n) for every t < T (the same rule on arrays; test_geom_cases.py compares)."""
    base = np.uint64(mix((seed ^ 0x9E3779B9) & M32))
    h = _mix_many(base + np.arange(T, dtype=np.uint64))
    out = np.zeros((T, k), np.int64)
    for j in range(k):
        c = ((_mix_many(h + np.uint64(j)) * np.uint64(n - j)) >> np.uint64(32)).astype(np.int64)
        if j:
            earlier = np.sort(out[:, :j], 1)
            for i in range(j):
                c += earlier[:, i] <= c
        out[:, j] = c
    return out


def _norm_many(P):
    c = P.mean(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(2) / np.sqrt(((P - c) ** 2).sum(2)).mean(1)
        T = np.zeros((len(P), 3, 3))
        T[:, 0, 0] = T[:, 1, 1] = s
        T[:, 0, 2], T[:, 1, 2], T[:, 2, 2] = -s * c[:, 0, 0], -s * c[:, 0, 1], 1
        return (P - c) * s[:, None, None], T


def finish64(model, M0):
    """What step 5 of the rule makes of hypotheses M0 [..., 3, 3] in pixel coordinates: rank 2 for F, unit norm."""
    M = np.asarray(M0, np.float64)
    if model == "F":
        U, S, Vt = np.linalg.svd(M)
        S[..., 2] = 0
        M = (U * S[..., None, :]) @ Vt
    with np.errstate(invalid="ignore", divide="ignore"):
        return M / np.linalg.norm(M, axis=(-2, -1), keepdims=True)


def solve_many(model, P1, P2):
    """The float64 solve of T samples at once (P1 -> P2, [T, k, 2]): Hartley normalisation, the SVD null vector of the
    zero-padded 9 x 9 system, back to pixel coordinates -> namespace M0 [T, 3, 3] (unit norm, what is scored), M (finish64 of
    it: what is returned), kappa [T] (sigma_1 / sigma_8 of the normalised design matrix), bad [T] (a non-finite system:
    coincident or non-finite points; M0 and M are zero there)."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a, T1 = _norm_many(P1)
        b, T2 = _norm_many(P2)
        x, y, u, v = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
        z, o = np.zeros_like(x), np.ones_like(x)
        if model == "H":
            A = np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], -1),
                                np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], -1)], 1)
        else:
            A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, o], -1)
    A = np.concatenate([A, np.zeros((len(A), 9 - A.shape[1], 9))], 1)
    bad = ~(np.isfinite(A).all((1, 2)) & np.isfinite(T1).all((1, 2)) & np.isfinite(T2).all((1, 2)))
    A[bad], T1[bad], T2[bad] = 0, np.eye(3), np.eye(3)
    _, S, Vt = np.linalg.svd(A)
    m = Vt[:, -1].reshape(-1, 3, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(S[:, 7] > 0, S[:, 0] / S[:, 7], np.inf)
    M0 = np.linalg.inv(T2) @ m @ T1 if model == "H" else T2.transpose(0, 2, 1) @ m @ T1
    M0 = M0 / np.linalg.norm(M0, axis=(1, 2), keepdims=True)
    M = finish64(model, M0)
    M0[bad], M[bad], kappa[bad] = 0, 0, np.inf
    return SimpleNamespace(M0=M0, M=M, kappa=kappa, bad=bad)


def gates_many(model, Ms, p1, p2, step=4096):
    """gate_many for hypotheses Ms [T, 3, 3] at once -> [T, n]."""
    Ms = np.asarray(Ms, np.float64)
    a, b = _h1(p1.astype(np.float64)), _h1(p2.astype(np.float64))
    out = np.empty((len(Ms), len(a)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(0, len(Ms), step):
            fx = np.einsum("tij,nj->tni", Ms[s:s + step], a)
            if model == "H":
                v = np.abs(fx[..., :2] / fx[..., 2:] - b[None, :, :2]).max(2)
            else:
                ft = np.einsum("tji,nj->tni", Ms[s:s + step], b)
                d = (b[None] * fx).sum(2)
                v = d * d / (fx[..., 0] ** 2 + fx[..., 1] ** 2 + ft[..., 0] ** 2 + ft[..., 1] ** 2)
            out[s:s + step] = np.where(np.isfinite(v), v, np.inf)
    return out


def hypotheses(model, p1, p2, seed, T, bound):
    """The model of all T hypotheses -> namespace idx [T, k], M0, M, kappa, bad (solve_many) and the score interval lo, hi
    [T]: the counts of gate values (float64, under M0: F is scored before rank 2) below bound / 2 and below 2 x bound.  The
    kernel's float32 score of a hypothesis lies between them unless its solve is off by more than a factor 2 in the gate."""
    idx = samples(seed, T, K[model], len(p1))
    h = solve_many(model, p1[idx], p2[idx])
    v = gates_many(model, h.M0, p1, p2)
    h.idx, h.lo, h.hi = idx, (v < bound / 2).sum(1), (v < 2 * bound).sum(1)
    h.lo[h.bad] = h.hi[h.bad] = 0
    return h


def winner(lo, hi):
    """-> (S, t*, the hypotheses that tie with t*) where the rule's winner is t* whatever float32 does inside the score
    intervals, or None: S = max hi; t* the first t with lo = S; every t before it has hi < S; every t with lo < S has
    hi <= S - 2."""
    S = int(hi.max())
    ties = np.flatnonzero(lo == S)
    if not len(ties) or (hi[:ties[0]] >= S).any() or hi[lo < S].max(initial=-2) > S - 2:
        return None
    return S, int(ties[0]), ties


def near_bound(model, M, p1, p2, bound, factor=1.0):
    """-> bool [n]: the gate value under M lies within factor x guided_cases.margins of the bound (decide64's band)."""
    b = float(np.float32(bound))
    d0, d1, se = _diag(gc.gates, M, p1, p2)
    m0, m1, ms = (factor * m for m in _diag(gc.margins, M, p1, p2))
    with np.errstate(invalid="ignore"):
        if model == "H":
            return ((np.abs(d0 - b) <= m0) & (d1 < b + m1)) | ((np.abs(d1 - b) <= m1) & (d0 < b + m0))
        return np.abs(se - b) <= ms


SOLO = ("H 300", "F 300", "H 65")    # the cases whose single hypotheses are held against float64 (image sizes 4096, 1000)
SOLO_SEEDS = range(1000, 1256)
KAPPA_MAX = 1.0e4


@functools.lru_cache(maxsize=None)
def solo(name):
    """Hypothesis 0 of each of SOLO_SEEDS on case `name` -> namespace idx [256, k], M, M0, kappa (solve_many), M32 (numpy's
    float32 SVD solve finished by the rule, rounded to float32: the reference for the kernel's error), use (kappa <=
    KAPPA_MAX), own (the largest gate value of M0 on the sample's own k points)."""
    c = case(name)
    idx = np.array([sample(s, 0, K[c.model], c.n) for s in SOLO_SEEDS])
    h = solve_many(c.model, c.p1[idx], c.p2[idx])
    h.idx, h.use = idx, h.kappa <= KAPPA_MAX
    h.M32 = np.stack([finish64(c.model, solve(c.model, c.p1[s], c.p2[s], np.float32, rank2=False).astype(np.float32))
                      for s in idx]).astype(np.float32)
    h.own = np.array([gate_many(c.model, h.M0[q], c.p1[s], c.p2[s]).max() for q, s in enumerate(idx)])
    return h


def distance(A, B):
    """min(|A - B|_F, |A + B|_F) in float64: matrices of unit norm up to their sign."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.minimum(np.linalg.norm(A - B, axis=(-2, -1)), np.linalg.norm(A + B, axis=(-2, -1)))


# ---- separated scenes: the index of the winner is exact ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_scene(n, nin, size, rs):
    """An H scene on the quarter-pixel grid: nin exact images of guided_cases' dyadic affine H, n - nin outliers on the grid
    at 4 x bound or more under the truth, rows shuffled -> namespace as scene()."""
    rng = np.random.default_rng(rs)
    truth = gc.matrices("affine")[0].astype(np.float64)
    p1 = rng.integers(0, size * gc.GRID, size=(n, 2)) / gc.GRID
    p2 = gc.project(truth, p1)
    for i in range(nin, n):
        while True:
            p2[i] = rng.integers(0, 2 * size * gc.GRID, 2) / gc.GRID
            if gate64("H", truth, p1[i:i + 1], p2[i:i + 1])[0] >= 4 * BOUND["H"]:
                break
    perm = rng.permutation(n)
    planted = np.zeros(n, bool)
    planted[:nin] = True
    p1, p2 = p1[perm].astype(np.float32), p2[perm].astype(np.float32)
    assert np.array_equal(p2[planted[perm]].astype(np.float64), gc.project(truth, p1[planted[perm]].astype(np.float64)))
    return SimpleNamespace(p1=p1, p2=p2, planted=planted[perm], truth=truth)


# name -> model, what the seed search establishes (see _established), n, inliers (H; F scenes have SHARE), T, image size, the
# scene's seed (H), the first seed tried.  The start seeds only shorten the search: every property is checked from them on.
SEPARATED = {
    "H waves": ("H", "waves", 64, 24, 256, 1000, 1, 1),
    "H blocks": ("H", "blocks", 64, 18, 1025, 1000, 2, 667),
    "H last": ("H", "last", 64, 7, 769, 1000, 3, 24121),
    "H dead lanes": ("H", "dead", 64, 7, 326, 1000, 4, 257),
    "H dense ties": ("H", "dense", 64, 32, 1024, 1000, 5, 1),
    "H 65536 a": ("H", "far", 64, 7, 65536, 1000, 6, 118),
    "H 65536 b": ("H", "near", 64, 7, 65536, 1000, 7, 6),
    "F waves": ("F", "waves", 65, None, 256, 1000, None, 103),
    "F blocks": ("F", "blocks", 24, None, 769, 1000, None, 39740),
    "F last": ("F", "last", 20, None, 257, 1000, None, 4847),
    "F dead lanes": ("F", "dead", 16, None, 70, 1000, None, 1),
    "F dense ties": ("F", "dense", 65, None, 1024, 1000, None, 1),
}


def _established(kind, T, ts, ties):
    """The property of the table in the issue that names the case, for the winner ts and its ties (ascending, ts first)."""
    later = ties[1:]
    if kind == "waves":         # lanes 64..255 of block 0; a tie in the same wavefront and one in a later wavefront
        return T == 256 and ts >= 64 and (later // 64 == ts // 64).any() and (later // 64 > ts // 64).any()
    if kind == "blocks":        # a block >= 1; ties in two later blocks or more, one of them the last, partial one
        blocks = set((later[later // 256 > ts // 256] // 256).tolist())
        return T % 256 == 1 and T >= 769 and ts >= 256 and len(blocks) >= 2 and (T - 1) // 256 in blocks
    if kind == "last":          # the last live lane, alone
        return T % 256 == 1 and ts == T - 1 and len(ties) == 1
    if kind == "dense":         # ties in every wavefront of every block
        return T == 1024 and len(set((ties // 64).tolist())) == 16
    if kind == "far":           # a finish thread beyond the first wavefront, a tie in a later block
        return ts // 256 >= 64 and (later // 256 > ts // 256).any()
    if kind == "near":          # a finish thread of the first wavefront, a tie in a block >= 64
        return ts // 256 < 64 and (later // 256 >= 64).any()
    raise ValueError(kind)


def _screen(model, p1, p2, planted, s, bound):
    """The T = 1 screen of case(): a float32 SVD solve of sample s puts every inlier within bound / 4, every outlier beyond
    2 x bound."""
    v = gate64(model, solve(model, p1[s], p2[s], np.float32).astype(np.float32), p1, p2)
    return bool(v[planted].max() < bound / 4 and v[~planted].min(initial=np.inf) >= 2 * bound)


FIRST_NOT_PINNED = ()      # the planted cases whose first all-inlier hypothesis does not pass the screen (checked on the CPU)


def first_all_inlier_is_sound(name):
    """The first all-inlier hypothesis of planted case `name` passes the screen: it scores every inlier, so the lowest-t rule
    names it.  test_matcher_estimate_gpu.py asks for exactly that index where this holds."""
    c = case(name)
    return _screen(c.model, c.p1, c.p2, c.planted, sample(c.seed, c.allin[0], K[c.model], c.n), c.bound)


@functools.lru_cache(maxsize=None)
def separated(name):
    """-> namespace as case() and: S (the winner's score), tstar, ties, lo, hi (over the T hypotheses); for the "dead lanes"
    cases tstar is None, S_all and dead (the dead lanes of the last block that reach S_all), S_live = max hi over t < T.
    The "dead lanes" cases give a dead lane the hypothesis of its own t: they catch a kernel that lets lanes t >= T take
    part with their own samples.  The kernel as written gives dead lanes the sample of t = 0, so dropping only its `live`
    test from the key would go unseen here (and would change no result: lane 0 holds the same hypothesis with a lower t)."""
    model, kind, n, nin, T, size, rs, start = SEPARATED[name]
    k, bound = K[model], BOUND[model]
    sc = grid_scene(n, nin, size, rs) if model == "H" else scene(model, n, size)
    p1, p2, planted = sc.p1, sc.p2, sc.planted
    want = int(planted.sum())
    full = 256 * ((T + 255) // 256)
    extra = {}
    for seed in range(start, start + 1000000):
        # cheap: what the all-inlier samples alone rule out
        if kind in ("last", "blocks") and not planted[sample(seed, T - 1, k, n)].all():
            continue
        if kind != "dense" and kind != "near" and planted[sample(seed, 0, k, n)].all():
            continue
        allin = np.flatnonzero(planted[samples(seed, full if kind == "dead" else min(T, 1025), k, n)].all(1))
        if kind == "dead":
            if (allin < T).any() or not (allin >= T).any():
                continue
            h = hypotheses(model, p1, p2, seed, full, bound)
            S_all, S_live = int(h.hi.max()), int(h.hi[:T].max())
            dead = np.flatnonzero(h.lo == S_all)
            if S_all != want or S_live >= S_all or not len(dead) or dead[0] < T or S_live < k:
                continue
            extra = dict(tstar=None, S=None, ties=None, S_all=S_all, S_live=S_live, dead=dead, lo=h.lo, hi=h.hi)
            break
        if T <= 1025 and (not len(allin) or not _established(kind, T, int(allin[0]), allin)):
            continue                                     # (a necessary condition: the ties are all-inlier samples)
        h = hypotheses(model, p1, p2, seed, T, bound)
        w = winner(h.lo, h.hi)
        if w is None or w[0] != want or not _established(kind, T, w[1], w[2]):
            continue
        if not np.array_equal(gates_many(model, h.M0[w[1]:w[1] + 1], p1, p2)[0] < bound / 2, planted):
            continue
        if model == "F" and not all(_screen(model, p1, p2, planted, h.idx[t], bound)
                                    for t in range(w[1] + 1) if planted[h.idx[t]].all()):
            continue
        extra = dict(S=w[0], tstar=w[1], ties=w[2], lo=h.lo, hi=h.hi)
        break
    else:
        raise AssertionError(f"no seed makes {name} valid")
    loc1, loc2, matches = _layout(p1, p2, size)
    return SimpleNamespace(name=name, model=model, kind=kind, n=n, T=T, bound=bound, seed=seed, loc1=loc1, loc2=loc2,
                           matches=matches, p1=p1, p2=p2, planted=planted, truth=sc.truth, **extra)


# ---- winner rules that are WRONG, as functions of the scores of all lanes (dead ones included) and T ------------------

def _first_max(s):
    return int(np.argmax(s)) if len(s) else -1


def _last_max(s):
    return len(s) - 1 - int(np.argmax(s[::-1])) if len(s) else -1


def _wave_maxima_to_the_higher(s, T):
    best = (-1, -1)                                      # blocks in ascending order, a later one only on a larger score
    for b in range(0, T, 256):
        top = (-1, -1)
        for w in range(b, min(b + 256, T), 64):          # wavefronts: first maximum each, a tie to the higher wavefront
            t = w + _first_max(s[w:min(w + 64, T)])
            if s[t] >= top[0]:
                top = (int(s[t]), t)
        if top[0] > best[0]:
            best = top
    return best[1]


def right_winner(s, T):
    return _first_max(s[:T])


WRONG_WINNER_RULES = {
    "highest t among equal scores": lambda s, T: _last_max(s[:T]),
    "first wavefront of each block only": lambda s, T: _first_max(np.where(np.arange(T) % 256 < 64, s[:T], -1)),
    "wavefront maxima, ties to the higher wavefront": _wave_maxima_to_the_higher,
    "first 64 block entries only": lambda s, T: _first_max(s[:min(T, 64 * 256)]),
    "last block ignored": lambda s, T: _first_max(s[:256 * ((T - 1) // 256)]),
    "dead lanes take part": lambda s, T: _first_max(s),
}


def lane_scores(c):
    """The model's scores (lo) of every lane of every block of separated case c, dead lanes with the hypothesis of their t."""
    full = 256 * ((c.T + 255) // 256)
    return c.lo if len(c.lo) == full else hypotheses(c.model, c.p1, c.p2, c.seed, full, c.bound).lo


# ---- a noisy scene ------------------------------------------------------------------------------------------------------

NOISY_SCENE_SEED = 229      # of the scene seeds 1..284 the one with the fewest close decisions (20 of 512 hypotheses)


@functools.lru_cache(maxsize=None)
def noisy():
    """H, n = 200: 100 inliers of H_TRUE with N(0, 1 px) noise on the second point, 100 outliers uniform in the image, rows
    shuffled; bound 3.0, T = 512.  A near-continuous range of scores.  NOISY_SCENE_SEED is chosen so that few float32
    decisions are close ones (test_geom_cases.py states the condition)."""
    n, size = 200, 1000
    rng = np.random.default_rng(NOISY_SCENE_SEED)
    p1 = rng.uniform(0, size, (n, 2))
    p2 = gc.project(H_TRUE, p1) + rng.normal(0, 1, (n, 2))
    p2[n // 2:] = rng.uniform(0, size, (n - n // 2, 2))
    perm = rng.permutation(n)
    planted = np.zeros(n, bool)
    planted[:n // 2] = True
    p1, p2 = p1[perm].astype(np.float32), p2[perm].astype(np.float32)
    loc1, loc2, matches = _layout(p1, p2, size)
    return SimpleNamespace(name="noisy H", model="H", n=n, T=512, bound=3.0, seed=1, loc1=loc1, loc2=loc2, matches=matches,
                           p1=p1, p2=p2, planted=planted[perm], truth=H_TRUE)


# ---- degenerate inputs -------------------------------------------------------------------------------------------------

DEGENERATE = ("same pair", "collinear", "repeated", "all non-finite", "some non-finite")


@functools.lru_cache(maxsize=None)
def degenerate(kind, model):
    """-> namespace model, T, bound, seed, loc1, loc2, matches, p1, p2, none (every sample is non-finite: no model), tstar (the
    exact winner where the model can state it, else None).
      same pair        every match names the same two rows: all points coincide
      collinear        H: every first point on one line; F: every point of both images on one line
      repeated         60 % of the matches are one correspondence (an inlier), the others those of "<model> waves"; the seed is
                       the first for which `winner` names t*, a sample with at most one copy, and no hypothesis before it
                       draws two copies (a singular sample; most later ones do: 82 % for H, 99 % for F).  H: t* >= 1, so a
                       sound hypothesis that loses stands before the winner; F: t* passes the float32 screen
      all non-finite   every row that a match names holds +-inf or NaN
      some non-finite  "<model> waves" with +-inf and NaN in six rows that matches name"""
    base = separated(f"{model} waves")
    k, T, bound, seed = K[model], 256, BOUND[model], base.seed
    loc1, loc2, matches = base.loc1.copy(), base.loc2.copy(), base.matches.copy()
    none, tstar = False, None
    rng = np.random.default_rng(7)
    if kind == "same pair":
        matches[:] = matches[5]
        none = True
    elif kind == "collinear":
        t = rng.uniform(0, 900, len(loc1)).astype(np.float32)
        loc1 = np.stack([t, (0.5 * t + 20).astype(np.float32)], 1)
        if model == "F":
            u = rng.uniform(0, 900, len(loc2)).astype(np.float32)
            loc2 = np.stack([u, (0.5 * u + 20).astype(np.float32)], 1)
    elif kind == "repeated":
        one = matches[np.flatnonzero(base.planted)[0]]
        copies = int(round(1.5 * base.n))                # 60 % of the total
        perm = rng.permutation(base.n + copies)
        matches = np.ascontiguousarray(np.concatenate([matches, np.repeat(one[None], copies, 0)])[perm])
        planted = np.concatenate([base.planted, np.ones(copies, bool)])[perm]
        p1, p2 = loc1[matches[:, 0]], loc2[matches[:, 1]]
        rep = (matches == one).all(1)
        for seed in range(1, 1000000):
            idx = samples(seed, 8, k, len(matches))
            good = planted[idx].all(1) & (rep[idx].sum(1) <= 1)
            first = int(np.argmax(good))
            if not good.any() or (rep[idx[:first]].sum(1) >= 2).any() or (model == "H" and first == 0):
                continue
            h = hypotheses(model, p1, p2, seed, T, bound)
            w = winner(h.lo, h.hi)
            if w is None or w[1] != first or w[0] != int(planted.sum()):
                continue
            if model == "F" and not _screen(model, p1, p2, planted, idx[first], bound):
                continue
            tstar = first
            break
        else:
            raise AssertionError(f"no seed makes repeated {model} valid")
    elif kind == "all non-finite":
        bad = np.array([np.inf, -np.inf, np.nan], np.float32)
        loc1[matches[:, 0]] = bad[rng.integers(0, 3, (len(matches), 2))]
        none = True
    elif kind == "some non-finite":
        rows = rng.permutation(len(matches))[:6]
        loc1[matches[rows[:3], 0]] = np.array([[np.inf, 5.0], [3.0, np.nan], [-np.inf, np.inf]], np.float32)
        loc2[matches[rows[3:], 1]] = np.array([[np.nan, np.nan], [7.0, -np.inf], [np.inf, 2.0]], np.float32)
    else:
        raise ValueError(kind)
    return SimpleNamespace(name=f"{kind} {model}", model=model, T=T, bound=bound, seed=seed, loc1=loc1, loc2=loc2,
                           matches=matches, p1=loc1[matches[:, 0]], p2=loc2[matches[:, 1]], none=none, tstar=tstar)
