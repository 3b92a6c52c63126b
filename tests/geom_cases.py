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


def solve(model, p1, p2, dtype=np.float64):
    """-> the unit-norm [3, 3] hypothesis of k correspondences p1 -> p2 ([k, 2]), computed in `dtype`."""
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
    else:
        U, S, Vt = np.linalg.svd(m)
        S[2] = 0
        M = T2.T @ ((U * S) @ Vt).astype(dtype) @ T1
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
    # the correspondences as rows of two location sets, in shuffled order, with rows that no match names
    rng = np.random.default_rng(n + 17)
    r1, r2 = rng.permutation(n + 7)[:n], rng.permutation(n + 3)[:n]
    loc1 = rng.uniform(0, size, (n + 7, 2)).astype(np.float32)
    loc2 = rng.uniform(0, size, (n + 3, 2)).astype(np.float32)
    loc1[r1], loc2[r2] = p1, p2
    matches = np.ascontiguousarray(np.stack([r1, r2], 1), dtype=np.int32)
    return SimpleNamespace(name=name, model=model, n=n, T=T, bound=bound, seed=seed, loc1=loc1, loc2=loc2, matches=matches,
                           p1=p1, p2=p2, planted=planted, allin=allin, truth=truth)
