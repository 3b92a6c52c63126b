// hess_geom_refit.h -- the serial arithmetic of the estimator's least-squares refit (include/hess_abi.h, step 6), free of HIP:
// from the sums that geom_refit_kernel (hess_geom.hip) reduces over the inliers to the candidate matrix and the decision on
// it.  The kernel runs it on one lane with its 9 x 9 work matrices in LDS; tests/geom_refit_main.cpp runs the same functions
// on the host under the sanitizers.  Standard headers only; every function is __host__ __device__ under hipcc.
//
//   geom_refit_moments     what one correspondence adds to the moment sums (the kernel's inner loop; it fixes their layout)
//   geom_refit_scales      step 2: the two scales from the mean distances, or "stop"
//   geom_refit_normal      step 3: the 9 x 9 normal matrix N from the moment sums
//   geom_refit_eigen       step 4: the unit eigenvector of N's smallest eigenvalue, cyclic Jacobi in double
//   geom_refit_candidate   step 4: back to pixel coordinates, geom_finalise, the sign rule, float32, the finiteness test
//   geom_refit_decide      step 5: discard, accept, or accept and stop
//   geom_rotate, geom_finalise   rank 2 and unit norm of a 3 x 3 matrix (also step 5 of the estimator: geom_finish_kernel)
#ifndef HESS_GEOM_REFIT_H
#define HESS_GEOM_REFIT_H

#include <cmath>

#if defined(__HIPCC__)
#define HESS_GEOM_HD __host__ __device__
#else
#define HESS_GEOM_HD
#endif

constexpr int GEOM_MODEL_H = 1, GEOM_MODEL_F = 2;  // HESS_GEOM_HOMOGRAPHY, HESS_GEOM_FUNDAMENTAL
// Moment sums per model.  With p = (x, y, 1), q = (u, v, 1) in normalised coordinates and the six products of a pair of
// entries in the order (00, 01, 02, 11, 12, 22):
//   H  24: P = sum p p^T, U = sum u p p^T, V = sum v p p^T, W = sum (u^2 + v^2) p p^T, six entries each, in this order;
//   F  36: sum (q q^T)_a (p p^T)_b at 6 a + b.
constexpr int geom_refit_sums(int model) { return model == GEOM_MODEL_H ? 24 : 36; }

HESS_GEOM_HD inline int geom_refit_sym(int i, int j) {  // the index of (i, j) = (j, i) among the six products
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a == 0 ? b : (a == 1 ? 2 + b : 5);
}

// acc += the moments of the correspondence (x, y) -> (u, v), normalised coordinates.  Compile-time indices only.
template <int MODEL>
HESS_GEOM_HD inline void geom_refit_moments(double x, double y, double u, double v, double (&acc)[geom_refit_sums(MODEL)]) {
  const double pp[6] = {x * x, x * y, x, y * y, y, 1.0};
  if (MODEL == GEOM_MODEL_H) {
    const double w = fma(u, u, v * v);
#pragma unroll
    for (int b = 0; b < 6; b++) {
      acc[b] += pp[b];
      acc[6 + b] = fma(u, pp[b], acc[6 + b]);
      acc[12 + b] = fma(v, pp[b], acc[12 + b]);
      acc[18 + b] = fma(w, pp[b], acc[18 + b]);
    }
  } else {
    const double qq[6] = {u * u, u * v, u, v * v, v, 1.0};
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = 0; b < 6; b++) acc[6 * a + b] = fma(qq[a], pp[b], acc[6 * a + b]);
  }
}

// Step 2: s = sqrt 2 / (mean distance to the centroid) per image from the distance sums over cnt inliers.  false: a mean
// distance is zero or not finite -- stop.
HESS_GEOM_HD inline bool geom_refit_scales(int cnt, double sd1, double sd2, double& s1, double& s2) {
  const double d1 = sd1 / cnt, d2 = sd2 / cnt;
  if (!(d1 > 0.0) || !(d2 > 0.0) || !(d1 <= 1.0e300) || !(d2 <= 1.0e300)) return false;
  s1 = 1.4142135623730951 / d1;
  s2 = 1.4142135623730951 / d2;
  return true;
}

// Step 3: N (9 x 9, row-major, both triangles) from the moment sums.  H rows [x y 1 0 0 0 -ux -uy -u] and
// [0 0 0 x y 1 -vx -vy -v]: N = [P 0 -U; 0 P -V; -U -V W].  F row [ux uy u vx vy v x y 1] = q (x) p.
HESS_GEOM_HD inline void geom_refit_normal(int model, const double* sums, double* N) {
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++)
      for (int j = 0; j < 3; j++)
        for (int l = 0; l < 3; l++) {
          double v;
          if (model == GEOM_MODEL_H) {
            const int b = geom_refit_sym(k, l), blk = i <= j ? 3 * i + j : 3 * j + i;  // the 3 x 3 block (i, j), symmetric
            v = blk == 0 || blk == 4 ? sums[b] : (blk == 2 ? -sums[6 + b] : (blk == 5 ? -sums[12 + b] : (blk == 8 ? sums[18 + b] : 0.0)));
          } else {
            v = sums[6 * geom_refit_sym(i, j) + geom_refit_sym(k, l)];
          }
          N[9 * (3 * i + k) + 3 * j + l] = v;
        }
}

// Step 4: the unit eigenvector x of the smallest eigenvalue of the symmetric A (9 x 9, destroyed; V: 81 doubles of work
// space), by cyclic Jacobi: sweeps over (p, q), p < q, in row order, each rotation annihilating A[p][q]; a rotation is
// skipped once |A[p][q]| <= 1e-20 trace(A), a sweep without a rotation ends the iteration, 30 sweeps at the most.  The
// smallest diagonal entry (the lowest index among equals) names the column of V.  Returns the sweeps that rotated.
// A and V are indexed at run time: the kernel keeps them in LDS (register arrays would go to scratch).
HESS_GEOM_HD inline int geom_refit_eigen(double* A, double* V, double (&x)[9]) {
  double tr = 0.0;
  for (int i = 0; i < 9; i++) {
    tr += fabs(A[10 * i]);
    for (int j = 0; j < 9; j++) V[9 * i + j] = i == j ? 1.0 : 0.0;
  }
  const double tiny = 1.0e-20 * tr;
  int sweeps = 0;
  for (; sweeps < 30; sweeps++) {
    bool rotated = false;
    for (int p = 0; p < 8; p++)
      for (int q = p + 1; q < 9; q++) {
        const double apq = A[9 * p + q];
        if (!(fabs(apq) > tiny)) continue;
        rotated = true;
        // t = tan of the rotation angle, the root of t^2 + 2 t theta - 1 of smaller magnitude, theta = (aqq - app) / (2 apq)
        const double d = A[10 * q] - A[10 * p];
        const double t = (d >= 0.0 ? 2.0 : -2.0) * apq / (fabs(d) + sqrt(fma(d, d, 4.0 * apq * apq)));
        const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = c * t;
        for (int k = 0; k < 9; k++) {  // columns p and q of A and of V
          const double ap = A[9 * k + p], aq = A[9 * k + q], vp = V[9 * k + p], vq = V[9 * k + q];
          A[9 * k + p] = c * ap - s * aq;
          A[9 * k + q] = s * ap + c * aq;
          V[9 * k + p] = c * vp - s * vq;
          V[9 * k + q] = s * vp + c * vq;
        }
        for (int k = 0; k < 9; k++) {  // rows p and q of A
          const double ap = A[9 * p + k], aq = A[9 * q + k];
          A[9 * p + k] = c * ap - s * aq;
          A[9 * q + k] = s * ap + c * aq;
        }
        A[9 * p + q] = A[9 * q + p] = 0.0;
      }
    if (!rotated) break;
  }
  int j = 0;
  for (int i = 1; i < 9; i++) j = A[10 * i] < A[10 * j] ? i : j;
  double n = 0.0;
  for (int i = 0; i < 9; i++) n = fma(V[9 * i + j], V[9 * i + j], n);
  n = 1.0 / sqrt(n);
  for (int i = 0; i < 9; i++) x[i] = V[9 * i + j] * n;
  return sweeps;
}

// One rotation of the one-sided Jacobi SVD: makes columns P and Q of w orthogonal, v collects the rotations.
template <int P, int Q>
HESS_GEOM_HD inline bool geom_rotate(double (&w)[9], double (&v)[9]) {
  double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    al = fma(w[3 * r + P], w[3 * r + P], al);
    be = fma(w[3 * r + Q], w[3 * r + Q], be);
    ga = fma(w[3 * r + P], w[3 * r + Q], ga);
  }
  if (ga == 0.0 || fabs(ga) <= 1.0e-17 * sqrt(al * be)) return false;
  const double ze = (be - al) / (2.0 * ga);
  const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double wp = w[3 * r + P], wq = w[3 * r + Q], vp = v[3 * r + P], vq = v[3 * r + Q];
    w[3 * r + P] = c * wp - s * wq;
    w[3 * r + Q] = s * wp + c * wq;
    v[3 * r + P] = c * vp - s * vq;
    v[3 * r + Q] = s * vp + c * vq;
  }
  return true;
}

// The matrix as returned: for F the nearest rank-2 matrix (A V = W with orthogonal columns, the shortest column of W zeroed,
// A' = W' V^T), then unit Frobenius norm.
HESS_GEOM_HD inline void geom_finalise(int model, double (&m)[9]) {
  if (model == GEOM_MODEL_F) {
    double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 30; sweep++) {
      const bool r01 = geom_rotate<0, 1>(m, v), r02 = geom_rotate<0, 2>(m, v), r12 = geom_rotate<1, 2>(m, v);
      if (!(r01 || r02 || r12)) break;
    }
    double n[3];
#pragma unroll
    for (int c = 0; c < 3; c++) n[c] = m[c] * m[c] + m[3 + c] * m[3 + c] + m[6 + c] * m[6 + c];
    const int z = n[0] <= n[1] && n[0] <= n[2] ? 0 : (n[1] <= n[2] ? 1 : 2);
    double a[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (k == z ? 0.0 : m[3 * r + k]) * v[3 * c + k];
        a[3 * r + c] = s;
      }
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = a[i];
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; i++) s += m[i] * m[i];
  s = 1.0 / sqrt(s);
#pragma unroll
  for (int i = 0; i < 9; i++) m[i] *= s;
}

// The normalisation of one iteration: p_n = s (p - c) per image.
struct GeomRefitNorm {
  double c1x, c1y, s1, c2x, c2y, s2;
};

// Step 4 from the eigenvector x (normalised coordinates) on: T2^-1 X T1 (H) or T2^T X T1 (F) in double, geom_finalise, the
// sign for which sum C_i prev_i >= 0, rounded to float32.  false: an entry is not finite -- stop.
HESS_GEOM_HD inline bool geom_refit_candidate(int model, const double (&x)[9], const GeomRefitNorm& nm, const float (&prev)[9],
                                              float (&C)[9]) {
  double g[9], m[9];
  for (int r = 0; r < 3; r++) {  // G = X T1, T1 = [s1 0 -s1 c1x; 0 s1 -s1 c1y; 0 0 1]
    g[3 * r] = x[3 * r] * nm.s1;
    g[3 * r + 1] = x[3 * r + 1] * nm.s1;
    g[3 * r + 2] = x[3 * r + 2] - nm.s1 * (x[3 * r] * nm.c1x + x[3 * r + 1] * nm.c1y);
  }
  for (int c = 0; c < 3; c++) {
    if (model == GEOM_MODEL_H) {  // T2^-1 = [1/s2 0 c2x; 0 1/s2 c2y; 0 0 1]
      m[c] = g[c] / nm.s2 + nm.c2x * g[6 + c];
      m[3 + c] = g[3 + c] / nm.s2 + nm.c2y * g[6 + c];
      m[6 + c] = g[6 + c];
    } else {                      // T2^T = [s2 0 0; 0 s2 0; -s2 c2x  -s2 c2y  1]
      m[c] = nm.s2 * g[c];
      m[3 + c] = nm.s2 * g[3 + c];
      m[6 + c] = g[6 + c] - nm.s2 * (nm.c2x * g[c] + nm.c2y * g[3 + c]);
    }
  }
  geom_finalise(model, m);
  double dot = 0.0;
  for (int i = 0; i < 9; i++) dot = fma(m[i], (double)prev[i], dot);
  const double sign = dot >= 0.0 ? 1.0 : -1.0;
  bool ok = true;
  for (int i = 0; i < 9; i++) {
    C[i] = (float)(sign * m[i]);
    ok = ok && fabsf(C[i]) <= 3.0e38f;  // (false for NaN and infinity)
  }
  return ok;
}

// Step 5 from the counts: the inliers before, the candidate's, and the correspondences on which the two masks differ.
enum { GEOM_REFIT_DISCARD = 0, GEOM_REFIT_ACCEPT = 1, GEOM_REFIT_ACCEPT_AND_STOP = 2 };
HESS_GEOM_HD inline int geom_refit_decide(int before, int candidate, int differ) {
  if (candidate < before) return GEOM_REFIT_DISCARD;
  return differ == 0 ? GEOM_REFIT_ACCEPT_AND_STOP : GEOM_REFIT_ACCEPT;
}

#endif  // HESS_GEOM_REFIT_H
