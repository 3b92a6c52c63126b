// hess_guided_gate.h -- the gate of guided matching (GetGuidedSiftMatch: MultiplyDescriptorG_Kernel, ProgramCU.cu:3618-3638),
// written once for match_dot_kernel, match_mfma_kernel<GUIDED> (hess_match.hip) and geom_gate (hess_geom.hip).  Standard
// headers only, so that tests/guided_gate_main.cpp runs it on the CPU.
//
// A pair (i, j) passes when the homography H maps location l1 of row i into the box of half width hdistmax around location
// l2 of column j, and the Sampson error of (l1, l2) under the fundamental matrix F is below fdistmax.  Everything that
// depends on the row alone (guided_row_h, guided_row_f) or on the column alone (guided_col) is split from the decision
// (guided_box, guided_sampson): the same operations on the same operands in the same order as the per-element form, and the
// build has -ffp-contract=off, so hoisting the terms out of an n1 x n2 loop changes no bit of any decision.  Anything
// non-finite (x2 == 0, a zero matrix) fails its comparison.
#ifndef HESS_GUIDED_GATE_H
#define HESS_GUIDED_GATE_H
#include <cmath>

#if defined(__HIPCC__)
#define HESS_GATE_FN __host__ __device__ inline
#else
#define HESS_GATE_FN inline
#endif

namespace hess {

struct GuidedRow { float px, py, fx0, fx1, fx2, rr; };  // H l1 projected; F l1 and the row's half of the Sampson denominator
struct GuidedCol { float x, y, ft0, ft1; };             // l2; the first two components of F^T l2

HESS_GATE_FN void guided_row_h(const float* H, float x, float y, GuidedRow& r) {
  const float x0 = fmaf(H[0], x, H[1] * y) + H[2];
  const float x1 = fmaf(H[3], x, H[4] * y) + H[5];
  const float x2 = fmaf(H[6], x, H[7] * y) + H[8];
  r.px = x0 / x2;
  r.py = x1 / x2;
}

HESS_GATE_FN void guided_row_f(const float* F, float x, float y, GuidedRow& r) {
  r.fx0 = fmaf(F[0], x, F[1] * y) + F[2];
  r.fx1 = fmaf(F[3], x, F[4] * y) + F[5];
  r.fx2 = fmaf(F[6], x, F[7] * y) + F[8];
  r.rr = fmaf(r.fx0, r.fx0, r.fx1 * r.fx1);
}

HESS_GATE_FN GuidedCol guided_col(const float* F, float x, float y) {
  GuidedCol c;
  c.x = x;
  c.y = y;
  c.ft0 = fmaf(F[0], x, F[3] * y) + F[6];
  c.ft1 = fmaf(F[1], x, F[4] * y) + F[7];
  return c;
}

HESS_GATE_FN bool guided_box(const GuidedRow& r, float x, float y, float hdistmax) {
  return fabsf(r.px - x) < hdistmax && fabsf(r.py - y) < hdistmax;
}

HESS_GATE_FN bool guided_sampson(const GuidedRow& r, const GuidedCol& c, float fdistmax) {
  const float x2fx1 = fmaf(c.x, r.fx0, c.y * r.fx1) + r.fx2;
  const float se = (x2fx1 * x2fx1) / fmaf(c.ft1, c.ft1, fmaf(c.ft0, c.ft0, r.rr));
  return se < fdistmax;
}

HESS_GATE_FN bool guided_pass(const GuidedRow& r, const GuidedCol& c, float hdistmax, float fdistmax) {
  return guided_box(r, c.x, c.y, hdistmax) && guided_sampson(r, c, fdistmax);
}

}  // namespace hess

#endif  // HESS_GUIDED_GATE_H
