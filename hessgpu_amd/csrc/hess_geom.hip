// hess_geom.hip -- two-view geometry from matches on the matcher's device: a deterministic, fixed-budget RANSAC for a
// homography or a fundamental matrix (hess_matcher_estimate, hess_matcher_estimate_pairs; the rule is stated in
// include/hess_abi.h).  No reference counterpart: SiftMatchGPU's callers do this step on the host.
//
//   geom_score_kernel    one workgroup per (pair, block of 256 hypotheses) of a work table, one hypothesis per lane: sample
//                        (geom_sample), solve in registers (geom_null_vector: fully unrolled Gauss-Jordan in double, pivots
//                        by selects), then count the pair's correspondences that pass the gate -- gathered once per
//                        workgroup into LDS as float4 (x1, y1, x2, y2), 2048 at a time, every lane reading the same
//                        address (a broadcast) -- and store the block's best (score, lowest t, matrix);
//   geom_finish_kernel   one workgroup per pair: arg-max over the block entries (score, then lowest t), rank 2 for F and
//                        unit norm in double (one thread), then the inlier mask with the guided gate's own formulas
//                        (hess_guided_gate.h, the matcher's) and its count;
//   geom_refit_kernel    only when params.refit > 0, one workgroup per pair after the finish kernel: up to `refit` times the
//                        least-squares DLT on the inliers (hess_abi.h, step 6) -- moment sums over the mask, the serial
//                        solve of hess_geom_refit.h on one lane, the candidate's mask into a second buffer, accept or stop;
//   geom_jobs_fill_kernel   the job and work tables of a chunk from match counts that only the device knows
//                        (hess_geom_enqueue for hess_matcher_verify_pairs: no host copy of the matches, no sync).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hess_abi.h"
#include "hess_geom_refit.h"
#include "hess_guided_gate.h"
#include "hess_matcher_int.h"

namespace {

constexpr int GEOM_CHUNK = 2048;        // correspondences in LDS at a time: 32 KB
constexpr int GEOM_DEFAULT_T = 2048;
constexpr int GEOM_MAX_T = 65536;       // 256 blocks of 256 hypotheses: one finish thread per block
constexpr int GEOM_PAIRS = 256;         // pairs per chunk (one set of launches), and
constexpr size_t GEOM_MATCHES = (size_t)4 << 20;  // correspondences per chunk (a pair above it is a chunk of its own)

constexpr int GEOM_MAX_REFIT = 8;
static_assert(GEOM_MODEL_H == HESS_GEOM_HOMOGRAPHY && GEOM_MODEL_F == HESS_GEOM_FUNDAMENTAL, "hess_geom_refit.h names the models");

constexpr int geom_k(int model) { return model == HESS_GEOM_HOMOGRAPHY ? 4 : 8; }

__host__ __device__ inline uint32_t geom_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// The sampling rule (hess_abi.h, step 1): k <= 8 distinct indices below n in draw order.  Compile-time indices only: with
// a constant k everything stays in registers.
__host__ __device__ inline void geom_sample(uint32_t seed, int t, int k, int n, int (&out)[8]) {
  const uint32_t h = geom_mix(geom_mix(seed ^ 0x9E3779B9u) + (uint32_t)t);
  int sorted[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    out[j] = 0;
    sorted[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (j < k) {
      int c = (int)(((uint64_t)geom_mix(h + (uint32_t)j) * (uint32_t)(n - j)) >> 32);
#pragma unroll
      for (int i = 0; i < j; i++) c += sorted[i] <= c ? 1 : 0;  // the earlier draws in ascending value
      out[j] = c;
#pragma unroll
      for (int i = j; i >= 0; i--) {  // insert c: sorted[0..j] ascending
        const int a = i < j ? sorted[i] : INT32_MAX, b = i > 0 ? sorted[i - 1] : -1;
        sorted[i] = a < c ? a : (b < c ? c : b);
      }
    }
  }
}

// The unit null vector direction x of the 8 x 9 matrix a (destroyed): Gauss-Jordan elimination with complete pivoting.
// Rows and columns are never moved: a pivot is the largest remaining |a[r][c]| over the unused rows and columns, found,
// read and applied through selects on compile-time indices, so the 72 entries stay in registers.  After eight steps one
// column f is left: x[f] = 1 and row r gives x[its pivot column] = -a[r][f] / a[r][pivot column].  A singular system
// divides by zero: the caller's finiteness test drops the hypothesis.  In double: in float32 the eight updates of every
// entry put the null vector up to 22 x (kappa 2^-24) from the exact one where a float32 SVD stays within 2 x
// (profiles/r18_estimate_tests.txt); the points around it stay float32.
__host__ __device__ inline void geom_null_vector(double (&a)[8][9], double (&x)[9]) {
  unsigned rused = 0, cused = 0;
  int pcol[8];
#pragma unroll
  for (int r = 0; r < 8; r++) pcol[r] = 0;
#pragma unroll
  for (int step = 0; step < 8; step++) {
    double best = -1.0;
    int pr = 0, pc = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const bool rfree = !((rused >> r) & 1u);
#pragma unroll
      for (int c = 0; c < 9; c++) {
        const double v = fabs(a[r][c]);
        const bool take = rfree && !((cused >> c) & 1u) && v > best;
        best = take ? v : best;
        pr = take ? r : pr;
        pc = take ? c : pc;
      }
    }
    rused |= 1u << pr;
    cused |= 1u << pc;
    double prow[9], piv = 0.0;
#pragma unroll
    for (int c = 0; c < 9; c++) {
      double v = a[0][c];
#pragma unroll
      for (int r = 1; r < 8; r++) v = pr == r ? a[r][c] : v;
      prow[c] = v;
      piv = pc == c ? v : piv;
    }
    const double inv = 1.0 / piv;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      double f = a[r][0];
#pragma unroll
      for (int c = 1; c < 9; c++) f = pc == c ? a[r][c] : f;
      f = pr == r ? 0.0 : f * inv;
      pcol[r] = pr == r ? pc : pcol[r];
#pragma unroll
      for (int c = 0; c < 9; c++) a[r][c] = fma(-f, prow[c], a[r][c]);
    }
  }
  int fc = 0;
#pragma unroll
  for (int c = 0; c < 9; c++) fc = ((cused >> c) & 1u) ? fc : c;
#pragma unroll
  for (int c = 0; c < 9; c++) x[c] = fc == c ? 1.0 : 0.0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    double num = a[r][0], den = a[r][0];
#pragma unroll
    for (int c = 1; c < 9; c++) {
      num = fc == c ? a[r][c] : num;
      den = pcol[r] == c ? a[r][c] : den;
    }
    const double v = -num / den;
#pragma unroll
    for (int c = 0; c < 9; c++) x[c] = pcol[r] == c ? v : x[c];
  }
}

// Hartley normalisation of K points: centre and scale s with mean distance sqrt 2, p_n = s (p - c).
template <int K>
__host__ __device__ inline void geom_normalise(float (&x)[K], float (&y)[K], float& cx, float& cy, float& s) {
  float sx = 0.0f, sy = 0.0f;
#pragma unroll
  for (int i = 0; i < K; i++) {
    sx += x[i];
    sy += y[i];
  }
  cx = sx * (1.0f / K);
  cy = sy * (1.0f / K);
  float d = 0.0f;
#pragma unroll
  for (int i = 0; i < K; i++) {
    x[i] -= cx;
    y[i] -= cy;
    d += sqrtf(fmaf(x[i], x[i], y[i] * y[i]));
  }
  s = 1.41421356237f * K / d;
#pragma unroll
  for (int i = 0; i < K; i++) {
    x[i] *= s;
    y[i] *= s;
  }
}

// The hypothesis of geom_k(MODEL) correspondences (x1, y1) -> (x2, y2) in pixel coordinates (destroyed); false: not finite.
template <int MODEL>
__host__ __device__ inline bool geom_hypothesis(float (&x1)[geom_k(MODEL)], float (&y1)[geom_k(MODEL)],
                                                float (&x2)[geom_k(MODEL)], float (&y2)[geom_k(MODEL)], float (&M)[9]) {
  constexpr int K = geom_k(MODEL);
  float c1x, c1y, s1, c2x, c2y, s2;
  geom_normalise<K>(x1, y1, c1x, c1y, s1);
  geom_normalise<K>(x2, y2, c2x, c2y, s2);
  double a[8][9];
#pragma unroll
  for (int i = 0; i < K; i++) {
    const double x = x1[i], y = y1[i], u = x2[i], v = y2[i];
    if (MODEL == HESS_GEOM_HOMOGRAPHY) {  // u (h6 x + h7 y + h8) = h0 x + h1 y + h2, and the same for v
      double(&r0)[9] = a[(2 * i) & 7];
      double(&r1)[9] = a[(2 * i + 1) & 7];
      r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = -u;
      r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -v * x; r1[7] = -v * y; r1[8] = -v;
    } else {                              // (u, v, 1) F (x, y, 1)^T = 0
      double(&r)[9] = a[i & 7];
      r[0] = u * x; r[1] = u * y; r[2] = u; r[3] = v * x; r[4] = v * y; r[5] = v; r[6] = x; r[7] = y; r[8] = 1.0;
    }
  }
  double hd[9];
  geom_null_vector(a, hd);
  float h[9];
#pragma unroll
  for (int c = 0; c < 9; c++) h[c] = (float)hd[c];
  // G = h T1, T1 = [s1 0 -s1 c1x; 0 s1 -s1 c1y; 0 0 1]
  float G[9];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    G[3 * r] = h[3 * r] * s1;
    G[3 * r + 1] = h[3 * r + 1] * s1;
    G[3 * r + 2] = h[3 * r + 2] - s1 * fmaf(h[3 * r], c1x, h[3 * r + 1] * c1y);
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (MODEL == HESS_GEOM_HOMOGRAPHY) {  // H = T2^-1 G, T2^-1 = [1/s2 0 c2x; 0 1/s2 c2y; 0 0 1]
      M[c] = fmaf(c2x, G[6 + c], G[c] / s2);
      M[3 + c] = fmaf(c2y, G[6 + c], G[3 + c] / s2);
      M[6 + c] = G[6 + c];
    } else {                              // F = T2^T G, T2^T = [s2 0 0; 0 s2 0; -s2 c2x  -s2 c2y  1]
      M[c] = s2 * G[c];
      M[3 + c] = s2 * G[3 + c];
      M[6 + c] = G[6 + c] - s2 * fmaf(c2x, G[c], c2y * G[3 + c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 9; c++) ok = ok && fabsf(M[c]) <= 3.0e38f;  // (false for NaN and infinity)
  return ok;
}

// Scoring test of a hypothesis: the gate's inequalities multiplied through by their (positive) denominators.
template <int MODEL>
__host__ __device__ inline bool geom_pass(const float (&M)[9], const float4 p, float bound) {
  if (MODEL == HESS_GEOM_HOMOGRAPHY) {
    const float x0 = fmaf(M[0], p.x, M[1] * p.y) + M[2];
    const float x1 = fmaf(M[3], p.x, M[4] * p.y) + M[5];
    const float x2 = fmaf(M[6], p.x, M[7] * p.y) + M[8];
    const float lim = bound * fabsf(x2);
    return fabsf(fmaf(-x2, p.z, x0)) < lim && fabsf(fmaf(-x2, p.w, x1)) < lim;
  } else {
    const float fx0 = fmaf(M[0], p.x, M[1] * p.y) + M[2];
    const float fx1 = fmaf(M[3], p.x, M[4] * p.y) + M[5];
    const float fx2 = fmaf(M[6], p.x, M[7] * p.y) + M[8];
    const float ft0 = fmaf(M[0], p.z, M[3] * p.w) + M[6];
    const float ft1 = fmaf(M[1], p.z, M[4] * p.w) + M[7];
    const float s = fmaf(p.z, fx0, p.w * fx1) + fx2;
    return s * s < bound * fmaf(ft1, ft1, fmaf(ft0, ft0, fmaf(fx0, fx0, fx1 * fx1)));
  }
}

// The guided gate itself (hess_guided_gate.h, the matcher's own): the mask's decision.
template <int MODEL>
__host__ __device__ inline bool geom_gate(const float (&M)[9], const float2 l1, const float2 l2, float bound) {
  hess::GuidedRow R;
  if (MODEL == HESS_GEOM_HOMOGRAPHY) {
    hess::guided_row_h(M, l1.x, l1.y, R);
    return hess::guided_box(R, l2.x, l2.y, bound);
  } else {
    hess::guided_row_f(M, l1.x, l1.y, R);
    return hess::guided_sampson(R, hess::guided_col(M, l2.x, l2.y), bound);
  }
}

// One pair of a launch: the locations of its two sets, its matches (and mask bytes) from moff on, its block entries from boff.
struct GeomJob {
  const float2 *l1, *l2;
  int moff, n;
  uint32_t seed;
  int boff, nblk, pad;
};
// The best hypothesis of one block of 256.
struct GeomBest {
  int score, t;
  float M[9];
  int pad;
};

__device__ __forceinline__ unsigned long long geom_key(int score, int t) {  // larger score, then lower t
  return ((unsigned long long)(unsigned)(score + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t);
}

__device__ __forceinline__ unsigned long long geom_block_max(unsigned long long key, unsigned long long* wmax) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = key;
  __syncthreads();
  const unsigned long long a = wmax[0] > wmax[1] ? wmax[0] : wmax[1], b = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
  return a > b ? a : b;
}

// work[blockIdx.x] = (job, block of hypotheses); a table built on the host lists only jobs with n >= k.
template <int MODEL>
__global__ __launch_bounds__(256) void geom_score_kernel(const GeomJob* jobs, const int2* work, const int2* matches, int T,
                                                         float bound, GeomBest* best) {
  constexpr int K = geom_k(MODEL);
  __shared__ float4 pts[GEOM_CHUNK];
  __shared__ unsigned long long wmax[4];
  const int2 w = work[blockIdx.x];
  const GeomJob J = jobs[w.x];
  // (workgroup-uniform, before any barrier.)  Only a table filled on the device (geom_jobs_fill_kernel) lists such a job:
  // geom_sample is undefined for n < k, and the finish kernel reads none of its block entries (nblk = 0)
  if (J.n < K) return;
  const int2* const mt = matches + J.moff;
  const int tid = threadIdx.x, t = w.y * 256 + tid;
  float M[9];
  bool live = t < T;
  {
    int idx[8];
    geom_sample(J.seed, live ? t : 0, K, J.n, idx);
    float x1[K], y1[K], x2[K], y2[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int2 m = mt[idx[j]];
      const float2 a = J.l1[m.x], b = J.l2[m.y];
      x1[j] = a.x; y1[j] = a.y; x2[j] = b.x; y2[j] = b.y;
    }
    const bool finite = geom_hypothesis<MODEL>(x1, y1, x2, y2, M);
    if (!finite) {  // scores 0
#pragma unroll
      for (int c = 0; c < 9; c++) M[c] = 0.0f;
    }
  }
  int score = 0;
  for (int base = 0; base < J.n; base += GEOM_CHUNK) {
    const int cnt = min(GEOM_CHUNK, J.n - base);
    if (base) __syncthreads();  // every lane is done with the chunk before
    for (int i = tid; i < cnt; i += 256) {
      const int2 m = mt[base + i];
      const float2 a = J.l1[m.x], b = J.l2[m.y];
      pts[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < cnt; i++) score += geom_pass<MODEL>(M, pts[i], bound) ? 1 : 0;
  }
  const unsigned long long key = live ? geom_key(score, t) : 0ull;
  const unsigned long long top = geom_block_max(key, wmax);
  if (live && key == top) {
    GeomBest e;
    e.score = score;
    e.t = t;
#pragma unroll
    for (int c = 0; c < 9; c++) e.M[c] = M[c];
    e.pad = 0;
    best[J.boff + w.y] = e;
  }
}

template <int MODEL>
__global__ __launch_bounds__(256) void geom_finish_kernel(const GeomJob* jobs, const int2* matches, const GeomBest* best,
                                                          float bound, hess_geom_result* results, unsigned char* mask) {
  constexpr int K = geom_k(MODEL);
  __shared__ unsigned long long wmax[4];
  __shared__ float sM[9];
  __shared__ int wcnt[4];
  const GeomJob J = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  GeomBest e;
  e.score = -1;
  e.t = 0;
  unsigned long long key = 0ull;
  if (tid < J.nblk) {
    e = best[J.boff + tid];
    key = geom_key(e.score, e.t);
  }
  const unsigned long long top = geom_block_max(key, wmax);
  const int score = (int)(top >> 32) - 1;
  unsigned char* const mk = mask + J.moff;
  hess_geom_result* const R = results + blockIdx.x;
  if (J.n < K || score < K) {  // no model (workgroup-uniform)
    for (int i = tid; i < J.n; i += 256) mk[i] = 0;
    if (tid < 9) R->M[tid] = 0.0f;
    if (tid == 0) {
      R->inliers = 0;
      R->hypothesis = -1;
      R->reserved[0] = R->reserved[1] = 0;
    }
    return;
  }
  if (key == top) {  // one thread: the keys of a pair are distinct
    double m[9];
#pragma unroll
    for (int c = 0; c < 9; c++) m[c] = (double)e.M[c];
    geom_finalise(MODEL, m);
#pragma unroll
    for (int c = 0; c < 9; c++) sM[c] = (float)m[c];
  }
  __syncthreads();
  float M[9];
#pragma unroll
  for (int c = 0; c < 9; c++) M[c] = sM[c];
  const int2* const mt = matches + J.moff;
  int cnt = 0;
  for (int i = tid; i < J.n; i += 256) {
    const int2 q = mt[i];
    const bool in = geom_gate<MODEL>(M, J.l1[q.x], J.l2[q.y], bound);
    mk[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid < 9) R->M[tid] = M[tid];
  if (tid == 0) {
    R->inliers = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    R->hypothesis = (int)(0xFFFFFFFFu - (unsigned)(top & 0xFFFFFFFFull));
    R->reserved[0] = R->reserved[1] = 0;
  }
}

// Sums of a workgroup in one fixed order: xor butterflies over the 64 lanes of a wavefront (a + b = b + a: every lane holds
// the same bits), then (w0 + w1) + (w2 + w3) over the four wavefronts.  red: [4][NV] in LDS.  Every thread gets the totals.
template <int NV>
__device__ __forceinline__ void geom_block_sum(double (&v)[NV], double* red) {
#pragma unroll
  for (int j = 0; j < NV; j++) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[j] += __shfl_xor(v[j], d);
  }
  __syncthreads();  // the totals of the sum before have been read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; j++) red[(threadIdx.x >> 6) * NV + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; j++) v[j] = (red[j] + red[NV + j]) + (red[2 * NV + j] + red[3 * NV + j]);
}

// The refit of hess_abi.h, step 6: blockIdx.x = the pair of the chunk, after geom_finish_kernel wrote its result and mask.
// Order of every sum over the inliers (it depends on the match list and the mask alone): lane l of 256 adds the inliers
// i = l, l + 256, l + 512, ... in ascending i (the LDS chunk of 2048 is a multiple of 256), then geom_block_sum's tree.
// Per iteration three passes over the correspondences (centroid sums; distances to the centroids; the moment sums of
// geom_refit_moments in normalised coordinates, all in double from the float32 locations), the serial solve on thread 0 with
// its two 9 x 9 matrices in LDS, and the gate pass that writes the candidate's mask to cand[] and counts it.  A list of at
// most GEOM_CHUNK correspondences is staged in LDS once, a longer one chunk by chunk in every pass.  Every mask byte is
// read and written by the thread that owns its index modulo 256: no ordering between threads is needed on mask or cand.
template <int MODEL>
__global__ __launch_bounds__(256) void geom_refit_kernel(const GeomJob* jobs, const int2* matches, float bound, int refit,
                                                         hess_geom_result* results, unsigned char* mask, unsigned char* cand) {
  constexpr int K = geom_k(MODEL), NS = geom_refit_sums(MODEL);
  __shared__ float4 pts[GEOM_CHUNK];
  __shared__ double red[4 * NS];
  __shared__ double sS[NS], sA[81], sV[81];
  __shared__ float sC[9];
  __shared__ int sok;
  __shared__ int wcnt[8];
  const GeomJob J = jobs[blockIdx.x];
  hess_geom_result* const R = results + blockIdx.x;
  if (R->hypothesis < 0) return;  // no model (workgroup-uniform; R is written at the end only)
  const int tid = threadIdx.x, n = J.n;
  const int2* const mt = matches + J.moff;
  unsigned char* const mk = mask + J.moff;
  unsigned char* const cd = cand + J.moff;
  float M[9];
#pragma unroll
  for (int c = 0; c < 9; c++) M[c] = R->M[c];
  const int first = R->inliers;
  int inl = first, refits = 0;
  const bool one = n <= GEOM_CHUNK;
  auto stage = [&](int base, int cnt) {
    __syncthreads();  // every lane is done with the chunk before
    for (int i = tid; i < cnt; i += 256) {
      const int2 m = mt[base + i];
      const float2 a = J.l1[m.x], b = J.l2[m.y];
      pts[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    __syncthreads();
  };
  if (one) stage(0, n);
  for (int r = 0; r < refit; r++) {
    if (inl < K) break;
    GeomRefitNorm nm;
    {  // centroids
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      for (int base = 0; base < n; base += GEOM_CHUNK) {
        const int cnt = min(GEOM_CHUNK, n - base);
        if (!one) stage(base, cnt);
        for (int i = tid; i < cnt; i += 256)
          if (mk[base + i]) {
            const float4 p = pts[i];
            s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z; s[3] += (double)p.w;
          }
      }
      geom_block_sum<4>(s, red);
      nm.c1x = s[0] / inl; nm.c1y = s[1] / inl; nm.c2x = s[2] / inl; nm.c2y = s[3] / inl;
    }
    {  // mean distances
      double s[2] = {0.0, 0.0};
      for (int base = 0; base < n; base += GEOM_CHUNK) {
        const int cnt = min(GEOM_CHUNK, n - base);
        if (!one) stage(base, cnt);
        for (int i = tid; i < cnt; i += 256)
          if (mk[base + i]) {
            const float4 p = pts[i];
            const double x = (double)p.x - nm.c1x, y = (double)p.y - nm.c1y, u = (double)p.z - nm.c2x, v = (double)p.w - nm.c2y;
            s[0] += sqrt(fma(x, x, y * y));
            s[1] += sqrt(fma(u, u, v * v));
          }
      }
      geom_block_sum<2>(s, red);
      if (!geom_refit_scales(inl, s[0], s[1], nm.s1, nm.s2)) break;  // (the same bits in every thread)
    }
    {  // moment sums, then the solve on one lane
      double acc[NS];
#pragma unroll
      for (int j = 0; j < NS; j++) acc[j] = 0.0;
      for (int base = 0; base < n; base += GEOM_CHUNK) {
        const int cnt = min(GEOM_CHUNK, n - base);
        if (!one) stage(base, cnt);
        for (int i = tid; i < cnt; i += 256)
          if (mk[base + i]) {
            const float4 p = pts[i];
            geom_refit_moments<MODEL>(nm.s1 * ((double)p.x - nm.c1x), nm.s1 * ((double)p.y - nm.c1y),
                                      nm.s2 * ((double)p.z - nm.c2x), nm.s2 * ((double)p.w - nm.c2y), acc);
          }
      }
      geom_block_sum<NS>(acc, red);
      if (tid == 0) {
#pragma unroll
        for (int j = 0; j < NS; j++) sS[j] = acc[j];
        geom_refit_normal(MODEL, sS, sA);
        double x[9];
        geom_refit_eigen(sA, sV, x);
        float C[9];
        sok = geom_refit_candidate(MODEL, x, nm, M, C) ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 9; c++) sC[c] = C[c];
      }
      __syncthreads();
    }
    if (!sok) break;
    float C[9];
#pragma unroll
    for (int c = 0; c < 9; c++) C[c] = sC[c];
    int cnt_in = 0, differ = 0;
    for (int base = 0; base < n; base += GEOM_CHUNK) {
      const int cnt = min(GEOM_CHUNK, n - base);
      if (!one) stage(base, cnt);
      for (int i = tid; i < cnt; i += 256) {
        const float4 p = pts[i];
        const bool in = geom_gate<MODEL>(C, make_float2(p.x, p.y), make_float2(p.z, p.w), bound);
        cd[base + i] = in ? 1 : 0;
        cnt_in += in ? 1 : 0;
        differ += (in ? 1 : 0) != (int)mk[base + i] ? 1 : 0;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      cnt_in += __shfl_xor(cnt_in, d);
      differ += __shfl_xor(differ, d);
    }
    __syncthreads();  // sok, sC and wcnt of the iteration before have been read
    if ((tid & 63) == 0) {
      wcnt[tid >> 6] = cnt_in;
      wcnt[4 + (tid >> 6)] = differ;
    }
    __syncthreads();
    cnt_in = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    differ = wcnt[4] + wcnt[5] + wcnt[6] + wcnt[7];
    const int what = geom_refit_decide(inl, cnt_in, differ);
    if (what == GEOM_REFIT_DISCARD) break;
    for (int i = tid; i < n; i += 256) mk[i] = cd[i];
#pragma unroll
    for (int c = 0; c < 9; c++) M[c] = C[c];
    inl = cnt_in;
    refits++;
    if (what == GEOM_REFIT_ACCEPT_AND_STOP) break;
  }
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < 9; c++) R->M[c] = M[c];
    R->inliers = inl;
    R->refits = refits;
    R->ransac_inliers = first;
  }
}

// The job and work tables of a chunk whose match counts are known on the device alone (hess_matcher_verify_pairs): pair q
// has its matches and mask bytes at q * mm, counts[q] of them, seed0 + q as its seed, its sets' locations from loc +
// lalb[q].x and .y on, and nblk block entries from q * nblk on; the work table lists every (pair, block), and a pair with
// fewer than K matches gets nblk = 0, which geom_score_kernel's early return and geom_finish_kernel's no-model branch honour.
__global__ __launch_bounds__(256) void geom_jobs_fill_kernel(const int2* lalb, const int* counts, const float2* loc, int np,
                                                             int mm, int nblk, int K, uint32_t seed0, GeomJob* jobs,
                                                             int2* work) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < np) {
    const int2 l = lalb[i];
    const int n = counts[i];
    GeomJob J;
    J.l1 = loc + l.x;
    J.l2 = loc + l.y;
    J.moff = i * mm;
    J.n = n;
    J.seed = seed0 + (uint32_t)i;
    J.boff = i * nblk;
    J.nblk = n >= K ? nblk : 0;
    J.pad = 0;
    jobs[i] = J;
  }
  if (i < np * nblk) work[i] = make_int2(i / nblk, i % nblk);
}

}  // namespace

// The estimator's scratch: one chunk's plan (jobs, work table), matches, block entries, results and masks.
struct hess_geom_state {
  DeviceBuf<unsigned char> plan, mask;
  DeviceBuf<int2> matches;
  DeviceBuf<GeomBest> best;
  DeviceBuf<hess_geom_result> results;
  DeviceBuf<unsigned char> cand;  // the refit's candidate masks (only with params.refit > 0)
};

void hess_geom_state_destroy(hess_geom_state* g) { delete g; }

namespace {

hess_geom_state* geom_state(hess_matcher_view& v) {
  if (!*v.geom) v.geom->reset(new (std::nothrow) hess_geom_state());
  return v.geom->get();
}

// One pair as the caller gave it: the locations and sizes of its two sets, its n matches (i of set 1, j of set 2).
struct GeomPair {
  const float2 *l1, *l2;
  int n1, n2;
  const int* matches;
  int n;
  uint32_t seed;
};

int geom_params_check(hess_matcher_view& v, const hess_geom_params* P, const char* what) {
  const std::string w = what;
  if (!P) { v.err = w + ": params is NULL"; return HESS_ERR_ARG; }
  if (P->model != HESS_GEOM_HOMOGRAPHY && P->model != HESS_GEOM_FUNDAMENTAL) {
    v.err = w + ": params.model must be HESS_GEOM_HOMOGRAPHY (1) or HESS_GEOM_FUNDAMENTAL (2), not " + std::to_string(P->model);
    return HESS_ERR_ARG;
  }
  if (P->hypotheses < 0 || P->hypotheses > GEOM_MAX_T) {
    v.err = w + ": params.hypotheses must lie in 0..65536, not " + std::to_string(P->hypotheses);
    return HESS_ERR_ARG;
  }
  if (P->refit < 0 || P->refit > GEOM_MAX_REFIT) {
    v.err = w + ": params.refit must lie in 0..8, not " + std::to_string(P->refit);
    return HESS_ERR_ARG;
  }
  for (int k = 1; k < 4; k++)
    if (P->reserved[k]) { v.err = w + ": params.reserved[" + std::to_string(k) + "] must be zero"; return HESS_ERR_ARG; }
  if (!(P->bound > 0.0f) || !std::isfinite(P->bound)) {
    v.err = w + ": params.bound must be finite and greater than 0";
    return HESS_ERR_ARG;
  }
  return 0;
}

// Every index of every pair lies in its set, or HESS_ERR_ARG naming the first that does not.
int geom_matches_check(hess_matcher_view& v, const std::vector<GeomPair>& pairs, const char* what) {
  for (size_t p = 0; p < pairs.size(); p++) {
    const GeomPair& G = pairs[p];
    for (int i = 0; i < G.n; i++) {
      const int a = G.matches[2 * i], b = G.matches[2 * i + 1];
      if (a < 0 || a >= G.n1 || b < 0 || b >= G.n2) {
        v.err = std::string(what) + ": match " + std::to_string(i) + " of pair " + std::to_string(p) + " is (" + std::to_string(a) +
                 ", " + std::to_string(b) + "), outside its sets of " + std::to_string(G.n1) + " and " + std::to_string(G.n2);
        return HESS_ERR_ARG;
      }
    }
  }
  return 0;
}

// The launches of one chunk: jobs and work table as laid out in a plan buffer (np jobs, then nwork entries), the matches and
// the result and mask buffers the jobs' offsets index.
struct GeomBuffers {
  const unsigned char* plan;
  const int2* matches;
  GeomBest* best;
  hess_geom_result* results;
  unsigned char *mask, *cand;
};

template <int MODEL>
hipError_t geom_launch(hipStream_t st, const GeomBuffers& b, int np, size_t nwork, int T, float bound, int refit) {
  const GeomJob* djobs = reinterpret_cast<const GeomJob*>(b.plan);
  const int2* dwork = reinterpret_cast<const int2*>(b.plan + (size_t)np * sizeof(GeomJob));
  if (nwork)
    hipLaunchKernelGGL(geom_score_kernel<MODEL>, dim3((unsigned)nwork), dim3(256), 0, st, djobs, dwork, b.matches, T, bound,
                       b.best);
  hipLaunchKernelGGL(geom_finish_kernel<MODEL>, dim3((unsigned)np), dim3(256), 0, st, djobs, b.matches, b.best, bound,
                     b.results, b.mask);
  if (refit > 0)
    hipLaunchKernelGGL(geom_refit_kernel<MODEL>, dim3((unsigned)np), dim3(256), 0, st, djobs, b.matches, bound, refit, b.results,
                       b.mask, b.cand);
  return hipGetLastError();
}

// The checked pairs in chunks: per chunk one upload (jobs, work table, matches), the two launches (three with a refit), one
// download (results, masks).  inlier: pair p's bytes at inlier + p * pitch, or NULL.
int geom_run(hess_matcher_view& v, const std::vector<GeomPair>& pairs, const hess_geom_params& P, hess_geom_result* out,
             unsigned char* inlier, size_t pitch) {
  hess_geom_state* const g = geom_state(v);
  if (!g) { v.err = "estimate: out of memory"; return HESS_ERR_NOMEM; }
  const int K = geom_k(P.model), T = P.hypotheses ? P.hypotheses : GEOM_DEFAULT_T, nblk = (T + 255) / 256;
  *v.last_ms = 0.0f;
  float total_ms = 0.0f;
  std::vector<unsigned char> hplan, hmask;
  std::vector<int> hmatch;
  std::vector<hess_geom_result> hres;
  for (size_t p0 = 0; p0 < pairs.size();) {
    size_t p1 = p0, nm = 0;
    while (p1 < pairs.size() && p1 - p0 < (size_t)GEOM_PAIRS && (p1 == p0 || nm + (size_t)pairs[p1].n <= GEOM_MATCHES))
      nm += (size_t)pairs[p1++].n;
    const int np = (int)(p1 - p0);
    size_t nwork = 0;
    for (size_t p = p0; p < p1; p++) nwork += pairs[p].n >= K ? (size_t)nblk : 0;
    hplan.assign((size_t)np * sizeof(GeomJob) + nwork * sizeof(int2), 0);
    hmatch.resize(nm * 2);
    GeomJob* const jobs = reinterpret_cast<GeomJob*>(hplan.data());
    int2* const work = reinterpret_cast<int2*>(hplan.data() + (size_t)np * sizeof(GeomJob));
    size_t moff = 0, boff = 0;
    for (int q = 0; q < np; q++) {
      const GeomPair& G = pairs[p0 + q];
      GeomJob& J = jobs[q];
      J.l1 = G.l1;
      J.l2 = G.l2;
      J.moff = (int)moff;
      J.n = G.n;
      J.seed = G.seed;
      J.boff = (int)boff;
      J.nblk = G.n >= K ? nblk : 0;
      if (G.n) memcpy(&hmatch[moff * 2], G.matches, (size_t)G.n * 2 * sizeof(int));
      for (int b = 0; b < J.nblk; b++) work[boff + b] = make_int2(q, b);
      moff += (size_t)G.n;
      boff += (size_t)J.nblk;
    }
    M_TRY(&v, g->plan.grow(hplan.size()));
    M_TRY(&v, g->matches.grow(std::max<size_t>(nm, 1)));
    M_TRY(&v, g->best.grow(std::max<size_t>(nwork, 1)));
    M_TRY(&v, g->results.grow((size_t)np));
    M_TRY(&v, g->mask.grow(std::max<size_t>(nm, 1)));
    if (P.refit > 0) M_TRY(&v, g->cand.grow(std::max<size_t>(nm, 1)));
    M_TRY(&v, hipMemcpyAsync(g->plan.p, hplan.data(), hplan.size(), hipMemcpyHostToDevice, v.st));
    if (nm) M_TRY(&v, hipMemcpyAsync(g->matches.p, hmatch.data(), nm * 2 * sizeof(int), hipMemcpyHostToDevice, v.st));
    (void)hipEventRecord(v.e0, v.st);
    const GeomBuffers B{g->plan.p, g->matches.p, g->best.p, g->results.p, g->mask.p, g->cand.p};
    M_TRY(&v, P.model == HESS_GEOM_HOMOGRAPHY ? geom_launch<HESS_GEOM_HOMOGRAPHY>(v.st, B, np, nwork, T, P.bound, P.refit)
                                             : geom_launch<HESS_GEOM_FUNDAMENTAL>(v.st, B, np, nwork, T, P.bound, P.refit));
    (void)hipEventRecord(v.e1, v.st);
    hres.resize((size_t)np);
    hmask.resize(std::max<size_t>(nm, 1));
    M_TRY(&v, hipMemcpyAsync(hres.data(), g->results.p, (size_t)np * sizeof(hess_geom_result), hipMemcpyDeviceToHost, v.st));
    if (nm && inlier) M_TRY(&v, hipMemcpyAsync(hmask.data(), g->mask.p, nm, hipMemcpyDeviceToHost, v.st));
    M_TRY(&v, hipStreamSynchronize(v.st));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, v.e0, v.e1);
    total_ms += ms;
    for (int q = 0; q < np; q++) {
      out[p0 + q] = hres[q];
      if (inlier && jobs[q].n) memcpy(inlier + (p0 + q) * pitch, hmask.data() + jobs[q].moff, (size_t)jobs[q].n);
    }
    p0 = p1;
  }
  *v.last_ms = total_ms;
  return 0;
}

}  // namespace

// ---- hess_matcher_int.h: estimates over matches that are on the device already (hess_matcher_verify_pairs) ------------

int hess_geom_params_check(hess_matcher* m, const hess_geom_params* P, const char* what) {
  hess_matcher_view v = hess_matcher_view_of(m);
  return geom_params_check(v, P, what);
}

int hess_geom_reserve(hess_matcher* m, const hess_geom_params& P, int np, int mm) {
  hess_matcher_view v = hess_matcher_view_of(m);
  hess_geom_state* const g = geom_state(v);
  if (!g) { v.err = "verify_pairs: out of memory"; return HESS_ERR_NOMEM; }
  const size_t nblk = (size_t)((P.hypotheses ? P.hypotheses : GEOM_DEFAULT_T) + 255) / 256, nwork = (size_t)np * nblk;
  M_TRY(&v, g->plan.grow((size_t)np * sizeof(GeomJob) + nwork * sizeof(int2)));
  M_TRY(&v, g->best.grow(nwork));
  if (P.refit > 0) M_TRY(&v, g->cand.grow(std::max<size_t>((size_t)np * mm, 1)));
  return 0;
}

hipError_t hess_geom_enqueue(hess_matcher* m, const hess_geom_params& P, const hess_geom_device_pairs& d) {
  const hess_matcher_view v = hess_matcher_view_of(m);
  hess_geom_state* const g = v.geom->get();
  const hipStream_t st = v.st;
  const int K = geom_k(P.model), T = P.hypotheses ? P.hypotheses : GEOM_DEFAULT_T, nblk = (T + 255) / 256;
  const size_t nwork = (size_t)d.np * nblk;
  GeomJob* const djobs = reinterpret_cast<GeomJob*>(g->plan.p);
  int2* const dwork = reinterpret_cast<int2*>(g->plan.p + (size_t)d.np * sizeof(GeomJob));
  hipLaunchKernelGGL(geom_jobs_fill_kernel, dim3((unsigned)((nwork + 255) / 256)), dim3(256), 0, st, d.lalb, d.counts,
                     v.bank_loc, d.np, d.mm, nblk, K, d.seed0, djobs, dwork);
  const GeomBuffers B{g->plan.p, d.matches, g->best.p, d.results, d.mask, g->cand.p};
  return P.model == HESS_GEOM_HOMOGRAPHY ? geom_launch<HESS_GEOM_HOMOGRAPHY>(st, B, d.np, nwork, T, P.bound, P.refit)
                                         : geom_launch<HESS_GEOM_FUNDAMENTAL>(st, B, d.np, nwork, T, P.bound, P.refit);
}

extern "C" {

int hess_geom_sample(uint32_t seed, int t, int k, int n, int* out) {
  if (!out || t < 0 || k < 1 || k > 8 || n < k) return HESS_ERR_ARG;
  int idx[8];
  geom_sample(seed, t, k, n, idx);
  for (int j = 0; j < k; j++) out[j] = idx[j];
  return 0;
}

int hess_matcher_estimate(hess_matcher* m, int nmatch, const int* pairs, const hess_geom_params* params,
                          hess_geom_result* out, unsigned char* inlier) {
  if (!m) return HESS_ERR_ARG;
  hess_matcher_view v = hess_matcher_view_of(m);
  if (const int rc = geom_params_check(v, params, "estimate")) return rc;
  if (!out) { v.err = "estimate: out is NULL"; return HESS_ERR_ARG; }
  if (nmatch < 0 || (nmatch > 0 && !pairs)) { v.err = "estimate: nmatch < 0 or pairs NULL"; return HESS_ERR_ARG; }
  for (int k = 0; k < 2; k++)
    if (v.nloc[k] < 0) {
      v.err = "estimate: slot " + std::to_string(k) + " has no locations (hess_matcher_set_locations after its descriptors)";
      return HESS_ERR_STATE;
    }
  std::vector<GeomPair> one(1);
  one[0] = GeomPair{v.loc[0], v.loc[1], v.nloc[0], v.nloc[1], pairs, nmatch, params->seed};
  if (const int rc = geom_matches_check(v, one, "estimate")) return rc;
  M_TRY(&v, hipSetDevice(v.device));
  return geom_run(v, one, *params, out, inlier, 0);
}

int hess_matcher_estimate_pairs(hess_matcher* m, int npairs, const int* pairs_ab, int max_match, const int* matches,
                                const int* counts, const hess_geom_params* params, hess_geom_result* out,
                                unsigned char* inlier) {
  if (!m) return HESS_ERR_ARG;
  hess_matcher_view v = hess_matcher_view_of(m);
  if (const int rc = geom_params_check(v, params, "estimate_pairs")) return rc;
  if (npairs < 0 || max_match < 0 || (npairs > 0 && (!pairs_ab || !counts || !out))) {
    v.err = "estimate_pairs: npairs or max_match < 0, or pairs_ab, counts or out is NULL";
    return HESS_ERR_ARG;
  }
  if (!v.bank_have_loc) {
    v.err = "estimate_pairs: the bank has no locations (hess_matcher_bank_set_locations after its descriptors)";
    return HESS_ERR_STATE;
  }
  const int nsets = (int)v.bank_num->size();
  std::vector<GeomPair> pairs((size_t)npairs);
  for (int p = 0; p < npairs; p++) {
    const int a = pairs_ab[2 * p], b = pairs_ab[2 * p + 1];
    if (a < 0 || a >= nsets || b < 0 || b >= nsets) {
      v.err = "estimate_pairs: pair " + std::to_string(p) + " names a set outside the bank of " + std::to_string(nsets);
      return HESS_ERR_ARG;
    }
    if (counts[p] < 0 || counts[p] > max_match) {
      v.err = "estimate_pairs: counts[" + std::to_string(p) + "] = " + std::to_string(counts[p]) + " lies outside 0..max_match";
      return HESS_ERR_ARG;
    }
    if (counts[p] > 0 && !matches) { v.err = "estimate_pairs: matches is NULL"; return HESS_ERR_ARG; }
    pairs[p] = GeomPair{v.bank_loc + (*v.bank_first)[a], v.bank_loc + (*v.bank_first)[b], (*v.bank_num)[a], (*v.bank_num)[b],
                        matches ? matches + (size_t)p * max_match * 2 : nullptr, counts[p], params->seed + (uint32_t)p};
  }
  if (const int rc = geom_matches_check(v, pairs, "estimate_pairs")) return rc;
  *v.last_ms = 0.0f;
  if (npairs == 0) return 0;
  M_TRY(&v, hipSetDevice(v.device));
  if (inlier) memset(inlier, 0, (size_t)npairs * max_match);
  return geom_run(v, pairs, *params, out, inlier, (size_t)max_match);
}

}  // extern "C"
