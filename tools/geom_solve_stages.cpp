// geom_solve_stages.cpp -- geom_hypothesis of hessgpu_amd/csrc/hess_geom.hip on the host, operation for operation (same
// order, an fma where the kernel has one; compile without contraction), with the precision of each of its three stages
// selectable: normalisation, elimination, denormalisation.  tools/geom_solve_stages.py drives it and compares the result
// with the float64 solve of tests/geom_cases.py (profiles/r18_estimate_tests.txt, section 1).  Host code only.
//
//   geom_solve_stages <H|F> <nnn> <variant>  < samples     nnn: f or d for each stage, e.g. fdf = the kernel as built
//   variant 0: Gauss-Jordan as in the kernel; 1: the factor as a quotient, not a product with the reciprocal;
//           2: Gaussian elimination on the unused rows only, then back substitution in pivot order
//   stdin: per sample k x (x1 y1 x2 y2), k = 4 (H) or 8 (F); stdout: the nine entries before geom_finalise, as float32.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

template <class R>
void null_vector(R (&a)[8][9], R (&x)[9], int variant) {
  unsigned rused = 0, cused = 0;
  int pcol[8] = {0}, prs[8], pcs[8];
  for (int step = 0; step < 8; step++) {
    R best = -1;
    int pr = 0, pc = 0;
    for (int r = 0; r < 8; r++) {
      const bool rfree = !((rused >> r) & 1u);
      for (int c = 0; c < 9; c++) {
        const R v = std::fabs(a[r][c]);
        const bool take = rfree && !((cused >> c) & 1u) && v > best;
        best = take ? v : best;
        pr = take ? r : pr;
        pc = take ? c : pc;
      }
    }
    rused |= 1u << pr;
    cused |= 1u << pc;
    prs[step] = pr;
    pcs[step] = pc;
    pcol[pr] = pc;
    R prow[9];
    for (int c = 0; c < 9; c++) prow[c] = a[pr][c];
    const R piv = prow[pc], inv = R(1) / piv;
    for (int r = 0; r < 8; r++) {
      const bool skip = variant == 2 ? ((rused >> r) & 1u) != 0 : pr == r;
      const R f = skip ? R(0) : (variant == 1 ? a[r][pc] / piv : a[r][pc] * inv);
      for (int c = 0; c < 9; c++) a[r][c] = std::fma(-f, prow[c], a[r][c]);
    }
  }
  int fc = 0;
  for (int c = 0; c < 9; c++) fc = ((cused >> c) & 1u) ? fc : c;
  for (int c = 0; c < 9; c++) x[c] = fc == c ? R(1) : R(0);
  if (variant == 2) {
    for (int step = 7; step >= 0; step--) {
      R s = 0;
      for (int c = 0; c < 9; c++) s = std::fma(c == pcs[step] ? R(0) : a[prs[step]][c], x[c], s);
      x[pcs[step]] = -s / a[prs[step]][pcs[step]];
    }
  } else {
    for (int r = 0; r < 8; r++) x[pcol[r]] = -a[r][fc] / a[r][pcol[r]];
  }
}

template <class R, int K>
void normalise(R (&x)[K], R (&y)[K], R& cx, R& cy, R& s) {
  R sx = 0, sy = 0;
  for (int i = 0; i < K; i++) {
    sx += x[i];
    sy += y[i];
  }
  cx = sx * R(1.0f / K);
  cy = sy * R(1.0f / K);
  R d = 0;
  for (int i = 0; i < K; i++) {
    x[i] -= cx;
    y[i] -= cy;
    d += std::sqrt(std::fma(x[i], x[i], y[i] * y[i]));
  }
  s = R(1.41421356237f) * K / d;
  for (int i = 0; i < K; i++) {
    x[i] *= s;
    y[i] *= s;
  }
}

// RN, RE, RD: the types of normalisation, elimination and denormalisation.  K = 4: H, K = 8: F.
template <int K, class RN, class RE, class RD>
void hypothesis(const float* in, int variant, double* M) {
  RN x1[K], y1[K], x2[K], y2[K], c1x, c1y, s1, c2x, c2y, s2;
  for (int i = 0; i < K; i++) {
    x1[i] = in[4 * i];
    y1[i] = in[4 * i + 1];
    x2[i] = in[4 * i + 2];
    y2[i] = in[4 * i + 3];
  }
  normalise<RN, K>(x1, y1, c1x, c1y, s1);
  normalise<RN, K>(x2, y2, c2x, c2y, s2);
  RE a[8][9];
  for (int i = 0; i < K; i++) {
    const RE x = (RE)x1[i], y = (RE)y1[i], u = (RE)x2[i], v = (RE)y2[i];
    if (K == 4) {
      const RE r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, -u}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, -v};
      memcpy(a[(2 * i) & 7], r0, sizeof(r0));
      memcpy(a[(2 * i + 1) & 7], r1, sizeof(r1));
    } else {
      const RE r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1};
      memcpy(a[i & 7], r, sizeof(r));
    }
  }
  RE he[9];
  null_vector(a, he, variant);
  RD h[9], G[9];
  const RD S1 = (RD)s1, S2 = (RD)s2, C1x = (RD)c1x, C1y = (RD)c1y, C2x = (RD)c2x, C2y = (RD)c2y;
  for (int c = 0; c < 9; c++) h[c] = (RD)he[c];
  for (int r = 0; r < 3; r++) {
    G[3 * r] = h[3 * r] * S1;
    G[3 * r + 1] = h[3 * r + 1] * S1;
    G[3 * r + 2] = h[3 * r + 2] - S1 * std::fma(h[3 * r], C1x, h[3 * r + 1] * C1y);
  }
  for (int c = 0; c < 3; c++) {
    if (K == 4) {
      M[c] = std::fma(C2x, G[6 + c], G[c] / S2);
      M[3 + c] = std::fma(C2y, G[6 + c], G[3 + c] / S2);
      M[6 + c] = G[6 + c];
    } else {
      M[c] = S2 * G[c];
      M[3 + c] = S2 * G[3 + c];
      M[6 + c] = G[6 + c] - S2 * std::fma(C2x, G[c], C2y * G[3 + c]);
    }
  }
}

template <int K>
void run(int key, const float* in, int variant, double* M) {
  switch (key) {
    case 0: hypothesis<K, float, float, float>(in, variant, M); break;
    case 1: hypothesis<K, float, float, double>(in, variant, M); break;
    case 2: hypothesis<K, float, double, float>(in, variant, M); break;
    case 3: hypothesis<K, float, double, double>(in, variant, M); break;
    case 4: hypothesis<K, double, float, float>(in, variant, M); break;
    case 5: hypothesis<K, double, float, double>(in, variant, M); break;
    case 6: hypothesis<K, double, double, float>(in, variant, M); break;
    default: hypothesis<K, double, double, double>(in, variant, M); break;
  }
}

int main(int argc, char** argv) {
  if (argc < 3 || strlen(argv[2]) != 3) {
    fprintf(stderr, "usage: geom_solve_stages <H|F> <fff..ddd> [variant] < samples\n");
    return 2;
  }
  const bool isF = argv[1][0] == 'F';
  const char* cfg = argv[2];
  const int variant = argc > 3 ? atoi(argv[3]) : 0, count = isF ? 32 : 16;
  const int key = (cfg[0] == 'd') * 4 + (cfg[1] == 'd') * 2 + (cfg[2] == 'd');
  float in[32];
  for (;;) {
    for (int i = 0; i < count; i++)
      if (scanf("%f", &in[i]) != 1) return 0;
    double M[9];
    if (isF) run<8>(key, in, variant, M);
    else run<4>(key, in, variant, M);
    for (int c = 0; c < 9; c++) printf("%.9g ", (double)(float)M[c]);
    printf("\n");
  }
}
