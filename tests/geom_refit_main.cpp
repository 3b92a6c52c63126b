// geom_refit_main.cpp -- runs the serial arithmetic of the estimator's refit (hessgpu_amd/csrc/hess_geom_refit.h) on the host for
// the cases on stdin and prints what it makes of them.  Built with -fsanitize=address,undefined and run by
// tests/test_geom_refit_cpu.py, which computes the sums in float64 and compares the output with numpy.  Exit status 0 = every case
// was read and run.
//
// stdin, one case per line, tokens separated by white space (doubles as %.17g):
//   MODEL(1 H, 2 F)  CNT  SD1 SD2  C1X C1Y C2X C2Y  PREV[9]  SUMS[24 or 36]  BEFORE CANDIDATE DIFFER
//     CNT inliers, the distance sums, the centroids, the matrix before, the moment sums in the header's layout, and three counts
//     for the decision
// stdout, per case:
//   case STOP(0, or 1: the scales say stop)  SWEEPS  FINITE  DECISION  X[9] (the eigenvector)  C[9] (the candidate, float32)  N[81]
//   and at the end: REFIT OK <cases>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hess_geom_refit.h"

static bool next(double& v) { return scanf("%lf", &v) == 1; }

int main() {
  int cases = 0;
  double first;
  while (next(first)) {
    const int model = (int)first;
    if (model != GEOM_MODEL_H && model != GEOM_MODEL_F) { fprintf(stderr, "case %d: model %d\n", cases, model); return 1; }
    double in[6 + 9], cnt;
    if (!next(cnt)) return 1;
    for (double& v : in)
      if (!next(v)) return 1;
    const int ns = geom_refit_sums(model);
    std::vector<double> sums((size_t)ns);  // (exactly: the sanitizer sees a read past it)
    for (double& v : sums)
      if (!next(v)) return 1;
    double dec[3];
    for (double& v : dec)
      if (!next(v)) return 1;
    GeomRefitNorm nm;
    nm.c1x = in[2]; nm.c1y = in[3]; nm.c2x = in[4]; nm.c2y = in[5];
    nm.s1 = nm.s2 = 0.0;
    const bool go = geom_refit_scales((int)cnt, in[0], in[1], nm.s1, nm.s2);
    float prev[9], C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 9; i++) prev[i] = (float)in[6 + i];
    std::vector<double> N(81), A(81), V(81);
    double x[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int sweeps = 0, finite = 0;
    if (go) {
      geom_refit_normal(model, sums.data(), N.data());
      A = N;
      sweeps = geom_refit_eigen(A.data(), V.data(), x);
      finite = geom_refit_candidate(model, x, nm, prev, C) ? 1 : 0;
    }
    printf("case %d %d %d %d", go ? 0 : 1, sweeps, finite, geom_refit_decide((int)dec[0], (int)dec[1], (int)dec[2]));
    for (int i = 0; i < 9; i++) printf(" %.17g", x[i]);
    for (int i = 0; i < 9; i++) printf(" %.9g", (double)C[i]);
    for (int i = 0; i < 81; i++) printf(" %.17g", N[i]);
    printf("\n");
    cases++;
  }
  printf("REFIT OK %d\n", cases);
  return 0;
}
