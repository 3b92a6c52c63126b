// guided_gate_main.cpp -- the guided gate (hessgpu_amd/csrc/hess_guided_gate.h) on the CPU, the way match_mfma_kernel<GUIDED>
// uses it: the row terms of every location of set 1 and the column terms of every location of set 2 are computed once, then
// every (i, j) is decided from them.  Built with -fsanitize=address,undefined by tests/test_guided_gate_cpu.py.
//
// stdin, per case (floats in C99 hexadecimal notation, exact): "case n1 n2", H[9], F[9], hdistmax, fdistmax, n1 (x, y), n2 (x, y).
// stdout, per case: "case n1 n2", then n1 lines of n2 characters '1' (passes) or '0'; at the end "GATE OK <cases>".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hess_guided_gate.h"

static bool read_float(float* out) {
  char tok[64];
  if (scanf("%63s", tok) != 1) return false;
  char* end = nullptr;
  *out = (float)strtod(tok, &end);
  return end && *end == 0;
}

int main() {
  int cases = 0, n1 = 0, n2 = 0;
  char word[16];
  while (scanf("%15s %d %d", word, &n1, &n2) == 3) {
    if (std::string(word) != "case" || n1 < 0 || n2 < 0) return 2;
    float H[9], F[9], hd = 0, fd = 0;
    for (float& v : H) if (!read_float(&v)) return 3;
    for (float& v : F) if (!read_float(&v)) return 3;
    if (!read_float(&hd) || !read_float(&fd)) return 3;
    std::vector<hess::GuidedRow> rows((size_t)n1);
    std::vector<hess::GuidedCol> cols((size_t)n2);
    for (int i = 0; i < n1; i++) {
      float x, y;
      if (!read_float(&x) || !read_float(&y)) return 4;
      hess::guided_row_h(H, x, y, rows[i]);
      hess::guided_row_f(F, x, y, rows[i]);
    }
    for (int j = 0; j < n2; j++) {
      float x, y;
      if (!read_float(&x) || !read_float(&y)) return 4;
      cols[j] = hess::guided_col(F, x, y);
    }
    printf("case %d %d\n", n1, n2);
    std::string line((size_t)n2, '0');
    for (int i = 0; i < n1; i++) {
      for (int j = 0; j < n2; j++) {
        const bool whole = hess::guided_pass(rows[i], cols[j], hd, fd);
        const bool parts = hess::guided_box(rows[i], cols[j].x, cols[j].y, hd) && hess::guided_sampson(rows[i], cols[j], fd);
        if (whole != parts) return 5;
        line[j] = whole ? '1' : '0';
      }
      puts(line.c_str());
    }
    cases++;
  }
  printf("GATE OK %d\n", cases);
  return 0;
}
