// match_plan_main.cpp -- prints the matcher's plan (hessgpu_amd/csrc/hess_match_plan.h) for the cases on stdin and checks what the
// kernels rely on in every one of them.  Built with -fsanitize=address,undefined and run by tests/test_match_plan_cpu.py, which
// compares the printed plans with the restatement in tests/matcher_cases.py.  Exit status 0 = every condition held.
//
// stdin, tokens separated by white space:
//   single N1 N2 MUTUAL                              the untyped single pair on the matrix cores (single_sps)
//   list TYPED NSETS NPAIRS MAX_MATCH MUTUAL  rows of each set (TYPED: of its four class groups)  A B of each pair
// stdout:
//   single N1 N2 NRB NSUPER NSEG SPS
//   plan STATUS JPP MM RS CP RM CM PLAN_BYTES OUTN NCHUNKS     (STATUS 0, or -1 = too big and nothing else follows)
//   chunk FIRST_PAIR END_PAIR SPS RS CP RM CM NWG NFIN         per chunk
//   job INDEX N1 N2 NRB NSUPER NSEG SPS RS CP RM CM            per job
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hess_match_plan.h"

using namespace hess::match_plan;

static int g_case = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      fprintf(stderr, "case %d, line %d: %s does not hold\n", g_case, __LINE__, #cond);    \
      exit(1);                                                                             \
    }                                                                                      \
  } while (0)

// One planned chunk: its jobs, its totals, and the plan buffer plan_fill makes of it.
static void check_chunk(const PairJob* jobs, const Entry* orig, const Chunk& c, int mutual) {
  const int np = c.p1 - c.p0;
  const PlanLayout L = plan_layout(c);
  CHECK(L.jobs == 0 && L.work == (size_t)np * sizeof(PairJob) && L.fin == L.work + c.nwg * 8 && L.orig == L.fin + c.nfin * 8);
  CHECK(L.bytes == L.orig + (c.jpp == 4 ? (size_t)c.pairs() * 8 : 0));
  CHECK(L.work % 8 == 0 && L.fin % 8 == 0 && L.orig % 8 == 0);
  CHECK(c.sps >= 1 && 4 * c.sps <= MM_MAX_TILES);
  std::vector<unsigned char> buf(L.bytes);  // (exactly: the sanitizer sees a write past it)
  plan_fill(buf.data(), jobs, orig, c, mutual);
  CHECK(!memcmp(buf.data(), jobs + c.p0, (size_t)np * sizeof(PairJob)));
  if (L.bytes > L.orig) CHECK(!memcmp(buf.data() + L.orig, orig + c.p0 / c.jpp, L.bytes - L.orig));
  const Entry* work = plan_ptr<Entry>(buf.data(), L.work);
  const Entry* fin = plan_ptr<Entry>(buf.data(), L.fin);
  size_t rs = 0, cp = 0, rm = 0, cm = 0, iw = 0, jf = 0;
  for (int q = 0; q < np; q++) {
    const PairJob& J = jobs[c.p0 + q];
    if (!J.n1) { CHECK(J.n2 == 0); continue; }
    CHECK(J.n1 > 0 && J.n2 > 0);
    CHECK(J.nrb == (J.n1 + MM_ROWS - 1) / MM_ROWS && J.nsuper == (J.n2 + MM_SUPER - 1) / MM_SUPER);
    CHECK(J.sps >= 1 && J.sps <= c.sps && 4 * J.sps <= MM_MAX_TILES);
    CHECK(J.nseg >= 1 && (long long)(J.nseg - 1) * J.sps < J.nsuper && (long long)J.nseg * J.sps >= J.nsuper);
    CHECK(J.nrb - 1 <= 0xffff && J.nseg - 1 <= 0x7fff);
    CHECK((size_t)J.rs == rs && (size_t)J.cp == cp && (size_t)J.rm == rm && (size_t)J.cm == cm);  // running sums
    rs += (size_t)J.n1 * J.nseg;
    cp += mutual ? (size_t)J.nrb * J.n2 : 0;
    rm += (size_t)J.n1;
    cm += mutual ? (size_t)J.n2 : 0;
    CHECK(rs <= c.rs && cp <= c.cp && rm <= c.rm && cm <= c.cm);
    // every (row block, segment) exactly once, in this job's stretch of the multiply table
    std::vector<char> seen((size_t)J.nrb * J.nseg, 0);
    for (size_t k = 0; k < seen.size(); k++, iw++) {
      CHECK(iw < c.nwg && work[iw].x == q);
      const int rb = work[iw].y & 0xffff, sg = work[iw].y >> 16;
      CHECK(work[iw].y >= 0 && rb < J.nrb && sg < J.nseg && !seen[(size_t)sg * J.nrb + rb]);
      seen[(size_t)sg * J.nrb + rb] = 1;
    }
    const int nfb = (J.n1 + 255) / 256 + (mutual ? (J.n2 + 31) / 32 : 0);
    for (int b = 0; b < nfb; b++, jf++) CHECK(jf < c.nfin && fin[jf].x == q && fin[jf].y == b);
  }
  CHECK(iw == c.nwg && jf == c.nfin && rs == c.rs && cp == c.cp && rm == c.rm && cm == c.cm);
  CHECK(c.rs + c.cp <= (size_t)INT32_MAX && c.nwg <= (size_t)INT32_MAX);
}

static void print_job(int idx, const PairJob& J) {
  printf("job %d %d %d %d %d %d %d %d %d %d %d\n", idx, J.n1, J.n2, J.nrb, J.nsuper, J.nseg, J.sps, J.rs, J.cp, J.rm, J.cm);
}

static int read_int() {
  int v = 0;
  if (scanf("%d", &v) != 1) { fprintf(stderr, "case %d: a number is missing\n", g_case); exit(2); }
  return v;
}

static void single_case() {
  const int n1 = read_int(), n2 = read_int(), mutual = read_int();
  PairJob job{};
  job.n1 = n1;
  job.n2 = n2;
  Chunk c{0, 1, single_sps(n1, n2), 0, 0, 0, 0, 0, 0, 1};
  plan_chunk(&job, c, mutual);
  check_chunk(&job, nullptr, c, mutual);
  printf("single %d %d %d %d %d %d\n", n1, n2, job.nrb, job.nsuper, job.nseg, job.sps);
}

static void list_case() {
  const int typed = read_int(), nsets = read_int(), npairs = read_int(), max_match = read_int(), mutual = read_int();
  CHECK(nsets > 0 && npairs > 0);
  std::vector<int> counts((size_t)nsets), gnum, goff, off((size_t)nsets), num((size_t)nsets), first((size_t)nsets), src((size_t)nsets);
  if (typed) {
    gnum.resize((size_t)nsets * 4);
    goff.resize((size_t)nsets * 4);
    for (int k = 0; k < nsets; k++) {
      counts[k] = 0;
      for (int c = 0; c < 4; c++) counts[k] += gnum[4 * k + c] = read_int();
    }
  } else {
    for (int k = 0; k < nsets; k++) counts[k] = read_int();
  }
  size_t padded = 0, gpadded = 0;
  CHECK(set_layout(nsets, counts.data(), INT_MAX, 128, off.data(), num.data(), first.data(), src.data(), &padded));
  for (int k = 0; k < nsets; k++) {
    CHECK(off[k] % MM_ROWS == 0 && num[k] == counts[k] && (k == 0 || (size_t)off[k] == off[k - 1] + pad_rows((size_t)num[k - 1])));
    CHECK(first[k] == src[k] && (k == 0 || first[k] == first[k - 1] + num[k - 1]));
  }
  if (typed) {
    CHECK(group_layout(4 * nsets, gnum.data(), 128, goff.data(), &gpadded));
    for (int g = 0; g < 4 * nsets; g++) CHECK(g == 0 ? goff[0] == 0 : (size_t)goff[g] == goff[g - 1] + pad_rows((size_t)gnum[g - 1]));
  }
  std::vector<int> ab((size_t)npairs * 2);
  for (int& v : ab) { v = read_int(); CHECK(v >= 0 && v < nsets); }
  const SetsLayout S{off.data(), num.data(), first.data(), typed ? goff.data() : nullptr, typed ? gnum.data() : nullptr};
  PairPlan P;
  if (!plan_pairs(S, S, npairs, ab.data(), max_match, mutual, P)) {
    printf("plan -1\n");
    return;
  }
  const int jpp = typed ? 4 : 1;
  CHECK(P.jpp == jpp && P.jobs.size() == (size_t)npairs * jpp && P.orig.size() == (typed ? (size_t)npairs : 0) && !P.chunks.empty());
  int mm = 0;
  for (int p = 0; p < npairs; p++) {
    const int n1 = num[ab[2 * p + 1]] ? num[ab[2 * p]] : 0;
    mm = n1 < max_match ? (n1 > mm ? n1 : mm) : (max_match > mm ? max_match : mm);
    if (typed) CHECK(P.orig[p].x == first[ab[2 * p]] && P.orig[p].y == num[ab[2 * p]]);
  }
  CHECK(P.mm == mm);
  printf("plan 0 %d %d %zu %zu %zu %zu %zu %zu %zu\n", P.jpp, P.mm, P.need.rs, P.need.cp, P.need.rm, P.need.cm, P.need.plan_bytes,
         P.need.outn, P.chunks.size());
  int next = 0;
  for (const Chunk& c : P.chunks) {  // the chunks partition the list in order
    CHECK(c.jpp == jpp && c.p0 == next && c.p1 > c.p0 && (c.p1 - c.p0) % jpp == 0 && c.pairs() <= MP_PAIRS);
    next = c.p1;
    const size_t scratch = 12 * (c.rs + c.cp) + 4 * (c.rm + c.cm);
    CHECK(scratch <= MP_SCRATCH || c.pairs() == 1);
    check_chunk(P.jobs.data(), P.orig.data(), c, mutual);
    CHECK(P.need.rs >= c.rs && P.need.cp >= c.cp && P.need.rm >= c.rm && P.need.cm >= c.cm && P.need.plan_bytes >= plan_layout(c).bytes &&
          P.need.outn >= (size_t)MP_PAIRS + (size_t)c.pairs() * P.mm * 2);
    CHECK(P.need.rs >= 1 && P.need.cp >= 1 && P.need.rm >= 1 && P.need.cm >= 1);
    printf("chunk %d %d %d %zu %zu %zu %zu %zu %zu\n", c.p0 / jpp, c.p1 / jpp, c.sps, c.rs, c.cp, c.rm, c.cm, c.nwg, c.nfin);
  }
  CHECK(next == npairs * jpp);
  for (size_t k = 0; k < P.jobs.size(); k++) print_job((int)k, P.jobs[k]);
}

int main() {
  char word[16];
  while (scanf("%15s", word) == 1) {
    g_case++;
    if (!strcmp(word, "single")) single_case();
    else if (!strcmp(word, "list")) list_case();
    else { fprintf(stderr, "case %d: unknown kind '%s'\n", g_case, word); return 2; }
  }
  printf("PLAN OK %d\n", g_case);
  return 0;
}
