// hess_match_plan.cpp -- the matcher's plan (hess_match_plan.h): host arithmetic on sizes, standard headers only.
#include "hess_match_plan.h"

#include <algorithm>
#include <cstring>

namespace hess::match_plan {

bool set_layout(int nsets, const int* counts, int max_sift, size_t KD, int* off, int* num, int* first, int* src, size_t* padded) {
  size_t pad = 0, srow = 0, orow = 0;
  for (int k = 0; k < nsets; k++) {
    const int n = counts[k] > max_sift ? max_sift : counts[k];
    off[k] = (int)pad;
    num[k] = n;
    first[k] = (int)orow;
    src[k] = (int)srow;
    orow += (size_t)n;
    pad += pad_rows((size_t)n);
    srow += (size_t)counts[k];
    if (pad > (size_t)INT32_MAX / KD || srow > (size_t)INT32_MAX) return false;
  }
  *padded = pad;
  return true;
}

bool group_layout(int ngroups, const int* gnum, size_t KD, int* goff, size_t* padded) {
  size_t pad = 0;
  for (int g = 0; g < ngroups; g++) {
    goff[g] = (int)pad;
    pad += pad_rows((size_t)gnum[g]);
    if (pad > (size_t)INT32_MAX / KD) return false;
  }
  *padded = pad;
  return true;
}

// Super tiles per segment at most for the single pair of hess_matcher_match on the matrix cores, one job: (256-row block,
// column segment) workgroups, at least two per CU where the problem allows.  Workgroups: whole rounds over the 256 CUs --
// two per CU (what the registers allow) when that leaves a workgroup at least four super tiles, else one per CU with twice
// the tiles (its prologue and the merge of the row states at its end cost about as much as two super tiles).  Same call,
// 4096^2 / 8192^2, TMAC/s: 256 workgroups 91 / 193, 384: 91 / 176, 512: 81 / 211, 768: 81 / 180
// (profiles/r06_experiments/matcher.txt).
int single_sps(int n1, int n2) {
  const int nrb = (n1 + MM_ROWS - 1) / MM_ROWS, nsuper = (n2 + MM_SUPER - 1) / MM_SUPER;
  const int target_wgs = (long long)nrb * nsuper >= 512 * 4 ? 512 : 256;
  int nseg = (target_wgs + nrb - 1) / nrb;
  nseg = nseg < 1 ? 1 : (nseg > nsuper ? nsuper : nseg);
  return std::min((nsuper + nseg - 1) / nseg, MM_MAX_SPS);
}

// Super tiles per segment at most for `work` (256-row block, super tile) units in one launch of a pair list: whole rounds of
// workgroups over the 256 CUs as in single_sps (two per CU when that leaves each at least four super tiles:
// profiles/r06_experiments/matcher.txt).  Not single_sps of a list of one: that one balances the segments over the row
// blocks of its pair, this one the work of the chunk, and they part in one shape of nine.
static int chunk_sps(size_t work) {
  const size_t target = work >= 512 * 4 ? 512 : 256;
  const size_t sps = (work + target - 1) / target;
  return sps < 1 ? 1 : (sps > (size_t)MM_MAX_SPS ? MM_MAX_SPS : (int)sps);
}

// Segments of a pair of nsuper super tiles: at most sps super tiles each (the tile index shares six key bits, so
// sps <= MM_MAX_SPS), as many as that needs, balanced: psps <= sps.
static void pair_seg(int nsuper, int sps, int& nseg, int& psps) {
  nseg = (nsuper + sps - 1) / sps;
  psps = (nsuper + nseg - 1) / nseg;
  nseg = (nsuper + psps - 1) / psps;
}

static size_t job_work(const PairJob& J) {
  return J.n1 ? (size_t)((J.n1 + MM_ROWS - 1) / MM_ROWS) * ((J.n2 + MM_SUPER - 1) / MM_SUPER) : 0;
}

// The jobs of the pair s1[sa] x s2[sb]: one, or for typed sets one per class; n1 = n2 = 0: no work.
static void pair_jobs(const SetsLayout& s1, int sa, const SetsLayout& s2, int sb, PairJob* J) {
  const bool typed = s1.goff && s2.goff;
  for (int c = 0; c < (typed ? 4 : 1); c++) {
    J[c] = PairJob{};
    J[c].a = typed ? s1.goff[4 * sa + c] : s1.off[sa];
    J[c].b = typed ? s2.goff[4 * sb + c] : s2.off[sb];
    J[c].n1 = typed ? s1.gnum[4 * sa + c] : s1.num[sa];
    J[c].n2 = typed ? s2.gnum[4 * sb + c] : s2.num[sb];
    if (J[c].n1 == 0 || J[c].n2 == 0) J[c].n1 = J[c].n2 = 0;  // an empty side: no work and no matches
  }
}

// Blocks of a job in the finish table: its rows 256 at a time, then for mutual best its columns 32 at a time.
static int job_fin(const PairJob& J, int mutual_best) { return (J.n1 + 255) / 256 + (mutual_best ? (J.n2 + 31) / 32 : 0); }

size_t plan_chunk(PairJob* jobs, Chunk& c, int mutual_best) {
  c.rs = c.cp = c.rm = c.cm = c.nwg = c.nfin = 0;
  for (int p = c.p0; p < c.p1; p++) {
    PairJob& J = jobs[p];
    if (!J.n1) continue;
    J.nrb = (J.n1 + MM_ROWS - 1) / MM_ROWS;
    J.nsuper = (J.n2 + MM_SUPER - 1) / MM_SUPER;
    pair_seg(J.nsuper, c.sps, J.nseg, J.sps);
    J.rs = (int)c.rs; J.cp = (int)c.cp; J.rm = (int)c.rm; J.cm = (int)c.cm;
    c.rs += (size_t)J.n1 * J.nseg;
    c.cp += mutual_best ? (size_t)J.nrb * J.n2 : 0;
    c.rm += J.n1;
    c.cm += mutual_best ? J.n2 : 0;
    c.nwg += (size_t)J.nrb * J.nseg;
    c.nfin += job_fin(J, mutual_best);
  }
  return 3 * sizeof(int) * (c.rs + c.cp) + sizeof(int) * (c.rm + c.cm);
}

PlanLayout plan_layout(const Chunk& c) {
  const size_t work = (size_t)(c.p1 - c.p0) * sizeof(PairJob), fin = work + c.nwg * sizeof(Entry), orig = fin + c.nfin * sizeof(Entry);
  return PlanLayout{0, work, fin, orig, orig + (c.jpp == 4 ? (size_t)c.pairs() : 0) * sizeof(Entry)};
}

void plan_fill(unsigned char* hp, const PairJob* jobs, const Entry* orig, const Chunk& c, int mutual_best) {
  const PlanLayout L = plan_layout(c);
  const int np = c.p1 - c.p0;
  memcpy(hp + L.jobs, jobs + c.p0, np * sizeof(PairJob));
  Entry* const work = reinterpret_cast<Entry*>(hp + L.work);
  Entry* const fin = reinterpret_cast<Entry*>(hp + L.fin);
  size_t iw = 0, jf = 0;
  for (int q = 0; q < np; q++) {
    const PairJob& J = jobs[c.p0 + q];
    if (!J.n1) continue;
    for (int sg = 0; sg < J.nseg; sg++)
      for (int rb = 0; rb < J.nrb; rb++) work[iw++] = Entry{q, rb | sg << 16};
    const int nfb = job_fin(J, mutual_best);
    for (int b = 0; b < nfb; b++) fin[jf++] = Entry{q, b};
  }
  if (L.bytes > L.orig) memcpy(hp + L.orig, orig + c.p0 / c.jpp, L.bytes - L.orig);
}

bool plan_pairs(const SetsLayout& s1, const SetsLayout& s2, int npairs, const int* pairs_ab, int max_match, int mutual_best,
                PairPlan& P) {
  const bool typed = s1.goff && s2.goff;
  const int jpp = P.jpp = typed ? 4 : 1;
  P.jobs.resize((size_t)npairs * jpp);
  P.orig.resize(typed ? (size_t)npairs : 0);
  for (int p = 0; p < npairs; p++) {
    const int sa = pairs_ab[2 * p], sb = pairs_ab[2 * p + 1];
    pair_jobs(s1, sa, s2, sb, &P.jobs[(size_t)p * jpp]);
    if (typed) P.orig[p] = Entry{s1.first[sa], s1.num[sa]};
    P.mm = std::max(P.mm, std::min(s2.num[sb] ? s1.num[sa] : 0, max_match));
  }
  // Segments per pair from the whole chunk's grid: chunk_sps of the chunk's work as it grows.
  for (int p0 = 0; p0 < npairs;) {  // (p0 and `pairs` count pairs, the chunk's p0 and p1 jobs)
    Chunk c{p0 * jpp, p0 * jpp, 1, 0, 0, 0, 0, 0, 0, jpp};
    size_t work = 0;
    int pairs = 0;
    while (p0 + pairs < npairs && pairs < MP_PAIRS) {
      size_t w = 0;
      for (int k = 0; k < jpp; k++) w += job_work(P.jobs[c.p1 + k]);
      Chunk t = c;
      t.p1 += jpp;
      t.sps = chunk_sps(work + w);
      if (pairs > 0 && plan_chunk(P.jobs.data(), t, mutual_best) > MP_SCRATCH) break;
      c = t;
      work += w;
      pairs++;
    }
    plan_chunk(P.jobs.data(), c, mutual_best);  // (the plan of the chunk as it ends)
    if (c.rs + c.cp > (size_t)INT32_MAX || c.nwg > (size_t)INT32_MAX) return false;
    P.chunks.push_back(c);
    p0 += pairs;
    PlanNeed& N = P.need;
    N.rs = std::max(N.rs, c.rs); N.cp = std::max(N.cp, c.cp); N.rm = std::max(N.rm, c.rm); N.cm = std::max(N.cm, c.cm);
    N.plan_bytes = std::max(N.plan_bytes, plan_layout(c).bytes);
    N.outn = std::max(N.outn, (size_t)MP_PAIRS + (size_t)c.pairs() * P.mm * 2);
  }
  return true;
}

}  // namespace hess::match_plan
