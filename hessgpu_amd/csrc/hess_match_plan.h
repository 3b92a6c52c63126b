// hess_match_plan.h -- the matcher's plan: everything hess_match.hip decides by arithmetic on sizes, without HIP (standard
// headers only, like hess_stager.h), so that tests/match_plan_main.cpp can run it on the CPU.
//   how descriptor sets are laid out in padded 256-row blocks (set_layout, group_layout);
//   how a pair is cut into row blocks, super tiles and segments (single_sps, chunk_sps, pair_seg, plan_chunk);
//   how a pair list becomes jobs and chunks and what the buffers must hold for it (plan_pairs);
//   where jobs, the two work tables and the `orig` table sit in the plan buffer (plan_layout, plan_fill, plan_ptr).
#ifndef HESS_MATCH_PLAN_H
#define HESS_MATCH_PLAN_H
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hess::match_plan {

constexpr int MM_ROWS = 256;       // rows of set 1 per workgroup (64 per wavefront)
constexpr int MM_SUPER = 128;      // columns per super tile
constexpr int MM_MAX_TILES = 60;   // tiles per segment: the tile index shares 6 key bits with "none"
constexpr int MM_MAX_SPS = MM_MAX_TILES / 4;  // super tiles per segment
// hess_matcher_match: n1 * n2 above it runs on the matrix cores; small problems (three launches of latency) stay on the
// one-pass dot kernel: 1024 x 1024 0.026 vs 0.033 ms
constexpr size_t MM_SINGLE_ABOVE = (size_t)3 << 20;
// Pairs of one match_pairs chunk, and the device scratch one chunk may use (row states n1 x nseg and, for mutual best,
// column partials nrb x n2 per pair, then row and column decisions).  A pair whose scratch alone exceeds the budget is
// a chunk of its own.
constexpr int MP_PAIRS = 64;
constexpr size_t MP_SCRATCH = (size_t)256 << 20;

// One pair of a launch.  a, b: first row of set 1 in the rows (and rfix) passed as set 1, of set 2 in those passed as set 2
// -- the bank twice for a bank pair, the two single-pair slots (a = b = 0) for hess_matcher_match; rs, cp, rm, cm: offsets
// of its row states, column partials, row and column decisions in the scratch.
struct PairJob {
  int a, b, n1, n2;
  int nrb, nsuper, nseg, sps;
  int rs, cp, rm, cm;
  int pad[4];
};
static_assert(sizeof(PairJob) == 64, "PairJob is read by the kernels");

// An entry of a table of the plan buffer, the kernels' int2.  Multiply table: (job, row block | segment << 16); finish table:
// (job, block); orig table: (first original row of the pair's set 1, rows of that set).
struct alignas(8) Entry { int x, y; };

// Jobs [p0, p1) of one multiply and one finish launch, with segments of at most sps super tiles; the scratch they use (row
// states, column partials, row and column decisions) and the entries of the two work tables.
// Typed sets (jpp = 4): four jobs per pair, one per class, and behind the work tables one orig entry per pair for
// match_types_compact_kernel.
struct Chunk {
  int p0, p1, sps;
  size_t rs, cp, rm, cm, nwg, nfin;
  int jpp;  // jobs per pair
  int pairs() const { return (p1 - p0) / jpp; }
};

// The plan buffer of a chunk, in a pinned host slot and on the device alike: byte offsets of its jobs, the multiply table
// (nwg entries), the finish table (nfin) and the orig table (one entry per pair of typed sets, else none).
struct PlanLayout { size_t jobs, work, fin, orig, bytes; };
PlanLayout plan_layout(const Chunk& c);
// Fills hp (plan_layout(c).bytes) from the planned jobs; orig: one entry per pair of the whole list (typed sets only).
void plan_fill(unsigned char* hp, const PairJob* jobs, const Entry* orig, const Chunk& c, int mutual_best);
template <class T> const T* plan_ptr(const unsigned char* base, size_t offset) { return reinterpret_cast<const T*>(base + offset); }

constexpr size_t pad_rows(size_t n) { return (n + MM_ROWS - 1) / MM_ROWS * MM_ROWS; }

// Sets back to back, each padded to whole 256-row blocks: set k is counts[k] source rows, of which the first max_sift are
// kept.  off: first padded row, num: rows kept, first: first original (kept) row, src: first source row.  False: more than
// INT32_MAX / KD padded rows or INT32_MAX source rows (HESS_ERR_TOO_BIG).
bool set_layout(int nsets, const int* counts, int max_sift, size_t KD, int* off, int* num, int* first, int* src, size_t* padded);
// The same for the class groups of typed sets: goff from gnum, ngroups = 4 x sets.
bool group_layout(int ngroups, const int* gnum, size_t KD, int* goff, size_t* padded);

// Where the sets of one side of a match are: per set the first padded row, rows kept and first original row, and for typed
// sets (goff != NULL) per (set, class) the first stored row and rows of the group.
struct SetsLayout { const int *off, *num, *first, *goff, *gnum; };

// Super tiles per segment at most, for the untyped single pair on the matrix cores; a pair list has its own rule (chunk_sps,
// with pair_seg, job_work and pair_jobs in hess_match_plan.cpp).
int single_sps(int n1, int n2);
// Plans c's jobs (a, b, n1, n2 given): shapes, segments and offsets into the scratch; and c's totals.  Returns the scratch bytes.
size_t plan_chunk(PairJob* jobs, Chunk& c, int mutual_best);

// What the matcher's buffers must hold: row states and column partials (int3 each), row and column decisions, plan bytes,
// ints of compacted output (0: the caller compacts on the host).
struct PlanNeed { size_t rs, cp, rm, cm, plan_bytes, outn; };

// A planned pair list.  Pair p is jobs [jpp p, jpp p + jpp); the chunks partition the list in order; mm: matches kept per
// pair in the pinned output slot -- max_match, at most the rows of the largest set 1 (0 where set 2 is empty); need: the
// maxima over the chunks, the output MP_PAIRS counts and mm (row, column) pairs per pair of a chunk.
struct PairPlan {
  int jpp = 1, mm = 0;
  std::vector<PairJob> jobs;
  std::vector<Entry> orig;
  std::vector<Chunk> chunks;
  PlanNeed need{1, 1, 1, 1, 0, 0};
};
// False: a chunk (one pair, then) needs more scratch than one launch can address (HESS_ERR_TOO_BIG).
bool plan_pairs(const SetsLayout& s1, const SetsLayout& s2, int npairs, const int* pairs_ab, int max_match, int mutual_best,
                PairPlan& P);

}  // namespace hess::match_plan

#endif  // HESS_MATCH_PLAN_H
