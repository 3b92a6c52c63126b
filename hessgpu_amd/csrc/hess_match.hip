// hess_match.hip -- descriptor matcher for gfx950: the step after the hot path.
//
// Replaces SiftMatchCU (SiftMatchCU.cpp:71-176) and its kernels MultiplyDescriptor(_G)_Kernel,
// RowMatch_Kernel, ColMatch_Kernel (ProgramCU.cu:3455-3843).  Integer work: results are bit-exact.
//
// Descriptor sets (the user's bank, the two single-pair slots) --
//   bank_build_kernel      sets padded to 256-row blocks, float sources quantised, score offsets from the byte sums;
//   bank_loc_gather_kernel the bank's locations from strided records into the caller's row order of the kept rows.
// Unguided match (GetSiftMatch), one pair or many pairs of a bank per call (hess_matcher_match_pairs, no reference
// counterpart): matrix cores, no score matrix in memory --
//   match_mfma_kernel      one workgroup per (pair, 256-row block, column segment) of a work table: the segment's
//                          descriptors of set 2 pass through LDS once for its four wavefronts, each of which holds 64 rows
//                          of set 1 in registers and folds the v_mfma_i32_32x32x32_i8 tiles into RowMatch_Kernel's
//                          per-thread states and the column partials as packed 32-bit keys; see the comment at the kernel;
//   match_finish_kernel    per (pair, block) of a second table: merges a row's per-segment states (largest score, then
//                          the reference's tie order: the tree's thread class, lower column), acos distance + ratio; and, in
//                          the same launch, the per-row-block (max, index, second) column partials in ascending row order
//                          (match_col_kernel: the same for the small / guided path);
//   match_pairs_compact_kernel  each pair's matches compacted on the device (a single pair is compacted on the host).
// Guided match of a pair list (hess_matcher_match_pairs_guided, no reference counterpart): the same kernels, match_mfma_kernel
// in its GUIDED form -- the gate of hess_guided_gate.h per pair and the per-8-row-block rule applied to the scores before the
// folds; see the comment at the kernel.
// Verified matches of a pair list (hess_matcher_verify_pairs, no reference counterpart): both forms above and the estimator
// of hess_geom.hip chained per group of chunks in stream order, the matches never leaving the device in between --
//   verify_geo_kernel      a group's guided geometry from its estimates; see run_verify.
// Feature types (hess_matcher_set_types, _bank_set_types; no reference counterpart): a typed set is stored grouped by class
// and a gated pair is one job of the same tables per class, the two kernels above unchanged --
//   type_classify_kernel / type_place_kernel / bank_gather_kernel   class and stable position of every row, its place, the move;
//   match_types_compact_kernel  the compaction in ORIGINAL row order through the maps; see the comment at type_classify_kernel.
// Small unguided match and guided match (GetGuidedSiftMatch: per-pair homography / fundamental-matrix gates,
// per-8-row-block rule) --
//   match_dot_kernel       64x64 tile of the dot-product matrix per workgroup, descriptor panels in LDS,
//                          v_dot4_u32_u8, gates per pair, score matrix written for
//   match_row_kernel       one wavefront per row over the matrix (same tie order), and match_col_kernel.
// Host side.  What the kernels are launched on is decided in hess_match_plan.h / .cpp, without HIP: the layout of the sets,
// the segments of a pair (two rules: single_sps for the untyped single pair, chunk_sps for a pair list), the chunks of a
// list, the scratch offsets and the tables of the plan buffer.  Here: grow_for (the buffers of a plan), run_chunk (upload,
// multiply, finish), run_slots (the double buffer of every pair list: hess_slot_pipeline.h with the events, the copy down, the
// wait and the error text) and run_pairs (a pair list planned, its chunks run through it and compacted on the device), which serves
// hess_matcher_match_pairs with (bank, bank) and the typed single pair with (slot 0, slot 1) and a list of one;
// hess_matcher_match otherwise plans one job and compacts on the host, or takes match_small.
// Lifetimes are written in types: the stream and the events are hess_owned.h's, every device allocation is a DeviceBuf -- the
// members of DescSets and of the matcher, and the temporaries of a load, which `stage` fills from a host array.  A set that must
// survive a failed change (sets_regroup, bank_locations) is built in local buffers and swapped in after the last call that can fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hess_abi.h"
#include "hess_dev.h"
#include "hess_guided_gate.h"
#include "hess_match_plan.h"
#include "hess_matcher_int.h"
#include "hess_owned.h"
#include "hess_slot_pipeline.h"

using namespace hess::match_plan;  // the constants MM_*, MP_*, PairJob, the plan of a pair list and of the plan buffer
static_assert(sizeof(Entry) == sizeof(int2) && alignof(Entry) == alignof(int2), "the kernels read the plan's tables as int2");

namespace {

constexpr int TM = 64, TN = 64;
// Descriptor length KD (bytes per row): 128, or 64 (-half: hess_matcher_set_dim).  A template parameter of the kernels that
// read descriptor bytes; everything that counts scores (tiles, segments, plans, the finish) does not depend on it.
constexpr bool dim_ok(int dim) { return dim == 128 || dim == 64; }

struct GeoParams {
  int guided;
  float H[9], F[9];
  float hdistmax, fdistmax;
};

// ColMatch_Kernel's merge of two column partials (max, row, second): strict '<', so the earlier rows keep a tie.
__device__ __forceinline__ void col_merge(int3& a, const int3& b) {  // a: earlier rows, b: later rows
  if (a.x < b.x) a = make_int3(b.x, b.y, max(a.x, b.z));
  else a.z = max(a.z, b.x);
}

// dotm[i][j] = what RowMatch reads (clamped at 0 in guided mode).  cpart[tile_row][j] = (max, index,
// second) of the reference's unclamped `results` over the tile's 64 rows in ascending order -- the
// d_temp partials of MultiplyDescriptor_Kernel (ProgramCU.cu:3510-3524), 64 rows at a time instead of 8.
template <int KD>
__global__ __launch_bounds__(256) void match_dot_kernel(const uint8_t* des1, int num1, const uint8_t* des2, int num2,
                                                        const float2* loc1, const float2* loc2, GeoParams gp,
                                                        int3* cpart, int* dotm) {
  __shared__ uint32_t a[TM][KD / 4 + 1];  // +1 dword: conflict-free column-of-rows reads
  __shared__ uint32_t b[TN][KD / 4 + 1];
  __shared__ int good_blk[TM / 8][TN];
  __shared__ int3 cp[TM / 4][TN];
  const int i0 = blockIdx.y * TM, j0 = blockIdx.x * TN, tid = threadIdx.x;
  for (int g = tid; g < TM * (KD / 16); g += 256) {  // 16-byte loads
    const int r = g / (KD / 16), q = g % (KD / 16);
    uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
    if (i0 + r < num1) va = *reinterpret_cast<const uint4*>(des1 + (size_t)(i0 + r) * KD + q * 16);
    if (j0 + r < num2) vb = *reinterpret_cast<const uint4*>(des2 + (size_t)(j0 + r) * KD + q * 16);
    a[r][q * 4] = va.x; a[r][q * 4 + 1] = va.y; a[r][q * 4 + 2] = va.z; a[r][q * 4 + 3] = va.w;
    b[r][q * 4] = vb.x; b[r][q * 4 + 1] = vb.y; b[r][q * 4 + 2] = vb.z; b[r][q * 4 + 3] = vb.w;
  }
  if (tid < (TM / 8) * TN) (&good_blk[0][0])[tid] = 0;
  for (int g = tid + 256; g < (TM / 8) * TN; g += 256) (&good_blk[0][0])[g] = 0;
  __syncthreads();
  const int ti = (tid >> 4) * 4, tj = (tid & 15) * 4;  // this thread: rows ti..ti+3, cols tj..tj+3 of the tile
  int acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] = 0;
#pragma unroll 4
  for (int k = 0; k < KD / 4; k++) {
    uint32_t av[4], bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) av[r] = a[ti + r][k];
#pragma unroll
    for (int c = 0; c < 4; c++) bv[c] = b[tj + c][k];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = (int)__builtin_amdgcn_udot4(av[r], bv[c], (uint32_t)acc[r][c], false);
  }
  int base[4][4];
  if (gp.guided) {  // ProgramCU.cu:3597-3635
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = i0 + ti + r;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int j = j0 + tj + c;
        int v = -262144;
        if (i < num1 && j < num2) {
          const float2 l1 = loc1[i], l2 = loc2[j];
          hess::GuidedRow R;
          hess::guided_row_h(gp.H, l1.x, l1.y, R);
          if (hess::guided_box(R, l2.x, l2.y, gp.hdistmax)) {
            hess::guided_row_f(gp.F, l1.x, l1.y, R);
            v = hess::guided_sampson(R, hess::guided_col(gp.F, l2.x, l2.y), gp.fdistmax) ? 0 : -262144;
          }
        }
        base[r][c] = v;
        if (v >= 0) atomicAdd(&good_blk[(ti + r) >> 3][tj + c], 1);  // `good_count` of the 8-row block
      }
    }
  }
  __syncthreads();
  int3 loc_c[4];
#pragma unroll
  for (int c = 0; c < 4; c++) loc_c[c] = make_int3(0, -1, 0);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int i = i0 + ti + r;
    if (i >= num1) continue;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = j0 + tj + c;
      if (j >= num2) continue;
      int res = acc[r][c];
      if (gp.guided) res = base[r][c] + (good_blk[(ti + r) >> 3][tj + c] > 0 ? acc[r][c] : 0);
      dotm[(size_t)i * num2 + j] = gp.guided ? max(res, 0) : res;  // ProgramCU.cu:3684
      if (cpart) {  // strict '>' in ascending row order: the lowest row keeps a tie (ProgramCU.cu:3516-3519)
        if (res > loc_c[c].x) loc_c[c] = make_int3(res, i, loc_c[c].x);
        else loc_c[c].z = max(loc_c[c].z, res);
      }
    }
  }
  if (cpart) {
#pragma unroll
    for (int c = 0; c < 4; c++) cp[tid >> 4][tj + c] = loc_c[c];
    __syncthreads();
    if (tid < TN && j0 + tid < num2) {
      int3 t = cp[0][tid];
      for (int q = 1; q < TM / 4; q++) col_merge(t, cp[q][tid]);  // the 16 four-row partials in row order
      cpart[(size_t)blockIdx.y * num2 + j0 + tid] = t;
    }
  }
}

__device__ __forceinline__ int decide(int best, int second, int idx, float distmax, float ratiomax) {
  const float dist = (float)acos(fmin((double)(best * 0.000003814697265625f), 1.0));     // ProgramCU.cu:3785
  const float distn = (float)acos(fmin((double)(second * 0.000003814697265625f), 1.0));
  return (dist < distmax) && (dist < distn * ratiomax) ? idx : -1;
}

// RowMatch_Kernel semantics: lane = (class c = j mod 32, half); strict '>' per lane keeps its first
// maximum; the two lanes of a class merge towards the lower j, then the classes merge with the
// reference's own tree (partner 16, 8, 4, 2, 1 away; a tie keeps the lower class of the pair).  Among equal
// maxima the tree does NOT keep the lowest class: the last step (partner 1 away) decides bit 0 of the class, the
// one before bit 1, ..., so it keeps the class whose BIT-REVERSED number is smallest (class 16 beats class 1, class 2
// beats class 1).  match_mfma_kernel and match_finish_kernel restate that order without the tree.
__global__ __launch_bounds__(256) void match_row_kernel(const int* dotm, int num1, int num2, float distmax,
                                                        float ratiomax, int* rowm) {
  const int row = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (row >= num1) return;
  const int* p = dotm + (size_t)row * num2;
  int mx = 0, nx = 0, ix = -1;
  for (int j = lane; j < num2; j += 64) {  // lane covers j = lane, lane+64, ...: class lane&31
    const int v = p[j];
    const bool t = v > mx;
    nx = t ? mx : max(nx, v);
    ix = t ? j : ix;
    mx = t ? v : mx;
  }
  // merge: first the two lanes of a class (lower j wins ties), then classes 16,8,4,2,1 apart (the lower class of each pair wins)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int omx = __shfl_down(mx, d), onx = __shfl_down(nx, d), oix = __shfl_down(ix, d);
    bool take;  // take the other lane's candidate?
    if (d == 32) take = (omx > mx) || (omx == mx && oix >= 0 && (ix < 0 || oix < ix));
    else take = omx > mx;
    const int nmx = take ? omx : mx;
    const int nnx = take ? max(mx, onx) : max(nx, omx);
    ix = take ? oix : ix;
    nx = nnx;
    mx = nmx;
  }
  if (lane == 0) rowm[row] = decide(mx, nx, ix, distmax, ratiomax);
}

// ColMatch_Kernel (ProgramCU.cu:3808-3827): merge the row-block partials of a column in ascending row order.
// The merge is associative (ties go to the earlier rows), so a column's partials are split into 8 consecutive
// chunks folded by 8 threads and combined in chunk order: 32 columns x 8 chunks per workgroup.
__device__ __forceinline__ void match_col_block(int block, const int3* cpart, int ntile, int num2, float distmax,
                                                float ratiomax, int* colm) {
  __shared__ int3 part[8][32];
  const int c = threadIdx.x & 31, ch = threadIdx.x >> 5;
  const int j = block * 32 + c;
  const int per = (ntile + 7) >> 3;
  const int q0 = ch * per, q1 = min(q0 + per, ntile);
  int3 t = make_int3(0, -1, 0);  // neutral: the per-block partials start from the same state
  if (j < num2)
    for (int q = q0; q < q1; q++) col_merge(t, cpart[(size_t)q * num2 + j]);
  part[ch][c] = t;
  __syncthreads();
  if (ch == 0 && j < num2) {
    for (int k = 1; k < 8; k++) col_merge(t, part[k][c]);
    colm[j] = decide(t.x, t.z, t.y, distmax, ratiomax);
  }
}

__global__ __launch_bounds__(256) void match_col_kernel(const int3* cpart, int ntile, int num2, float distmax,
                                                        float ratiomax, int* colm) {
  match_col_block(blockIdx.x, cpart, ntile, num2, distmax, ratiomax, colm);
}

// ---- unguided match on the matrix cores -----------------------------------------------------------------
// The num1 x num2 dot products are never written out.
//
// Work split.  A workgroup (four wavefronts) owns 256 rows of set 1 and a segment of the columns (set 2); wavefront w
// holds rows 64 w .. 64 w + 63 as the A fragments of two 32-row blocks, resident in registers.  The segment is walked
// in SUPER TILES of 128 columns: the workgroup copies the 16 KB of descriptors (biased, see below) and the 128 column
// offsets into LDS -- one coalesced 16-byte load per thread and quarter, issued a whole super tile ahead, double
// buffered, one barrier per super tile -- and every wavefront reads its B fragments from there: set 2 crosses L2 once
// per 256 rows (round 1-5's kernel: once per 32 rows, straight from L2, 16 bytes per lane at a 32-byte stride).
// Per 32-column tile a wavefront issues 2 x 4 v_mfma_i32_32x32x32_i8.  (Figures for 128-d descriptors.  At KD = 64 a
// super tile is 8 KB, staged as two 16-byte pieces per thread, and a tile takes 2 x 2 MFMAs; the tiles, the folds and the
// keys are the same: a score is at most 64 * 255^2 < 2^22.)
//
// Scores.  Descriptors are unsigned bytes, the instruction multiplies signed ones: bytes are biased by -128 (xor 0x80)
// and the exact dot product is dot_s + 128 (sum a + sum b) - 128^2 * KD.  The row part (rfix) rides in as the MFMA's
// C operand, the column part (cfix) is added while the key is formed.  Both sets are padded with zero descriptors to
// whole blocks (rows: 256, columns: 128), whose exact score is 0 -- never a maximum (the reference's scans start at 0
// and replace on '>' only), so there is no validity test anywhere in the loop.
//
// Folds.  The C layout puts column j0 + (lane & 31) on the lane and 16 rows of a block in its registers, and a tile
// aligned to 32 columns holds exactly one element of each of RowMatch_Kernel's 32 strided threads (class = j mod 32 =
// lane & 31): the per-thread scan of the reference (strict '>' keeps the first maximum, second = second largest,
// ProgramCU.cu:3745-3760) is a per-lane fold over the tiles with no cross-lane traffic.  State per (lane, register): two
// packed keys, key = score << 6 | (62 - tile index in the segment): `best = max(best, key)` keeps the largest score and,
// among equal scores, the earliest tile; `second = med3(best, key, second)` is the second largest key, whose score is the
// second largest score counting duplicates -- three vector instructions per element (shift-add, med3, max) where
// the (max, second, index) triple took seven.  63 in the low bits = "none yet" (a score of 0 forms a key below it).
// Column partials (max, row, second over the wavefront's rows in ascending order, ColMatch's rule, ProgramCU.cu:3510-3519)
// the same way with key = score << 6 | (62 - row in the lane's half), formed from the row key by one add of a scalar.
// At the end of the segment the 32 classes of a row are merged through LDS (one lane per row and half walks 16 of them in
// the order in which the reference's tree prefers them on ties -- ascending BIT-REVERSED class, see match_row_kernel and
// ProgramCU.cu:3776-3787) and ONE (best, second, column) per row and segment is stored.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// LDS bytes per staged descriptor: KD + 16, i.e. 36 dwords (128-d) or 20 (64-d).  A 16-byte read is served in groups of 16
// lanes whose columns are distinct mod 16 (0-3, 12-15, 20-27 | 4-11, 16-19, 28-31), each lane taking 4 consecutive banks of
// 64: the group is conflict-free exactly when pitch / 16 bytes is odd (9, 5), a bijection of the columns mod 16 onto the 16
// four-bank slots.  The unpadded 64 bytes (4) would be 4-way.  (Staging stores at 64-d: 8 lanes write two columns, 20 dwords
// apart over 32 banks: one of their 8 pieces meets a busy bank.)
template <int KD> constexpr int mm_pitch() { return KD + 16; }
constexpr int MM_RS_PITCH = 33;         // row-state exchange: 8-byte entries per row (32 classes + 1 pad)
constexpr int MM_RS_BYTES = 4 * 32 * MM_RS_PITCH * 8;
// One of the two descriptor buffers: a super tile, and half of the row-state exchange that reuses both at the end (at 64-d
// the exchange, 33 792 B, is larger than two staged super tiles, 20 480 B)
template <int KD> constexpr int mm_buf_bytes() {
  return MM_SUPER * mm_pitch<KD>() > MM_RS_BYTES / 2 ? MM_SUPER * mm_pitch<KD>() : MM_RS_BYTES / 2;
}

// median of three (v_med3_i32: the compiler does not form it from min/max of three variables)
__device__ __forceinline__ int med3i(int a, int b, int c) {
  int d;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// One pair's geometry on the device (hess_matcher_match_pairs_guided): hess_guided_pair and where the locations of its two
// sets start in the bank's locations (DescSets::first: the caller's row order, not padded).  A matrix with a non-finite
// entry arrives as zeros: nothing passes.
struct GuidedGeo {
  float H[9], F[9];
  float hdistmax, fdistmax;
  int la, lb;
};
static_assert(sizeof(hess_guided_pair) == 80, "hess_guided_pair is ABI");

// The work of one workgroup (PairJob, the tables: hess_match_plan.h): work[blockIdx.x] = (job, rb | sg << 16), row block rb of the job's set 1 against its column
// segment sg of set 2.
//
// GUIDED (hess_matcher_match_pairs_guided): the score that enters the folds is the one MultiplyDescriptorG_Kernel stores
// (match_dot_kernel above): the dot product where (row, column) passes the gate of geo[job] (hess_guided_gate.h), the dot
// product - 2^18 clamped at 0 where it fails but a row of its 8-row block passes with that column (`good_count`), else 0.
// A lane's 16 accumulator registers are 16 consecutive rows from a multiple of 16 (set starts are 256-row aligned), i.e.
// two whole 8-row blocks, so `good_count > 0` is a lane-local OR of eight pass bits.  The row terms of the workgroup's 256
// rows are computed once into LDS (rowh, rowf; a half-wave reads one address), the column terms of a super tile beside cfix
// (bufG).  Locations are not padded: a row >= n1 or a column >= n2 reads none and holds NaN, which fails the box test --
// a padded row that passed would switch on the block rule for the real rows of a ragged last block.
template <bool COLS, int KD, bool GUIDED>
__global__ __launch_bounds__(256) void match_mfma_kernel(const uint8_t* rows1, const int* rfix, const uint8_t* rows2,
                                                         const int* cfix, const PairJob* jobs, const int2* work,
                                                         int3* cpart, int3* rstate, const GuidedGeo* geo, const float2* loc) {
  constexpr int MM_PITCH = mm_pitch<KD>(), KK = KD / 32;  // MFMAs (32 bytes of every descriptor each) per block and tile
  __shared__ __attribute__((aligned(16))) uint8_t bufB[2][mm_buf_bytes<KD>()];
  __shared__ int bufC[2][MM_SUPER];
  __shared__ int3 cp[2][4][MM_SUPER];  // the four wavefronts' column partials of a super tile, merged after its barrier
  // GUIDED, per row of the workgroup: (px, py), (fx0, fx1, fx2, rr), and the row's score offset, which the other form keeps
  // in registers as the MFMA's C operand (32 of them: the gate needs the room)
  __shared__ float2 rowh[GUIDED ? MM_ROWS : 1];
  __shared__ float4 rowf[GUIDED ? MM_ROWS : 1];
  __shared__ __attribute__((aligned(16))) int rowc[GUIDED ? MM_ROWS : 1];
  __shared__ float bufG[GUIDED ? 2 : 1][GUIDED ? 4 : 1][GUIDED ? MM_SUPER : 1];              // x, y, ft0, ft1 of a super tile's columns
  static_assert(sizeof(bufB) >= MM_RS_BYTES && mm_buf_bytes<KD>() % 16 == 0, "the row-state exchange reuses the descriptor buffers");
  const int2 w = work[blockIdx.x];
  const PairJob& J = jobs[w.x];
  const unsigned rb = w.y & 0xffff;
  const int sg = w.y >> 16;
  const uint8_t* const des1 = rows1 + (size_t)J.a * KD;
  const uint8_t* const des2 = rows2 + (size_t)J.b * KD;
  const int num1 = J.n1, num2 = J.n2, nseg = J.nseg, nsuper = J.nsuper;
  rfix += J.a;
  cfix += J.b;
  cpart += J.cp;
  rstate += J.rs;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int i0 = rb * MM_ROWS + wv * 64;  // this wavefront's first row
  const int s0 = sg * J.sps, s1 = min(s0 + J.sps, nsuper);
  v4i a[2][KK];
  v16i ra[2];
  {
    // hardware row r of a tile carries descriptor row perm(r) of the block, chosen so that the 16 accumulator registers
    // of a lane are 16 CONSECUTIVE descriptor rows (reg + 16 h): a lane's column partial is then a plain in-order fold
    const int prow = (r & 3) + 4 * (r >> 3) + 16 * ((r >> 2) & 1);
#pragma unroll
    for (int blk = 0; blk < 2; blk++) {
      const uint8_t* pa = des1 + (size_t)(i0 + 32 * blk + prow) * KD + 16 * h;  // (set 1 is padded to whole workgroups)
#pragma unroll
      for (int kk = 0; kk < KK; kk++) a[blk][kk] = *reinterpret_cast<const v4i*>(pa + kk * 32) ^ (int)0x80808080;
      if constexpr (!GUIDED) {
        const v4i* const pr = reinterpret_cast<const v4i*>(rfix + i0 + 32 * blk + 16 * h);  // (16 consecutive rows: 64-byte aligned)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const v4i t = pr[q];
          ra[blk][4 * q] = t.x; ra[blk][4 * q + 1] = t.y; ra[blk][4 * q + 2] = t.z; ra[blk][4 * q + 3] = t.w;
        }
      }
    }
  }
  int rmx[2][16], rnx[2][16];
#pragma unroll
  for (int blk = 0; blk < 2; blk++)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) { rmx[blk][reg] = 63; rnx[blk][reg] = 0; }

  // staging: thread t copies 16-byte pieces t, t + 256, ... (KD / 32 of them) of a super tile (piece = KD / 16 x column + part)
  v4i st[KK];
  int stc = 0;
  [[maybe_unused]] float hdm = 0.0f, fdm = 0.0f;
  [[maybe_unused]] hess::GuidedCol stg = {0.0f, 0.0f, 0.0f, 0.0f};
  [[maybe_unused]] const float2* loc2 = nullptr;
  [[maybe_unused]] const float* gF = nullptr;
  if constexpr (GUIDED) {
    const GuidedGeo& G = geo[w.x];
    hdm = G.hdistmax;
    fdm = G.fdistmax;
    gF = G.F;
    loc2 = loc + G.lb;
    // the row terms of this workgroup's 256 rows, one row per thread (visible after the barrier below)
    const int gi = (int)rb * MM_ROWS + tid;
    hess::GuidedRow R;
    R.px = R.py = __builtin_nanf("");
    R.fx0 = R.fx1 = R.fx2 = R.rr = 0.0f;
    if (gi < num1) {
      const float2 l1 = loc[G.la + gi];
      hess::guided_row_h(G.H, l1.x, l1.y, R);
      hess::guided_row_f(G.F, l1.x, l1.y, R);
    }
    rowh[tid] = make_float2(R.px, R.py);
    rowf[tid] = make_float4(R.fx0, R.fx1, R.fx2, R.rr);
    rowc[tid] = rfix[gi];  // (set 1 is padded to whole workgroups)
  }
  auto stage_load = [&](int sup) {
    const uint8_t* src = des2 + (size_t)sup * MM_SUPER * KD + (size_t)tid * 16;
#pragma unroll
    for (int q = 0; q < KK; q++) st[q] = *reinterpret_cast<const v4i*>(src + q * 4096);
    if (tid < MM_SUPER) stc = cfix[sup * MM_SUPER + tid];
    if constexpr (GUIDED) {
      if (tid < MM_SUPER) {
        const int j = sup * MM_SUPER + tid;
        stg = hess::GuidedCol{__builtin_nanf(""), __builtin_nanf(""), 0.0f, 0.0f};
        if (j < num2) {
          const float2 l2 = loc2[j];
          stg = hess::guided_col(gF, l2.x, l2.y);
        }
      }
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int q = 0; q < KK; q++) {
      const int piece = tid + 256 * q;
      constexpr int PS = KD == 128 ? 3 : 2;  // log2 of the pieces per column
      *reinterpret_cast<v4i*>(&bufB[buf][(piece >> PS) * MM_PITCH + (piece & (KD / 16 - 1)) * 16]) = st[q] ^ (int)0x80808080;
    }
    if (tid < MM_SUPER) bufC[buf][tid] = stc;
    if constexpr (GUIDED) {
      if (tid < MM_SUPER) {
        bufG[buf][0][tid] = stg.x; bufG[buf][1][tid] = stg.y; bufG[buf][2][tid] = stg.ft0; bufG[buf][3][tid] = stg.ft1;
      }
    }
  };
  stage_load(s0);
  stage_store(0);
  __syncthreads();
  for (int sup = s0; sup < s1; sup++) {
    const int cur = (sup - s0) & 1;
    if (sup + 1 < s1) stage_load(sup + 1);  // in flight while this super tile is multiplied
    // (one tile at a time: a software pipeline over the tiles -- the next tile's fragments read and its MFMAs issued between
    // this tile's folds -- was measured twice and lost both times: unrolled it needs 260 registers and spills (- 9 %),
    // rolled it fits 191 and runs 3 % slower than this loop, whose waits the SIMD's other wavefront fills:
    // profiles/r06_experiments/matcher.txt)
#pragma unroll 1
    for (int tt = 0; tt < 4; tt++) {
      const int tl = (sup - s0) * 4 + tt;     // tile index in the segment
      const int ct = 62 - tl;
      const uint8_t* pb = &bufB[cur][(tt * 32 + r) * MM_PITCH + 16 * h];
      v4i b[KK];
#pragma unroll
      for (int kk = 0; kk < KK; kk++) b[kk] = *reinterpret_cast<const v4i*>(pb + kk * 32);
      const int cbk = (bufC[cur][tt * 32 + r] << 6) | ct;
      [[maybe_unused]] hess::GuidedCol gc = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (GUIDED)
        gc = hess::GuidedCol{bufG[cur][0][tt * 32 + r], bufG[cur][1][tt * 32 + r], bufG[cur][2][tt * 32 + r], bufG[cur][3][tt * 32 + r]};
      int cx = 63, cz = 0;  // column partial over this lane's 32 rows
      auto fold = [&](int blk, int reg, int k) {  // key k of (row reg of block blk, this lane's column) into both states
        rnx[blk][reg] = med3i(rmx[blk][reg], k, rnx[blk][reg]);
        rmx[blk][reg] = max(rmx[blk][reg], k);
        if (COLS) {
          const int kc = k + ((62 - (reg + 16 * blk)) - ct);            // low bits: 62 - row in the lane's half
          cz = med3i(cx, kc, cz);
          cx = max(cx, kc);
        }
      };
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
        v16i c;
        if constexpr (GUIDED) {
          const v4i* const pr = reinterpret_cast<const v4i*>(&rowc[wv * 64 + 32 * blk + 16 * h]);
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const v4i t = pr[q];
            c[4 * q] = t.x; c[4 * q + 1] = t.y; c[4 * q + 2] = t.z; c[4 * q + 3] = t.w;
          }
        } else {
          c = ra[blk];
        }
#pragma unroll
        for (int kk = 0; kk < KK; kk++) c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[blk][kk], b[kk], c, 0, 0, 0);
        if constexpr (GUIDED) {
          // an 8-row block at a time: the pass bits of its rows with this lane's column, then the block rule on the scores
          const int cf = bufC[cur][tt * 32 + r];
#pragma unroll
          for (int half = 0; half < 2; half++) {
            const int lr = wv * 64 + 32 * blk + 16 * h + 8 * half;  // the block's first row in the workgroup
            unsigned pass = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
              const float2 t = rowh[lr + q];
              hess::GuidedRow R;
              R.px = t.x;
              R.py = t.y;
              pass |= hess::guided_box(R, gc.x, gc.y, hdm) ? 1u << q : 0u;
            }
            // (wavefront-uniform.)  Where no lane's block passes the box, every score of the 8 x 64 elements is 0: a key below
            // "none yet" and below every second best that carries a score, so folding it changes no state that is ever
            // decoded -- the F part and the folds are skipped, which is most blocks under a real H bound
            if (__builtin_amdgcn_ballot_w64(pass != 0) != 0) {
              unsigned pf = 0;
#pragma unroll
              for (int q = 0; q < 8; q++) {
                const float4 t = rowf[lr + q];
                hess::GuidedRow R;
                R.fx0 = t.x; R.fx1 = t.y; R.fx2 = t.z; R.rr = t.w;
                pf |= hess::guided_sampson(R, gc, fdm) ? 1u << q : 0u;
                // (four divisions in flight, not eight: scheduled as one block the 128-d form with column partials needs
                // 262 registers and falls to one wavefront per SIMD; with this fence 231, without scratch)
                if (q == 3) __builtin_amdgcn_sched_barrier(0);
              }
              pass &= pf;
#pragma unroll
              for (int q = 0; q < 8; q++) {
                const int sc = c[8 * half + q] + cf;  // the dot product
                const int sg = (pass >> q) & 1u ? sc : (pass != 0 && sc > 262144 ? sc - 262144 : 0);
                fold(blk, 8 * half + q, (sg << 6) | ct);
              }
            }
          }
        } else {
#pragma unroll
          for (int reg = 0; reg < 16; reg++)
            fold(blk, reg, (int)(((unsigned)c[reg] << 6) + (unsigned)cbk));  // (score << 6) | ct: score = c + column offset >= 0
        }
      }
      if (COLS) {
        // the lane's rows are (reg, 32 + reg) + 16 h of the wavefront's 64: decode, then merge the two lane halves
        // (largest score; equal scores: the lower row, ColMatch's ascending order)
        const int low = cx & 63, rl = 62 - low;
        int bx = cx >> 6, by = low == 63 ? -1 : i0 + 32 * (rl >> 4) + (rl & 15) + 16 * h, bz = cz >> 6;
        const int ox = __shfl_xor(bx, 32), oy = __shfl_xor(by, 32), oz = __shfl_xor(bz, 32);
        const bool take = ox > bx || (ox == bx && oy >= 0 && (by < 0 || oy < by));
        const int nz = max(max(bz, oz), min(bx, ox));
        bx = take ? ox : bx;
        by = take ? oy : by;
        if (h == 0) cp[cur][wv][tt * 32 + r] = make_int3(bx, by, nz);
      }
    }
    if (sup + 1 < s1) stage_store(cur ^ 1);  // (read last during super tile sup - 1: every wavefront is past that barrier)
    __syncthreads();
    if (COLS && tid < MM_SUPER) {
      // one partial per column and WORKGROUP (256 rows): the wavefronts' partials in row order (ColMatch's merge rule);
      // cp[cur] is next written during super tile sup + 2, i.e. after the barrier that ends sup + 1
      int3 t = cp[cur][0][tid];
#pragma unroll
      for (int w = 1; w < 4; w++) col_merge(t, cp[cur][w][tid]);
      const int j = sup * MM_SUPER + tid;
      if (j < num2) cpart[(size_t)rb * num2 + j] = t;
    }
  }
  // ---- the 32 classes of every row -> one state per row and segment, through LDS (the descriptor buffers are free) ----
  int2* const rs = reinterpret_cast<int2*>(&bufB[0][0]) + wv * 32 * MM_RS_PITCH;
#pragma unroll
  for (int blk = 0; blk < 2; blk++) {
#pragma unroll
    for (int reg = 0; reg < 16; reg++) rs[(reg + 16 * h) * MM_RS_PITCH + r] = make_int2(rmx[blk][reg], rnx[blk][reg]);
    __builtin_amdgcn_wave_barrier();  // (one wavefront's LDS operations complete in order)
    {
      // the tree's order of preference among equal scores is ascending bit-reversed class: position k = c2 + 16 hh of that
      // order is class brev5(k) = 2 brev4(c2) + hh.  Lane (row r, half hh) walks its 16 classes (the even ones for hh = 0, the
      // odd ones for hh = 1) in that order ('>' on the score: the earlier position keeps a tie); then the two halves of a
      // row are combined the same way (half 0, positions 0..15, wins a tie)
      const int2* const row = rs + r * MM_RS_PITCH + h;
      int2 s = row[0];
      int cls = h;
#pragma unroll 5
      for (int c2 = 1; c2 < 16; c2++) {
        const int c = 2 * (int)(__brev((unsigned)c2) >> 28);  // (uniform: scalar)
        const int2 u = row[c];
        const bool take = (u.x >> 6) > (s.x >> 6);
        s.y = take ? max(s.x, u.y) : max(s.y, u.x);
        s.x = take ? u.x : s.x;
        cls = take ? c + h : cls;
      }
      const int ox = __shfl_xor(s.x, 32), oy = __shfl_xor(s.y, 32), ocls = __shfl_xor(cls, 32);
      const bool take = (ox >> 6) > (s.x >> 6);   // (meaningful in the lanes of half 0, which store)
      s.y = take ? max(s.x, oy) : max(s.y, ox);
      s.x = take ? ox : s.x;
      cls = take ? ocls : cls;
      const int low = s.x & 63;
      const int grow = i0 + 32 * blk + r;
      if (h == 0 && grow < num1)
        rstate[(size_t)grow * nseg + sg] = make_int3(s.x >> 6, s.y >> 6, low == 63 ? -1 : (s0 * 4 + 62 - low) * 32 + cls);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Rows and columns of every pair of a launch: work[blockIdx.x] = (job, block); blocks [0, row blocks of the job) take its
// rows, the rest its columns (match_col_block) -- a launch of its own for either costs more than its work: 5 us each at
// 8192 x 8192.  Rows: merge the per-segment states in the reference's order -- largest score; equal scores: the thread
// class (column mod 32) the tree prefers, i.e. the smaller bit-reversed class (see match_row_kernel), then the lower column
// (a thread keeps its first maximum).
__global__ __launch_bounds__(256) void match_finish_kernel(const PairJob* jobs, const int2* work, const int3* rstate,
                                                           const int3* cpart, float distmax, float ratiomax, int* rowm,
                                                           int* colm) {
  const int2 w = work[blockIdx.x];
  const PairJob& J = jobs[w.x];
  const int row_blocks = (J.n1 + 255) / 256;
  if (w.y >= row_blocks) {  // (workgroup-uniform)
    match_col_block(w.y - row_blocks, cpart + J.cp, J.nrb, J.n2, distmax, ratiomax, colm + J.cm);
    return;
  }
  const int row = w.y * 256 + threadIdx.x;
  if (row >= J.n1) return;
  const int3* p = rstate + J.rs + (size_t)row * J.nseg;
  int3 s = p[0];
  for (int q = 1; q < J.nseg; q++) {
    const int3 u = p[q];
    const unsigned bu = __brev((unsigned)u.z) >> 27, bs = __brev((unsigned)s.z) >> 27;  // bit-reversed classes
    const bool take = u.x > s.x || (u.x == s.x && u.z >= 0 && (s.z < 0 || bu < bs || (bu == bs && u.z < s.z)));
    s.y = u.x > s.x ? max(s.x, u.y) : max(s.y, u.x);
    if (take) { s.x = u.x; s.z = u.z; }
  }
  rowm[J.rm + row] = decide(s.x, s.y, s.z, distmax, ratiomax);
}

// Descriptor sets: back to back on the device, each padded with zero descriptors to whole 256-row blocks, with the score
// offsets of both sides.  Build: KD / 4 lanes x 4 bytes per descriptor, 8 (128-d) or 16 (64-d) per workgroup.  sets[s] =
// (first padded row, first source row, rows) in ascending padded rows; padded rows past a set's count are zero.  Float
// sources are quantised as the host does and as the descriptor kernels' byte output is: desc_pack4 (hess_dev.h).
template <bool F32, int KD>
__global__ __launch_bounds__(256) void bank_build_kernel(const void* src, const int3* sets, int nsets, int total,
                                                         uint8_t* bank, int* rfix, int* cfix) {
  constexpr int LPD = KD / 4;  // lanes per descriptor
  const int g = blockIdx.x * (256 / LPD) + threadIdx.x / LPD, l = threadIdx.x % LPD;
  if (g >= total) return;  // (uniform over the lanes of a descriptor)
  int lo = 0, hi = nsets - 1;  // the last set starting at or before g (empty sets share their successor's start)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sets[mid].x <= g) lo = mid;
    else hi = mid - 1;
  }
  const int3 S = sets[lo];
  const int r = g - S.x;
  uint32_t v = 0;
  if (r < S.z) {
    const size_t e = ((size_t)S.y + r) * KD + 4 * l;
    if (F32) {
      const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + e);
      v = hess::desc_pack4(f.x, f.y, f.z, f.w);
    } else {
      v = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src) + e);
    }
  }
  *reinterpret_cast<uint32_t*>(bank + (size_t)g * KD + 4 * l) = v;
  int sum = (int)(v & 255) + (int)((v >> 8) & 255) + (int)((v >> 16) & 255) + (int)(v >> 24);
#pragma unroll
  for (int d = LPD / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, LPD);
  if (l == 0) {  // score offsets of match_mfma_kernel: rows 128*sum - 128^2*KD, columns 128*sum
    cfix[g] = 128 * sum;
    rfix[g] = 128 * sum - 128 * 128 * KD;
  }
}

// ---- feature types (hess_matcher_set_types / _bank_set_types): sets stored grouped by class ---------------------------
// Class of a feature = type & 3 (dark, bright, saddle, none).  A typed set is stored as four class groups, each in
// ascending original order and padded to whole 256-row blocks like a set, so the gated match of a pair is the ungated
// match of up to four (group of set 1, group of set 2) jobs of the same tables: match_mfma_kernel and match_finish_kernel
// see smaller sets and nothing else.  fwd[original row] = stored row, inv[stored row] = original row of its set (-1: padding).
//
// One workgroup per set: pos[original row] = (position within its class) << 2 | class and counts[set][class].  Ballots
// and prefix counts in row order: the positions do not depend on scheduling.  sets[s] = (first value of the caller's
// array, rows kept, first original row).
__global__ __launch_bounds__(256) void type_classify_kernel(const uint8_t* types, size_t stride, const int3* sets, int* pos,
                                                            int* counts) {
  __shared__ int wsum[4][4];
  const int3 S = sets[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  for (int base = 0; base < S.y; base += 256) {
    const int i = base + tid;
    int cls = 4;
    if (i < S.y) cls = *reinterpret_cast<const uint16_t*>(types + ((size_t)S.x + i) * stride) & 3;
    int before = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const unsigned long long bal = __ballot(cls == c);
      if (lane == 0) wsum[wv][c] = __popcll(bal);
      if (cls == c) before = __popcll(bal & ((1ull << lane) - 1));
    }
    __syncthreads();
    int t[4], mine = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      t[c] = wsum[0][c] + wsum[1][c] + wsum[2][c] + wsum[3][c];
      int w = 0;
      for (int k = 0; k < wv; k++) w += wsum[k][c];
      const int start = c == 0 ? n0 : c == 1 ? n1 : c == 2 ? n2 : n3;
      if (cls == c) mine = start + w + before;
    }
    if (i < S.y) pos[S.z + i] = mine << 2 | cls;
    n0 += t[0]; n1 += t[1]; n2 += t[2]; n3 += t[3];
    __syncthreads();
  }
  if (tid == 0) {
    counts[4 * blockIdx.x] = n0; counts[4 * blockIdx.x + 1] = n1;
    counts[4 * blockIdx.x + 2] = n2; counts[4 * blockIdx.x + 3] = n3;
  }
}

// One thread per original row: where it is stored now (old_fwd, or its set's plain order without one) and where it goes
// (its class group by pos, or the plain order without one).  tab[s] = {first original row, first padded row of the plain
// order, first row of each class group}.  src and inv arrive filled with -1 (padding).
struct TypeSet { int first, off, grp[4]; };
__global__ __launch_bounds__(256) void type_place_kernel(const TypeSet* tab, int nsets, int total, const int* pos,
                                                         const int* old_fwd, int* fwd, int* inv, int* src) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  int lo = 0, hi = nsets - 1;  // the last set starting at or before idx (empty sets share their successor's start)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= idx) lo = mid;
    else hi = mid - 1;
  }
  const TypeSet S = tab[lo];
  const int i = idx - S.first;
  int to = S.off + i;
  if (pos) {
    const int p = pos[idx];
    to = S.grp[p & 3] + (p >> 2);
  }
  src[to] = old_fwd ? old_fwd[idx] : S.off + i;
  if (fwd) { fwd[idx] = to; inv[to] = i; }
}

// The sets in another order: row g and its score offsets from row src[g] of the old storage, zero (bank_build_kernel's
// padding) where src[g] < 0.  KD / 16 lanes x 16 bytes per descriptor.
template <int KD>
__global__ __launch_bounds__(256) void bank_gather_kernel(const uint8_t* orows, const int* orfix, const int* ocfix,
                                                          const int* src, int total, uint8_t* rows, int* rfix, int* cfix) {
  constexpr int LPD = KD / 16;
  const int g = blockIdx.x * (256 / LPD) + threadIdx.x / LPD, l = threadIdx.x % LPD;
  if (g >= total) return;
  const int s = src[g];
  uint4 v = make_uint4(0, 0, 0, 0);
  if (s >= 0) v = *reinterpret_cast<const uint4*>(orows + (size_t)s * KD + 16 * l);
  *reinterpret_cast<uint4*>(rows + (size_t)g * KD + 16 * l) = v;
  if (l == 0) {
    cfix[g] = s >= 0 ? ocfix[s] : 0;
    rfix[g] = s >= 0 ? orfix[s] : -128 * 128 * KD;
  }
}

// One 256-row step of a compaction, by the whole workgroup: row i's match (i, j) goes to place n + (the rows before it in
// the step with j >= 0) of out if that is below max_match; n counts on.  wsum: four ints of LDS.
__device__ __forceinline__ void compact_step(int i, int j, int& n, int max_match, int* out, int* wsum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(j >= 0);
  if (lane == 0) wsum[wv] = __popcll(bal);
  __syncthreads();
  int pos = n + __popcll(bal & ((1ull << lane) - 1));
  for (int k = 0; k < wv; k++) pos += wsum[k];
  if (j >= 0 && pos < max_match) { out[2 * pos] = i; out[2 * pos + 1] = j; }
  n += wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
}

// match_pairs_compact_kernel for typed sets.  Pair blockIdx.x is jobs[4 x + class] (a job without work has n1 = 0);
// orig[x] = (first original row of its set 1, rows of that set).  The ORIGINAL rows in ascending order: each row's
// decision is looked up through fwd in the job of its class, its column mapped back through inv, so the first max_match
// kept are those of the definition.
__global__ __launch_bounds__(256) void match_types_compact_kernel(const PairJob* jobs, const int2* orig, const int* fwd1,
                                                                  const int* inv2, const int* rowm, const int* colm,
                                                                  int mutual_best, int max_match, int* counts, int* pairs) {
  __shared__ int wsum[4];
  const PairJob* const J4 = jobs + 4 * blockIdx.x;
  const int2 O = orig[blockIdx.x];
  int* out = pairs + (size_t)blockIdx.x * max_match * 2;
  const int tid = threadIdx.x;
  // a row's answer is a chain of four dependent loads (fwd, row decision, column decision, inv) and a pair has one
  // workgroup: four 256-row steps are looked up at once, stage by stage and without branches (a row without an answer
  // reads element 0 and drops it), so that their chains are in flight together; then they are placed in order
  constexpr int U = 4;
  int n = 0;
  const bool work = (J4[0].n1 | J4[1].n1 | J4[2].n1 | J4[3].n1) != 0;  // (else set 2 may have no inv at all)
  for (int base = 0; work && base < O.y && n < max_match; base += 256 * U) {
    int jv[U], g[U], r[U], n2[U], cm[U], b[U], jj[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; u++) g[u] = fwd1[O.x + min(base + 256 * u + tid, O.y - 1)];
#pragma unroll
    for (int u = 0; u < U; u++) {
      int rm = 0;
      ok[u] = false;
      r[u] = n2[u] = cm[u] = b[u] = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const PairJob& J = J4[c];
        const int rr = g[u] - J.a;
        const bool in = rr >= 0 && rr < J.n1;
        ok[u] = ok[u] || in;
        r[u] = in ? rr : r[u]; rm = in ? J.rm : rm; n2[u] = in ? J.n2 : n2[u]; cm[u] = in ? J.cm : cm[u]; b[u] = in ? J.b : b[u];
      }
      ok[u] = ok[u] && base + 256 * u + tid < O.y;
      jj[u] = rowm[ok[u] ? rm + r[u] : 0];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      ok[u] = ok[u] && jj[u] >= 0 && jj[u] < n2[u];
      if (mutual_best) ok[u] = (colm[ok[u] ? cm[u] + jj[u] : 0] == r[u]) && ok[u];  // (uniform)
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int v = inv2[ok[u] ? b[u] + jj[u] : 0];
      jv[u] = ok[u] ? v : -1;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      compact_step(base + 256 * u + tid, jv[u], n, max_match, out, wsum);
    }
  }
  if (tid == 0) counts[blockIdx.x] = min(n, max_match);
}

// One workgroup per pair: the rows i in ascending order with rowm[i] >= 0 (and, for mutual best, colm[rowm[i]] == i),
// the first max_match of them.  out: [MP_PAIRS] counts, then [pair][max_match][2].
__global__ __launch_bounds__(256) void match_pairs_compact_kernel(const PairJob* jobs, const int* rowm, const int* colm,
                                                                  int mutual_best, int max_match, int* counts,
                                                                  int* pairs) {
  __shared__ int wsum[4];
  const PairJob& J = jobs[blockIdx.x];
  const int* rm = rowm + J.rm;
  const int* cm = colm + J.cm;
  int* out = pairs + (size_t)blockIdx.x * max_match * 2;
  const int tid = threadIdx.x;
  int n = 0;
  for (int base = 0; base < J.n1 && n < max_match; base += 256) {
    const int i = base + tid;
    int j = -1;
    if (i < J.n1) {
      j = rm[i];
      if (j >= J.n2 || (j >= 0 && mutual_best && cm[j] != i)) j = -1;
    }
    compact_step(i, j, n, max_match, out, wsum);
  }
  if (tid == 0) counts[blockIdx.x] = min(n, max_match);
}

// hess_matcher_verify_pairs: the guided geometry of a chunk's np pairs from the estimates res[q], by the rules the host path
// (run_pairs) applies to a caller's hess_guided_pair -- the estimated matrix with `bound`, the identity with 1e20 for the
// other gate (the one-matrix rule), zeros for a matrix with a non-finite entry -- and the first location rows lalb[q] of the
// pair's sets.  A pair without a model has M all zero: nothing passes.
__global__ __launch_bounds__(64) void verify_geo_kernel(const hess_geom_result* res, const int2* lalb, int np, int model_h,
                                                        float bound, GuidedGeo* geo) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= np) return;
  GuidedGeo g;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const float v = res[q].M[k], id = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
    finite = finite && fabsf(v) <= 3.402823466e38f;  // (false for NaN and infinity)
    g.H[k] = model_h ? v : id;
    g.F[k] = model_h ? id : v;
  }
  if (!finite) {
#pragma unroll
    for (int k = 0; k < 9; k++) g.H[k] = g.F[k] = 0.0f;
  }
  g.hdistmax = model_h ? bound : 1e20f;
  g.fdistmax = model_h ? 1e20f : bound;
  const int2 l = lalb[q];
  g.la = l.x;
  g.lb = l.y;
  geo[q] = g;
}

// out[first kept row of set + i] = the (x, y) at record (first record of the set + i) of src, records `stride` bytes apart.
// sets[s] = (first kept row, first record, rows kept) in ascending kept rows.
__global__ __launch_bounds__(256) void bank_loc_gather_kernel(const unsigned char* src, size_t stride, const int3* sets,
                                                              int nsets, int total, float2* out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  int lo = 0, hi = nsets - 1;  // the last set starting at or before g (empty sets share their successor's start)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sets[mid].x <= g) lo = mid;
    else hi = mid - 1;
  }
  const int3 S = sets[lo];
  const float* p = reinterpret_cast<const float*>(src + ((size_t)S.y + (size_t)(g - S.x)) * stride);
  out[g] = make_float2(p[0], p[1]);
}

// Descriptor sets on the device (bank_build_kernel's layout); a zero-padded set serves as either side of a match.  Every
// buffer frees itself: not copyable, and what empties a set (sets_clear, sets_drop_locations) resets members.
struct DescSets {
  int dim = 128;  // bytes per row (the matcher's dim when the sets were built)
  DeviceBuf<uint8_t> rows;
  DeviceBuf<int> rfix;                   // 2 x padded rows, allocated to the element: the row offsets, then the column offsets
  std::vector<int> off, num;             // first padded row and stored descriptors of each set (in the caller's order)
  std::vector<int> cnt, first;           // descriptors the caller counted per set (before max_sift); first original row
  bool built = false;                    // descriptors were loaded (possibly none)
  // feature types (hess_matcher_set_types, _bank_set_types): the rows are stored by class instead
  bool typed = false;
  std::vector<int> goff, gnum;           // [set][class]: first stored row and rows of the class group
  DeviceBuf<int> fwd, inv;               // original row (first[s] + i) -> stored row; stored row -> i, -1 for padding
  // locations (hess_matcher_set_locations, _bank_set_locations): one (x, y) per kept row in the caller's order, set s from
  // first[s] on -- NOT padded like the descriptors, and not moved by the types.  A set without rows has them with loc.p NULL.
  DeviceBuf<float2> loc;
  bool have_loc = false;
  int* cfix() const { return rfix.p + rfix.cap / 2; }
  int count(int s) const { return s < (int)num.size() ? num[s] : 0; }
  SetsLayout layout() const { return {off.data(), num.data(), first.data(), typed ? goff.data() : nullptr, typed ? gnum.data() : nullptr}; }
};

}  // namespace

// Every member frees itself (hess_owned.h, DescSets, DeviceBuf, PinnedSlots), so hess_matcher_destroy is `delete`.  The stream
// and the events stand BEFORE everything that holds memory: members go in reverse order, the buffers first, the handles last.
// Calls on one matcher are serialised by the caller and every entry point returns with the stream idle, so the pair-list
// entry points share one plan buffer and one output buffer.
struct hess_matcher {
  int device = 0, max_sift = 4096;
  int dim = 128;  // descriptor length of every set and argument: hess_matcher_set_dim
  hess::Stream st;
  hess::Event e0, e1;        // around the kernels of a single pair
  hess::Event mp_ev[2][3];   // per pinned slot of a pair list: start, kernels done, copy done; created by slot_events
  DescSets bank, slot[2];    // hess_matcher_bank_*; the one-set slots of set_descriptors(0|1)
  hess_geom_state_ptr geom;  // hess_geom.hip: the estimator's buffers
  // small / guided path: score matrix and column partials per 64-row tile (sized together: match_small)
  DeviceBuf<int3> cpart;
  DeviceBuf<int> dotm;
  // matrix-core path: row states, column partials per 256-row block
  DeviceBuf<int3> mm_rstate, mm_cpart;
  // row and column decisions of both paths
  DeviceBuf<int> rowm, colm;
  std::vector<int> hrow, hcol;
  std::string err;
  float last_ms = 0.0f;
  // pair lists and the single pair on the matrix cores: the plan (jobs, work tables; for verify_pairs those of a group's
  // chunks) on the device and in two pinned host slots
  DeviceBuf<uint8_t> plan;
  PinnedSlots<uint8_t> hplan;
  // pair lists: a unit's results on the device (match_pairs: counts, then compacted matches; verify_pairs: VerifyLayout) and
  // through two pinned host slots, in bytes
  DeviceBuf<uint8_t> out;
  PinnedSlots<uint8_t> hout;
  DeviceBuf<GuidedGeo> geo;  // match_pairs_guided: the call's geometry table; verify_pairs: a group's
  DeviceBuf<int2> vp_lalb;   // verify_pairs: per pair of the call the first location rows of its two sets
};

namespace {

void sets_drop_locations(DescSets& s) {
  s.loc.reset();
  s.have_loc = false;
}

void sets_clear(DescSets& s) {
  s.rows.reset();
  s.rfix.reset();
  s.fwd.reset();
  s.inv.reset();
  for (std::vector<int>* v : {&s.off, &s.num, &s.cnt, &s.first, &s.goff, &s.gnum}) v->clear();
  s.built = s.typed = false;
  sets_drop_locations(s);
}

// d = the n elements at h, in an allocation of at least one element: copied on stream st or, without one, before the return.
// Every host array that a kernel reads goes up through here, into a buffer that frees itself.
template <class T>
hipError_t stage(DeviceBuf<T>& d, const T* h, size_t n, hipStream_t st = nullptr) {
  const hipError_t e = d.grow(n ? n : 1);
  if (e != hipSuccess) return e;
  if (st) return hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, st);
  return hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice);
}

template <int KD>
void launch_bank_build(hipStream_t st, size_t padded, bool f32, const void* src, const int3* dsets, int nsets, uint8_t* rows,
                       int* rfix, int* cfix) {
  const dim3 grid((unsigned)((padded + 1024 / KD - 1) / (1024 / KD)));
  if (f32)
    hipLaunchKernelGGL((bank_build_kernel<true, KD>), grid, dim3(256), 0, st, src, dsets, nsets, (int)padded, rows, rfix, cfix);
  else
    hipLaunchKernelGGL((bank_build_kernel<false, KD>), grid, dim3(256), 0, st, src, dsets, nsets, (int)padded, rows, rfix, cfix);
}

// `s` (cleared) from `src` (device memory, u8 or f32 [sum of counts][dim]): set k is counts[k] rows, of which the first
// max_sift are kept (SetDescriptors).  Returns after the sets are built.
int sets_build(hess_matcher* m, DescSets& s, int nsets, const int* counts, const void* src, bool f32) {
  const size_t KD = (size_t)m->dim;
  s.dim = m->dim;
  std::vector<int3> sets((size_t)nsets);
  std::vector<int> off((size_t)nsets), num((size_t)nsets), first((size_t)nsets), srow((size_t)nsets);
  size_t padded = 0;
  if (!set_layout(nsets, counts, m->max_sift, KD, off.data(), num.data(), first.data(), srow.data(), &padded)) {
    m->err = "bank too large";
    return HESS_ERR_TOO_BIG;
  }
  for (int k = 0; k < nsets; k++) sets[k] = make_int3(off[k], srow[k], num[k]);
  if (padded) {
    DeviceBuf<int3> dsets;
    M_TRY(m, s.rows.grow(padded * KD));
    M_TRY(m, s.rfix.grow(2 * padded));
    M_TRY(m, stage(dsets, sets.data(), sets.size(), m->st));
    if (m->dim == 128) launch_bank_build<128>(m->st, padded, f32, src, dsets.p, nsets, s.rows.p, s.rfix.p, s.cfix());
    else launch_bank_build<64>(m->st, padded, f32, src, dsets.p, nsets, s.rows.p, s.rfix.p, s.cfix());
    const hipError_t e = hipGetLastError(), es = hipStreamSynchronize(m->st);
    M_TRY(m, e);
    M_TRY(m, es);
  }
  s.off.swap(off);
  s.num.swap(num);
  s.first.swap(first);
  s.cnt.assign(counts, counts + nsets);
  s.built = true;
  return 0;
}

// `s` from host bytes: `rows` (the sum of counts) staged on the device, then sets_build.  On failure `s` is empty.
int sets_load(hess_matcher* m, DescSets& s, int nsets, const int* counts, const unsigned char* des, size_t rows) {
  sets_clear(s);
  DeviceBuf<uint8_t> staging;  // (stays empty for a bank without rows)
  if (rows) M_TRY(m, stage(staging, des, rows * (size_t)m->dim));
  const int rc = sets_build(m, s, nsets, counts, staging.p, false);
  if (rc) sets_clear(s);
  return rc;
}

template <int KD>
void launch_bank_gather(hipStream_t st, size_t padded, const DescSets& o, const int* src, uint8_t* rows, int* rfix, int* cfix) {
  const dim3 grid((unsigned)((padded + 4096 / KD - 1) / (4096 / KD)));
  hipLaunchKernelGGL(bank_gather_kernel<KD>, grid, dim3(256), 0, st, o.rows.p, o.rfix.p, o.cfix(), src, (int)padded, rows, rfix, cfix);
}

// Stores the rows of `s` grouped by the class of dev_types (device memory: one u16 per descriptor the caller counted,
// `stride` bytes apart), or back in the caller's order for dev_types == NULL.  The rows move from the present storage,
// typed or not; `s` changes only when everything succeeded.  Returns after the sets are ready.
int sets_regroup(hess_matcher* m, DescSets& s, const void* dev_types, size_t stride) {
  if (!dev_types && !s.typed) return 0;
  const int nsets = (int)s.num.size();
  const size_t KD = (size_t)s.dim;
  const size_t total = nsets ? (size_t)s.first[nsets - 1] + s.num[nsets - 1] : 0;
  std::vector<int> goff, gnum;
  size_t padded = 0;
  std::vector<TypeSet> tab((size_t)nsets);
  for (int k = 0; k < nsets; k++) tab[k] = TypeSet{s.first[k], s.off[k], {0, 0, 0, 0}};
  // what `s` will hold, built aside (fwd and inv stay empty without types), and what only this call needs: all of it is
  // freed on every way out, after the commit below the former with the buffers `s` held before
  DeviceBuf<uint8_t> rows;
  DeviceBuf<int> rfix, fwd, inv, pos, src, dcounts;
  DeviceBuf<int3> dsets;
  DeviceBuf<TypeSet> dtab;
  if (dev_types) {
    goff.assign((size_t)nsets * 4, 0);
    gnum.assign((size_t)nsets * 4, 0);
    if (total) {
      std::vector<int3> sets((size_t)nsets);
      size_t srow = 0;
      for (int k = 0; k < nsets; k++) {
        sets[k] = make_int3((int)srow, s.num[k], s.first[k]);
        srow += (size_t)s.cnt[k];
      }
      M_TRY(m, pos.grow(total));
      M_TRY(m, dcounts.grow((size_t)nsets * 4));
      M_TRY(m, stage(dsets, sets.data(), sets.size(), m->st));
      hipLaunchKernelGGL(type_classify_kernel, dim3(nsets), dim3(256), 0, m->st, static_cast<const uint8_t*>(dev_types), stride,
                         dsets.p, pos.p, dcounts.p);
      M_TRY(m, hipGetLastError());
      M_TRY(m, hipMemcpyAsync(gnum.data(), dcounts.p, gnum.size() * sizeof(int), hipMemcpyDeviceToHost, m->st));
      M_TRY(m, hipStreamSynchronize(m->st));
    }
    if (!group_layout(4 * nsets, gnum.data(), KD, goff.data(), &padded)) { m->err = "set_types: bank too large"; return HESS_ERR_TOO_BIG; }
    for (int k = 0; k < nsets; k++) memcpy(tab[k].grp, &goff[4 * k], sizeof(tab[k].grp));
  } else if (nsets) {
    padded = (size_t)s.off[nsets - 1] + pad_rows((size_t)s.num[nsets - 1]);
  }
  if (total) {  // (so there are sets and padded rows: no size below is zero)
    M_TRY(m, rows.grow(padded * KD));
    M_TRY(m, rfix.grow(2 * padded));
    M_TRY(m, src.grow(padded));
    M_TRY(m, hipMemsetAsync(src.p, 0xff, padded * sizeof(int), m->st));
    if (dev_types) {
      M_TRY(m, fwd.grow(total));
      M_TRY(m, inv.grow(padded));
      M_TRY(m, hipMemsetAsync(inv.p, 0xff, padded * sizeof(int), m->st));
    }
    M_TRY(m, stage(dtab, tab.data(), tab.size(), m->st));
    hipLaunchKernelGGL(type_place_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->st, dtab.p, nsets, (int)total,
                       pos.p, s.typed ? s.fwd.p : nullptr, fwd.p, inv.p, src.p);
    if (s.dim == 128) launch_bank_gather<128>(m->st, padded, s, src.p, rows.p, rfix.p, rfix.p + padded);
    else launch_bank_gather<64>(m->st, padded, s, src.p, rows.p, rfix.p, rfix.p + padded);
    M_TRY(m, hipGetLastError());
    M_TRY(m, hipStreamSynchronize(m->st));
    s.rows.swap(rows);  // the commit: nothing fails from here on
    s.rfix.swap(rfix);
  }
  s.fwd.swap(fwd);
  s.inv.swap(inv);
  s.typed = dev_types != nullptr;
  s.goff.swap(goff);
  s.gnum.swap(gnum);
  return 0;
}

// The strided host values of a types argument, packed and staged on the device, then sets_regroup.
int sets_types_host(hess_matcher* m, DescSets& s, const uint16_t* types, size_t stride) {
  if (!types) return sets_regroup(m, s, nullptr, 0);
  size_t n = 0;
  for (int c : s.cnt) n += (size_t)c;
  std::vector<uint16_t> h(n ? n : 1);
  for (size_t i = 0; i < n; i++) memcpy(&h[i], reinterpret_cast<const char*>(types) + i * stride, 2);
  DeviceBuf<uint16_t> d;
  M_TRY(m, stage(d, h.data(), h.size()));
  return sets_regroup(m, s, d.p, 2);
}

// What every types setter refuses: `what` names the entry point in the error text.
int types_args(hess_matcher* m, const DescSets& s, const void* types, size_t stride, const char* what) {
  if (!s.built) { m->err = std::string(what) + ": load the descriptors before their types"; return HESS_ERR_STATE; }
  if (types && (stride < 2 || stride % 2)) {
    m->err = std::string(what) + ": stride_bytes must be even and at least 2, not " + std::to_string(stride);
    return HESS_ERR_ARG;
  }
  return 0;
}

// The bank's locations from records in device memory (checked), `stride` bytes apart.
int bank_locations(hess_matcher* m, const void* dev, size_t stride) {
  DescSets& b = m->bank;
  const int nsets = (int)b.num.size();
  std::vector<int3> sets((size_t)nsets);
  size_t srow = 0, total = 0;
  for (int k = 0; k < nsets; k++) {
    sets[k] = make_int3(b.first[k], (int)srow, b.num[k]);
    srow += (size_t)b.cnt[k];
    total = (size_t)b.first[k] + (size_t)b.num[k];
  }
  DeviceBuf<float2> loc;  // built aside: a failure leaves the bank's present locations in place
  DeviceBuf<int3> dsets;
  if (total) {
    M_TRY(m, loc.grow(total));
    M_TRY(m, stage(dsets, sets.data(), sets.size(), m->st));
    hipLaunchKernelGGL(bank_loc_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->st,
                       static_cast<const unsigned char*>(dev), stride, dsets.p, nsets, (int)total, loc.p);
    const hipError_t e = hipGetLastError(), es = hipStreamSynchronize(m->st);
    M_TRY(m, e);
    M_TRY(m, es);
  }
  b.loc.swap(loc);
  b.have_loc = true;
  return 0;
}

// What both bank_set_locations forms refuse.  rows: the records the caller counted.
int bank_locations_args(hess_matcher* m, size_t stride, const char* what, size_t* rows) {
  if (!m->bank.built) {
    m->err = std::string(what) + ": load the bank's descriptors before their locations";
    return HESS_ERR_STATE;
  }
  if (stride < 8 || stride % 4) {
    m->err = std::string(what) + ": stride_bytes must be a multiple of 4 and at least 8, not " + std::to_string(stride);
    return HESS_ERR_ARG;
  }
  size_t n = 0;
  for (int c : m->bank.cnt) n += (size_t)c;
  *rows = n;
  return 0;
}

// Host floats quantised as the reference does, int(512*d + 0.5) into a byte (SiftMatchCU.cpp:88-100): set k is counts[k]
// rows of KD floats, of which the first max_sift (kept[k]) are kept.
std::vector<unsigned char> quantise(const float* des, size_t KD, int nsets, const int* counts, int max_sift, int* kept) {
  size_t nk = 0;
  for (int k = 0; k < nsets; k++) nk += (size_t)(kept[k] = counts[k] > max_sift ? max_sift : counts[k]);
  std::vector<unsigned char> q(nk * KD);
  size_t src = 0, dst = 0;
  for (int k = 0; k < nsets; k++) {
    for (size_t i = 0; i < (size_t)kept[k] * KD; ++i) q[dst + i] = (unsigned char)hess::desc_byte(des[src + i]);
    src += (size_t)counts[k] * KD;
    dst += (size_t)kept[k] * KD;
  }
  return q;
}

int bank_args(hess_matcher* m, int nsets, const int* counts, const void* des, size_t* rows) {
  if (!m) return HESS_ERR_ARG;
  if (nsets < 0 || (nsets > 0 && !counts)) { m->err = "bank: nsets < 0 or counts NULL"; return HESS_ERR_ARG; }
  size_t t = 0;
  for (int s = 0; s < nsets; s++) {
    if (counts[s] < 0) { m->err = "bank: negative count for set " + std::to_string(s); return HESS_ERR_ARG; }
    t += (size_t)counts[s];
  }
  if (t && !des) { m->err = "bank: descriptors NULL"; return HESS_ERR_ARG; }
  *rows = t;
  return 0;
}

// What every pair-list entry point refuses: `what` names it in the error text.
int pair_list_args(hess_matcher* m, int npairs, const int* pairs_ab, int max_match, const int* out_pairs, const int* out_counts,
                   const char* what) {
  if (npairs < 0 || max_match < 0 || (npairs > 0 && (!pairs_ab || !out_counts || (max_match > 0 && !out_pairs)))) {
    m->err = std::string(what) + ": npairs or max_match < 0, or an array is NULL";
    return HESS_ERR_ARG;
  }
  const int nsets = (int)m->bank.num.size();
  for (int p = 0; p < npairs; p++)
    if (pairs_ab[2 * p] < 0 || pairs_ab[2 * p] >= nsets || pairs_ab[2 * p + 1] < 0 || pairs_ab[2 * p + 1] >= nsets) {
      m->err = std::string(what) + ": pair " + std::to_string(p) + " names a set outside the bank of " + std::to_string(nsets);
      return HESS_ERR_ARG;
    }
  return 0;
}

// The events of the two pinned slots of a chunked pair list.
int slot_events(hess_matcher* m) {
  for (int k = 0; k < 2; k++)
    for (int q = 0; q < 3; q++)
      M_TRY(m, hess::ensure(m->mp_ev[k][q]));
  return 0;
}

// Grows the matcher's buffers to the scratch of a plan, plan_bytes of plan buffer and, for a pair list (out_bytes > 0), the
// output buffer with its two pinned slots and their events.
int grow_for(hess_matcher* m, const PlanNeed& n, size_t plan_bytes, size_t out_bytes) {
  M_TRY(m, m->mm_rstate.grow(n.rs));
  M_TRY(m, m->mm_cpart.grow(n.cp));
  M_TRY(m, m->rowm.grow(n.rm));
  M_TRY(m, m->colm.grow(n.cm));
  M_TRY(m, m->plan.grow(plan_bytes));
  M_TRY(m, m->hplan.grow(plan_bytes));
  if (!out_bytes) return 0;
  M_TRY(m, m->out.grow(out_bytes));
  M_TRY(m, m->hout.grow(out_bytes));
  return slot_events(m);
}

// The multiply and the finish of chunk c, whose plan buffer is at dplan on the device (run_chunk: m->plan;
// hess_matcher_verify_pairs launches both forms from one upload).  dgeo (guided pair lists only, else NULL): the device
// geometry of job 0 of the chunk onwards, and loc the bank's locations.
hipError_t launch_chunk(hess_matcher* m, const uint8_t* dplan, const DescSets& s1, const DescSets& s2, const Chunk& c,
                        int mutual_best, float distmax, float ratiomax, const GuidedGeo* dgeo, const float2* loc) {
  const PlanLayout L = plan_layout(c);
  if (c.nwg) {
    if (s1.dim != s2.dim || !dim_ok(s1.dim)) return hipErrorInvalidValue;  // (set_dim empties every set: not reached)
    const PairJob* djobs = plan_ptr<PairJob>(dplan, L.jobs);
    auto* const kern =
        dgeo ? (s1.dim == 128 ? (mutual_best ? match_mfma_kernel<true, 128, true> : match_mfma_kernel<false, 128, true>)
                              : (mutual_best ? match_mfma_kernel<true, 64, true> : match_mfma_kernel<false, 64, true>))
             : (s1.dim == 128 ? (mutual_best ? match_mfma_kernel<true, 128, false> : match_mfma_kernel<false, 128, false>)
                              : (mutual_best ? match_mfma_kernel<true, 64, false> : match_mfma_kernel<false, 64, false>));
    hipLaunchKernelGGL(kern, dim3((unsigned)c.nwg), dim3(256), 0, m->st, s1.rows.p, s1.rfix.p, s2.rows.p, s2.cfix(), djobs,
                       plan_ptr<int2>(dplan, L.work), m->mm_cpart.p, m->mm_rstate.p, dgeo, loc);
    hipLaunchKernelGGL(match_finish_kernel, dim3((unsigned)c.nfin), dim3(256), 0, m->st, djobs, plan_ptr<int2>(dplan, L.fin),
                       m->mm_rstate.p, m->mm_cpart.p, distmax, ratiomax, m->rowm.p, m->colm.p);
  }
  return hipGetLastError();
}

// Enqueues planned chunk c on m->st: its plan buffer (plan_fill) into the pinned slot hp and up to m->plan, then `start`,
// the multiply and the finish.  s1, s2: the sets the jobs' a, b index.  The caller has grown every buffer to c's size.
hipError_t run_chunk(hess_matcher* m, const DescSets& s1, const DescSets& s2, const PairJob* jobs, const Entry* orig,
                     const Chunk& c, uint8_t* hp, hipEvent_t start, int mutual_best, float distmax, float ratiomax,
                     const GuidedGeo* dgeo = nullptr, const float2* loc = nullptr) {
  plan_fill(hp, jobs, orig, c, mutual_best);
  const hipError_t e = hipMemcpyAsync(m->plan.p, hp, plan_layout(c).bytes, hipMemcpyHostToDevice, m->st);
  if (e != hipSuccess) return e;
  (void)hipEventRecord(start, m->st);
  return launch_chunk(m, m->plan.p, s1, s2, c, mutual_best, distmax, ratiomax, dgeo, loc);
}

// One pair-list call of n units through the two pinned slots (hess_slot_pipeline.h: unit k is enqueued into slot k & 1 and its
// results are read on the host while unit k + 1 runs).  enqueue(k, slot, &bytes) puts unit k's upload and launches on m->st,
// records the slot's first event behind the upload and says how many bytes of m->out are its results; deliver(k, h) hands
// unit k to the caller from its pinned copy h.  Here: the second event and the copy down behind every unit, the wait before
// its delivery, m->last_ms as the sum of the units' kernel intervals (first to second event) and, after a device error, the
// stream synchronised and `what`, the entry point's name, in front of the error's text.
template <class Enqueue, class Deliver>
int run_slots(hess_matcher* m, size_t n, const char* what, Enqueue&& enqueue, Deliver&& deliver) {
  // A list of one unit (the typed single pair) waits for the stream and records no third event: the event after the copy
  // and the wait for it cost 7 us per call, a tenth of that pair's wall time.  Behind the last of several units the
  // stream wait is the slower one (profiles/r19_matcher_plan.txt).
  const bool one_unit = n == 1;
  float total_ms = 0.0f;
  const hipError_t err = hess::slot_pipeline(
      n, hipSuccess,
      [&](size_t k, int slot) -> hipError_t {
        size_t bytes = 0;
        hipError_t e = enqueue(k, slot, &bytes);
        if (e != hipSuccess) return e;
        (void)hipEventRecord(m->mp_ev[slot][1], m->st);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(m->hout.p[slot], m->out.p, bytes, hipMemcpyDeviceToHost, m->st);
        if (e == hipSuccess && !one_unit) (void)hipEventRecord(m->mp_ev[slot][2], m->st);
        return e;
      },
      [&](size_t k, int slot) -> hipError_t {
        hipError_t e = one_unit ? hipStreamSynchronize(m->st) : hipEventSynchronize(m->mp_ev[slot][2]);
        if (e != hipSuccess) return e;
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, m->mp_ev[slot][0], m->mp_ev[slot][1]);
        if (e != hipSuccess) return e;
        total_ms += ms;
        deliver(k, m->hout.p[slot]);
        return hipSuccess;
      });
  if (err != hipSuccess) {
    (void)hipStreamSynchronize(m->st);
    m->err = std::string(what) + ": " + hipGetErrorString(err);
    return HESS_ERR_DEVICE;
  }
  m->last_ms = total_ms;
  return 0;
}

// Plans the pair list pairs_ab of sets s1 x s2 (plan_pairs), runs it chunk by chunk (run_slots) and delivers every pair's
// matches compacted on the device: out_counts[p] and out_pairs[p][max_match][2] (in the pinned slot the pairs are P.mm
// apart).  m->last_ms covers multiply, finish and compaction.  `what` names the entry point in the text of an error.
// geo (with loc, the locations both sets' `first` index; untyped sets): the guided match, pair p gated by geo[p] -- the table
// goes up once, before the first chunk, and chunk k's launch reads it from its first pair on.
int run_pairs(hess_matcher* m, const DescSets& s1, const DescSets& s2, int npairs, const int* pairs_ab, int max_match,
              int* out_pairs, int* out_counts, float distmax, float ratiomax, int mutual_best, const char* what,
              const hess_guided_pair* geo = nullptr, const float2* loc = nullptr) {
  PairPlan P;
  if (!plan_pairs(s1.layout(), s2.layout(), npairs, pairs_ab, max_match, mutual_best, P)) {
    m->err = std::string(what) + ": a pair needs more scratch than one launch can address";
    return HESS_ERR_TOO_BIG;
  }
  if (const int rc = grow_for(m, P.need, P.need.plan_bytes, P.need.outn * sizeof(int))) return rc;
  if (geo) {
    std::vector<GuidedGeo> h((size_t)npairs);
    for (int p = 0; p < npairs; p++) {
      GuidedGeo& g = h[p];
      memcpy(g.H, geo[p].H, sizeof(g.H));
      memcpy(g.F, geo[p].F, sizeof(g.F));
      bool finite = true;
      for (int k = 0; k < 9; k++) finite = finite && std::isfinite(g.H[k]) && std::isfinite(g.F[k]);
      if (!finite) { memset(g.H, 0, sizeof(g.H)); memset(g.F, 0, sizeof(g.F)); }
      g.hdistmax = geo[p].hdistmax;
      g.fdistmax = geo[p].fdistmax;
      g.la = s1.first[pairs_ab[2 * p]];
      g.lb = s2.first[pairs_ab[2 * p + 1]];
    }
    M_TRY(m, m->geo.grow((size_t)npairs));
    M_TRY(m, hipMemcpy(m->geo.p, h.data(), h.size() * sizeof(GuidedGeo), hipMemcpyHostToDevice));  // (complete on return)
  }
  const int mm = P.mm;
  int* const dout = reinterpret_cast<int*>(m->out.p);
  return run_slots(
      m, P.chunks.size(), what,
      [&](size_t k, int slot, size_t* bytes) -> hipError_t {
        const Chunk& c = P.chunks[k];
        const PlanLayout L = plan_layout(c);
        const hipError_t e = run_chunk(m, s1, s2, P.jobs.data(), P.orig.data(), c, m->hplan.p[slot], m->mp_ev[slot][0], mutual_best,
                                       distmax, ratiomax, geo ? m->geo.p + c.p0 : nullptr, loc);
        if (e != hipSuccess) return e;
        if (P.jpp == 4)
          hipLaunchKernelGGL(match_types_compact_kernel, dim3(c.pairs()), dim3(256), 0, m->st, plan_ptr<PairJob>(m->plan.p, L.jobs),
                             plan_ptr<int2>(m->plan.p, L.orig), s1.fwd.p, s2.inv.p, m->rowm.p, m->colm.p, mutual_best, mm, dout,
                             dout + MP_PAIRS);
        else
          hipLaunchKernelGGL(match_pairs_compact_kernel, dim3(c.pairs()), dim3(256), 0, m->st, plan_ptr<PairJob>(m->plan.p, L.jobs),
                             m->rowm.p, m->colm.p, mutual_best, mm, dout, dout + MP_PAIRS);
        *bytes = (MP_PAIRS + (size_t)c.pairs() * mm * 2) * sizeof(int);
        return hipSuccess;
      },
      [&](size_t k, const uint8_t* slot_bytes) {
        const Chunk& c = P.chunks[k];
        const int* h = reinterpret_cast<const int*>(slot_bytes);
        const int q0 = c.p0 / c.jpp, q1 = c.p1 / c.jpp;
        for (int p = q0; p < q1; p++) {
          const int n = h[p - q0];
          out_counts[p] = n;
          if (n) memcpy(out_pairs + (size_t)p * max_match * 2, h + MP_PAIRS + (size_t)(p - q0) * mm * 2, (size_t)n * 2 * sizeof(int));
        }
      });
}

// hess_matcher_verify_pairs works on GROUPS of up to VP_GROUP consecutive chunks of the pair plan: the matcher's kernels run
// chunk by chunk (MP_PAIRS pairs: the plan's unit), the estimator's once per group.  Its refit kernel is one workgroup per
// pair with a serial solve, 0.27 ms a launch whether it has 64 pairs or 256, and its score kernel fills the device only from
// a few hundred pairs on (profiles/r22_verify_pairs.txt): a group is what one chunk of hess_matcher_estimate_pairs holds.
constexpr int VP_GROUP = 4, VP_PAIRS = VP_GROUP * MP_PAIRS;

// Where a group's results sit in m->out and in its pinned slot.  A head of fixed size (the counts of both matches and the
// results of both estimates, VP_PAIRS entries each), the guided matches, then the mask of the final estimate and the
// putative matches where the caller takes them: [0, copy) is what one copy brings down.  The sections the caller does not
// take, and the putative estimate's mask, lie behind it.  Matches and masks are mm per pair.
struct VerifyLayout { size_t cnt1, cnt2, res1, res2, guided, mask2, put, mask1, copy, bytes; };
VerifyLayout verify_layout(int np, int mm, bool want_mask, bool want_put) {
  const size_t prs = (size_t)np * mm * 2 * sizeof(int), mk = ((size_t)np * mm + 15) / 16 * 16;
  VerifyLayout L;
  L.cnt1 = 0;
  L.cnt2 = VP_PAIRS * sizeof(int);
  L.res1 = 2 * VP_PAIRS * sizeof(int);
  L.res2 = L.res1 + VP_PAIRS * sizeof(hess_geom_result);
  size_t o = L.res2 + VP_PAIRS * sizeof(hess_geom_result);
  static_assert((2 * VP_PAIRS * sizeof(int) + 2 * VP_PAIRS * sizeof(hess_geom_result)) % 16 == 0, "the matches are read as int2");
  L.guided = o; o += prs;
  if (want_mask) { L.mask2 = o; o += mk; }
  if (want_put) { L.put = o; o += prs; }
  L.copy = o;
  if (!want_mask) { L.mask2 = o; o += mk; }
  if (!want_put) { L.put = o; o += prs; }
  L.mask1 = o;
  L.bytes = o + mk;
  return L;
}

// The chain of hess_abi.h at hess_matcher_verify_pairs, per group of chunks of the pair plan in stream order: the plan
// buffers of the group's chunks up; per chunk the unguided multiply, finish and compaction; the estimate on the group's
// matches (hess_geom_enqueue: counts and matches stay on the device); the group's guided geometry (verify_geo_kernel); per
// chunk the guided multiply, finish and compaction from the SAME plan buffer and scratch (the first compaction has consumed
// the decisions); optionally the estimate again; one copy into the pinned slot g & 1, read while group g + 1 runs
// (run_slots).  Arguments are checked and nothing has been launched.
int run_verify(hess_matcher* m, int npairs, const int* pairs_ab, const hess_verify_params& V, int max_match, int* out_pairs,
               int* out_counts, hess_verify_result* out, unsigned char* inlier, int* putative_pairs, const float2* loc) {
  const char* const what = "verify_pairs";
  const DescSets& S = m->bank;
  const int mutual_best = V.mutual_best ? 1 : 0;
  const bool fin = V.final_estimate != 0, want_mask = fin && inlier, want_put = putative_pairs != nullptr;
  PairPlan P;
  if (!plan_pairs(S.layout(), S.layout(), npairs, pairs_ab, max_match, mutual_best, P)) {
    m->err = std::string(what) + ": a pair needs more scratch than one launch can address";
    return HESS_ERR_TOO_BIG;
  }
  const int mm = P.mm;
  // group g: chunks [VP_GROUP g, VP_GROUP g + VP_GROUP) of the plan, pairs [first pair of its first chunk, last of its last)
  const size_t nchunks = P.chunks.size(), ngroups = (nchunks + VP_GROUP - 1) / VP_GROUP;
  auto group_first = [&](size_t g) { return P.chunks[g * VP_GROUP].p0; };
  auto group_end = [&](size_t g) { return P.chunks[std::min(nchunks, (g + 1) * VP_GROUP) - 1].p1; };
  int npmax = 0;
  for (size_t g = 0; g < ngroups; g++) npmax = std::max(npmax, group_end(g) - group_first(g));
  if ((size_t)npmax * mm > (size_t)INT_MAX) {  // (the estimator's jobs index a group's matches with an int)
    m->err = std::string(what) + ": " + std::to_string(npmax) + " pairs of up to " + std::to_string(mm) + " matches are more than one launch can address";
    return HESS_ERR_TOO_BIG;
  }
  const size_t pstride = (P.need.plan_bytes + 63) / 64 * 64;  // a chunk's plan buffer within the group's
  if (const int rc = grow_for(m, P.need, VP_GROUP * pstride, verify_layout(npmax, mm, want_mask, want_put).bytes)) return rc;
  M_TRY(m, m->geo.grow((size_t)VP_PAIRS));
  M_TRY(m, m->vp_lalb.grow((size_t)npairs));
  if (const int rc = hess_geom_reserve(m, V.geom, npmax, mm)) return rc;
  std::vector<int2> lalb((size_t)npairs);  // (alive until the stream has been waited for: every return below)
  for (int p = 0; p < npairs; p++) lalb[p] = make_int2(S.first[pairs_ab[2 * p]], S.first[pairs_ab[2 * p + 1]]);
  M_TRY(m, hipMemcpyAsync(m->vp_lalb.p, lalb.data(), lalb.size() * sizeof(int2), hipMemcpyHostToDevice, m->st));
  if (inlier) memset(inlier, 0, (size_t)npairs * max_match);
  const float gbound = V.guided_bound != 0.0f ? V.guided_bound : V.geom.bound;
  hess_geom_result none;
  memset(&none, 0, sizeof(none));
  none.hypothesis = -1;
  uint8_t* const d = m->out.p;
  // The two matches of the group's chunk k from its plan buffer: multiply and finish (guided with dgeo), then the compaction
  // to the chunk's place (its first pair's offset in the group) in the count words at `cnt` and the lists at `lists`.
  auto match_chunk = [&](size_t k, int p0, size_t cnt, size_t lists, const GuidedGeo* dgeo) -> hipError_t {
    const Chunk& c = P.chunks[k];
    const uint8_t* const dplan = m->plan.p + (k % VP_GROUP) * pstride;
    const int q0 = c.p0 - p0;
    const hipError_t e = launch_chunk(m, dplan, S, S, c, mutual_best, V.distmax, V.ratiomax, dgeo ? dgeo + q0 : nullptr, loc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(match_pairs_compact_kernel, dim3(c.pairs()), dim3(256), 0, m->st, plan_ptr<PairJob>(dplan, plan_layout(c).jobs),
                       m->rowm.p, m->colm.p, mutual_best, mm, reinterpret_cast<int*>(d + cnt) + q0,
                       reinterpret_cast<int*>(d + lists) + (size_t)q0 * mm * 2);
    return hipGetLastError();
  };
  return run_slots(
      m, ngroups, what,
      [&](size_t g, int slot, size_t* bytes) -> hipError_t {
        const size_t k0 = g * VP_GROUP, k1 = std::min(nchunks, k0 + VP_GROUP);
        const int p0 = group_first(g), np = group_end(g) - p0;
        const VerifyLayout L = verify_layout(np, mm, want_mask, want_put);
        uint8_t* const hp = m->hplan.p[slot];
        hess_geom_device_pairs E{np, mm, m->vp_lalb.p + p0, reinterpret_cast<const int*>(d + L.cnt1), reinterpret_cast<const int2*>(d + L.put),
                                 V.geom.seed + (uint32_t)p0, reinterpret_cast<hess_geom_result*>(d + L.res1), d + L.mask1};
        for (size_t k = k0; k < k1; k++) plan_fill(hp + (k - k0) * pstride, P.jobs.data(), nullptr, P.chunks[k], mutual_best);
        hipError_t err = hipMemcpyAsync(m->plan.p, hp, (k1 - k0 - 1) * pstride + plan_layout(P.chunks[k1 - 1]).bytes, hipMemcpyHostToDevice, m->st);
        if (err != hipSuccess) return err;
        (void)hipEventRecord(m->mp_ev[slot][0], m->st);
        for (size_t k = k0; k < k1 && err == hipSuccess; k++) err = match_chunk(k, p0, L.cnt1, L.put, nullptr);
        if (err != hipSuccess) return err;
        err = hess_geom_enqueue(m, V.geom, E);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL(verify_geo_kernel, dim3((np + 63) / 64), dim3(64), 0, m->st, E.results, E.lalb, np,
                           V.geom.model == HESS_GEOM_HOMOGRAPHY ? 1 : 0, gbound, m->geo.p);
        for (size_t k = k0; k < k1 && err == hipSuccess; k++) err = match_chunk(k, p0, L.cnt2, L.guided, m->geo.p);
        if (err != hipSuccess) return err;
        if (fin) {
          E.counts = reinterpret_cast<const int*>(d + L.cnt2);
          E.matches = reinterpret_cast<const int2*>(d + L.guided);
          E.results = reinterpret_cast<hess_geom_result*>(d + L.res2);
          E.mask = d + L.mask2;
          err = hess_geom_enqueue(m, V.geom, E);
        }
        *bytes = L.copy;
        return err;
      },
      [&](size_t g, const uint8_t* h) {
        const int p0 = group_first(g), np = group_end(g) - p0;
        const VerifyLayout L = verify_layout(np, mm, want_mask, want_put);
        const int* n1 = reinterpret_cast<const int*>(h + L.cnt1);
        const int* n2 = reinterpret_cast<const int*>(h + L.cnt2);
        for (int q = 0; q < np; q++) {
          const size_t p = (size_t)p0 + q;
          hess_verify_result& R = out[p];
          memset(&R, 0, sizeof(R));
          memcpy(&R.putative, h + L.res1 + q * sizeof(hess_geom_result), sizeof(hess_geom_result));
          if (fin) memcpy(&R.final, h + L.res2 + q * sizeof(hess_geom_result), sizeof(hess_geom_result));
          else R.final = none;
          R.nputative = n1[q];
          R.nguided = out_counts[p] = n2[q];
          if (n2[q]) memcpy(out_pairs + p * max_match * 2, h + L.guided + (size_t)q * mm * 2 * sizeof(int), (size_t)n2[q] * 2 * sizeof(int));
          if (want_mask && n2[q]) memcpy(inlier + p * max_match, h + L.mask2 + (size_t)q * mm, (size_t)n2[q]);
          if (want_put && n1[q])
            memcpy(putative_pairs + p * max_match * 2, h + L.put + (size_t)q * mm * 2 * sizeof(int), (size_t)n1[q] * 2 * sizeof(int));
        }
      });
}

// The small unguided and the guided single pair, from m->e0 on: the score matrix (match_dot_kernel, gates per pair), the row
// decisions and, for mutual best, the column decisions.
int match_small(hess_matcher* m, int n1, int n2, const float* H, const float* F, float distmax, float ratiomax,
                float hdistmax, float fdistmax, int mutual_best) {
  M_TRY(m, m->rowm.grow((size_t)n1));
  M_TRY(m, m->colm.grow((size_t)n2));
  const size_t need = (size_t)n1 * n2;
  if (need > m->dotm.cap) {  // the column partials go with the matrix: for max_sift rows and columns, whatever the pair has
    m->cpart.reset();
    m->dotm.reset();
    M_TRY(m, m->cpart.grow((size_t)((m->max_sift + TM - 1) / TM + 1) * m->max_sift));
    M_TRY(m, m->dotm.grow(need));
  }
  GeoParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.guided = H ? 1 : 0;
  if (gp.guided) { memcpy(gp.H, H, 36); memcpy(gp.F, F, 36); gp.hdistmax = hdistmax; gp.fdistmax = fdistmax; }
  (void)hipEventRecord(m->e0, m->st);
  hipLaunchKernelGGL(m->dim == 128 ? match_dot_kernel<128> : match_dot_kernel<64>, dim3((n2 + TN - 1) / TN, (n1 + TM - 1) / TM),
                     dim3(256), 0, m->st, m->slot[0].rows.p, n1, m->slot[1].rows.p, n2, m->slot[0].loc.p, m->slot[1].loc.p, gp,
                     mutual_best ? m->cpart.p : nullptr, m->dotm.p);
  hipLaunchKernelGGL(match_row_kernel, dim3((n1 + 3) / 4), dim3(256), 0, m->st, m->dotm.p, n1, n2, distmax, ratiomax,
                     m->rowm.p);
  if (mutual_best)
    hipLaunchKernelGGL(match_col_kernel, dim3((n2 + 31) / 32), dim3(256), 0, m->st, m->cpart.p, (n1 + TM - 1) / TM, n2,
                       distmax, ratiomax, m->colm.p);
  return 0;
}

}  // namespace

extern "C" {

hess_matcher* hess_matcher_create(int device, int max_sift) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fprintf(stderr, "hessgpu: no usable HIP device %d (found %d)\n", device, ndev);
    return nullptr;
  }
  std::unique_ptr<hess_matcher> m(new (std::nothrow) hess_matcher());
  if (m && hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&m->st.h, hipStreamNonBlocking) == hipSuccess) {
    m->device = device;
    m->max_sift = max_sift > 0 ? max_sift : 4096;
    (void)hess::ensure(m->e0);
    (void)hess::ensure(m->e1);
  } else {
    m.reset();
  }
  return m.release();
}

void hess_matcher_destroy(hess_matcher* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;  // (members in reverse order: every buffer, then the events and the stream)
}

int hess_matcher_set_max(hess_matcher* m, int max_sift) {
  if (!m || max_sift <= 0) return HESS_ERR_ARG;
  m->max_sift = max_sift;
  return 0;
}

// Descriptor length of every set and descriptor argument: 128 (a new matcher) or 64.  A change empties the bank, the two
// single-pair slots and their locations: their rows have the other pitch.
int hess_matcher_set_dim(hess_matcher* m, int dim) {
  if (!m) return HESS_ERR_ARG;
  if (!dim_ok(dim)) {
    m->err = "set_dim: descriptors are 128-d or 64-d, not " + std::to_string(dim) + "-d";
    return HESS_ERR_ARG;
  }
  if (dim == m->dim) return 0;
  M_TRY(m, hipSetDevice(m->device));
  M_TRY(m, hipStreamSynchronize(m->st));
  sets_clear(m->bank);
  for (int k = 0; k < 2; k++) sets_clear(m->slot[k]);
  m->dim = dim;
  return 0;
}

int hess_matcher_dim(hess_matcher* m) { return m ? m->dim : HESS_ERR_ARG; }

// SiftMatchCU::SetDescriptors(index, num, const unsigned char*), SiftMatchCU.cpp:71-85: slot `index` becomes a one-set bank.
int hess_matcher_set_descriptors(hess_matcher* m, int index, int num, const unsigned char* des) {
  if (!m || !des || num < 0) return HESS_ERR_ARG;
  index = index > 1 ? 1 : (index < 0 ? 0 : index);
  M_TRY(m, hipSetDevice(m->device));
  if (num > m->max_sift) num = m->max_sift;
  return sets_load(m, m->slot[index], 1, &num, des, (size_t)num);
}

// Float descriptors are quantised as the reference does (SiftMatchCU.cpp:88-100).
int hess_matcher_set_descriptors_f32(hess_matcher* m, int index, int num, const float* des) {
  if (!m || !des || num < 0) return HESS_ERR_ARG;
  int kept = 0;
  std::vector<unsigned char> q = quantise(des, (size_t)m->dim, 1, &num, m->max_sift, &kept);
  return hess_matcher_set_descriptors(m, index, kept, q.data());
}

// SiftMatchCU::SetFeautreLocation, SiftMatchCU.cpp:103-123: (x, y) pairs, `gap` floats skipped after each.
int hess_matcher_set_locations(hess_matcher* m, int index, const float* locations, int gap) {
  if (!m || !locations || index < 0 || index > 1) return HESS_ERR_ARG;
  DescSets& s = m->slot[index];
  const int n = s.count(0);
  if (n <= 0) return 0;
  M_TRY(m, hipSetDevice(m->device));
  std::vector<float2> h((size_t)n);
  for (int i = 0; i < n; i++) { h[i].x = locations[0]; h[i].y = locations[1]; locations += 2 + gap; }
  sets_drop_locations(s);
  M_TRY(m, stage(s.loc, h.data(), h.size()));
  s.have_loc = true;
  return 0;
}

// SiftMatchCU::GetSiftMatch / GetGuidedSiftMatch + GetBestMatch (SiftMatchCU.cpp:125-173).
// H, F: 3x3 row-major, both NULL for the unguided match.  Returns the number of matches (>= 0) or a
// negative hess_status.
int hess_matcher_match(hess_matcher* m, int max_match, int* pairs, const float* H, const float* F, float distmax,
                       float ratiomax, float hdistmax, float fdistmax, int mutual_best) {
  if (!m || !pairs || max_match < 0) return HESS_ERR_ARG;
  const int n1 = m->slot[0].count(0), n2 = m->slot[1].count(0);
  const bool guided = (H != nullptr) || (F != nullptr);
  const bool typed = m->slot[0].typed && m->slot[1].typed;
  if (guided && (m->slot[0].typed || m->slot[1].typed)) {
    m->err = "match: guided matching (H, F) with feature types is not built; remove the types (set_types NULL) first";
    return HESS_ERR_UNSUPPORTED;
  }
  if (m->slot[0].typed != m->slot[1].typed) {
    m->err = std::string("match: slot ") + (m->slot[0].typed ? "1" : "0") + " has no types and the other has (set_types both, or NULL both)";
    return HESS_ERR_STATE;
  }
  if (n1 <= 0 || n2 <= 0) return 0;
  if (guided && (!H || !F)) { m->err = "guided matching needs both H and F"; return HESS_ERR_ARG; }
  if (guided && (!m->slot[0].have_loc || !m->slot[1].have_loc)) return 0;  // SiftMatchCU.cpp:131
  M_TRY(m, hipSetDevice(m->device));
  if (typed) {
    // the gated pair: a list of one through the job tables at any size (bank pairs take them below the switch too), compacted
    // on the device in original row order
    const int ab[2] = {0, 0};
    int nmatch = 0;
    const int rc = run_pairs(m, m->slot[0], m->slot[1], 1, ab, max_match, pairs, &nmatch, distmax, ratiomax, mutual_best ? 1 : 0, "match");
    return rc ? rc : nmatch;
  }
  if (!guided && (size_t)n1 * n2 > MM_SINGLE_ABOVE) {
    // matrix cores, the pair as a chunk of one job with the segments of single_sps
    PairJob job{0, 0, n1, n2};
    Chunk c{0, 1, single_sps(n1, n2), 0, 0, 0, 0, 0, 0, 1};
    plan_chunk(&job, c, mutual_best);
    if (const int rc = grow_for(m, PlanNeed{c.rs, c.cp, c.rm, c.cm, 0, 0}, plan_layout(c).bytes, 0)) return rc;  // (0: compacted on the host, below)
    M_TRY(m, run_chunk(m, m->slot[0], m->slot[1], &job, nullptr, c, m->hplan.p[0], m->e0, mutual_best, distmax, ratiomax));
  } else if (const int rc = match_small(m, n1, n2, H, F, distmax, ratiomax, hdistmax, fdistmax, mutual_best)) {
    return rc;
  }
  (void)hipEventRecord(m->e1, m->st);
  m->hrow.resize(n1);
  m->hcol.resize(n2);
  M_TRY(m, hipMemcpyAsync(m->hrow.data(), m->rowm.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, m->st));
  if (mutual_best) M_TRY(m, hipMemcpyAsync(m->hcol.data(), m->colm.p, (size_t)n2 * 4, hipMemcpyDeviceToHost, m->st));
  M_TRY(m, hipStreamSynchronize(m->st));
  (void)hipEventElapsedTime(&m->last_ms, m->e0, m->e1);
  int nmatch = 0;
  for (int i = 0; i < n1 && nmatch < max_match; ++i) {
    const int j = m->hrow[i];
    if (j >= 0 && (!mutual_best || m->hcol[j] == i)) {
      pairs[2 * nmatch] = i;
      pairs[2 * nmatch + 1] = j;
      nmatch++;
    }
  }
  return nmatch;
}

// ---- bank of descriptor sets, many pairs per call --------------------------------------------------------------------

int hess_matcher_bank_set(hess_matcher* m, int nsets, const int* counts, const unsigned char* des) {
  size_t rows = 0;
  if (const int rc = bank_args(m, nsets, counts, des, &rows)) return rc;
  M_TRY(m, hipSetDevice(m->device));
  return sets_load(m, m->bank, nsets, counts, des, rows);
}

// Host floats: quantised on the host as hess_matcher_set_descriptors_f32 does, then the byte path.
int hess_matcher_bank_set_f32(hess_matcher* m, int nsets, const int* counts, const float* des) {
  size_t rows = 0;
  if (const int rc = bank_args(m, nsets, counts, des, &rows)) return rc;
  std::vector<int> kept((size_t)nsets);
  std::vector<unsigned char> q = quantise(des, (size_t)m->dim, nsets, counts, m->max_sift, kept.data());
  const int rc = hess_matcher_bank_set(m, nsets, kept.data(), q.empty() ? nullptr : q.data());
  if (rc == 0) m->bank.cnt.assign(counts, counts + nsets);  // (types are indexed as the caller counted)
  return rc;
}

// `bytes` from p on must be device memory of the matcher's device and lie within one allocation: HESS_ERR_ARG otherwise.
static int device_range(hess_matcher* m, const void* p, size_t bytes, const char* what, const char* noun) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != m->device) {
    (void)hipGetLastError();
    m->err = std::string(what) + ": the " + noun + " are not device memory of device " + std::to_string(m->device);
    return HESS_ERR_ARG;
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess ||
      (const char*)p + bytes > (const char*)base + size) {
    (void)hipGetLastError();
    m->err = std::string(what) + ": the counts reach past the end of the " + noun + "' allocation";
    return HESS_ERR_ARG;
  }
  (void)hipGetLastError();
  return 0;
}

// The bank from descriptors in device memory, float (quantised by bank_build_kernel<true>) or bytes (<false>: stored as they
// are).  Everything about the pointer is checked before anything is launched.
static int bank_set_device(hess_matcher* m, int nsets, const int* counts, const void* dev_desc, bool f32) {
  size_t rows = 0;
  if (const int rc = bank_args(m, nsets, counts, dev_desc, &rows)) return rc;
  M_TRY(m, hipSetDevice(m->device));
  if (rows) {
    const size_t align = f32 ? 16 : 4, esz = f32 ? sizeof(float) : 1;  // what one lane of bank_build_kernel loads
    if ((uintptr_t)dev_desc % align) {
      m->err = "bank_set_device: the descriptors must be " + std::to_string(align) + "-byte aligned";
      return HESS_ERR_ARG;
    }
    if (const int rc = device_range(m, dev_desc, rows * (size_t)m->dim * esz, "bank_set_device", "descriptors")) return rc;
  }
  sets_clear(m->bank);
  const int rc = sets_build(m, m->bank, nsets, counts, dev_desc, f32);
  if (rc) sets_clear(m->bank);
  return rc;
}

int hess_matcher_bank_set_device(hess_matcher* m, int nsets, const int* counts, const float* dev_desc) {
  return bank_set_device(m, nsets, counts, dev_desc, true);
}

int hess_matcher_bank_set_device_u8(hess_matcher* m, int nsets, const int* counts, const unsigned char* dev_desc) {
  return bank_set_device(m, nsets, counts, dev_desc, false);
}

int hess_matcher_bank_read(hess_matcher* m, int set, unsigned char* out) {
  if (!m) return HESS_ERR_ARG;
  if (set < 0 || set >= (int)m->bank.num.size()) {
    m->err = "bank_read: no set " + std::to_string(set) + " in a bank of " + std::to_string(m->bank.num.size());
    return HESS_ERR_ARG;
  }
  const int n = m->bank.num[set];
  if (out && n) {
    M_TRY(m, hipSetDevice(m->device));
    const size_t KD = (size_t)m->bank.dim;
    if (m->bank.typed) {  // the set's four class groups, then the caller's order through fwd
      const int g0 = m->bank.goff[4 * set];
      size_t ext = 0;
      for (int c = 0; c < 4; c++) ext += pad_rows((size_t)m->bank.gnum[4 * set + c]);
      std::vector<unsigned char> grp(ext * KD);
      std::vector<int> fwd((size_t)n);
      M_TRY(m, hipMemcpy(grp.data(), m->bank.rows.p + (size_t)g0 * KD, ext * KD, hipMemcpyDeviceToHost));
      M_TRY(m, hipMemcpy(fwd.data(), m->bank.fwd.p + m->bank.first[set], (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; i++) memcpy(out + (size_t)i * KD, grp.data() + (size_t)(fwd[i] - g0) * KD, KD);
    } else {
      M_TRY(m, hipMemcpy(out, m->bank.rows.p + (size_t)m->bank.off[set] * KD, (size_t)n * KD, hipMemcpyDeviceToHost));
    }
  }
  return n;
}

// ---- feature types: see the comment at type_classify_kernel ----------------------------------------------------------

int hess_matcher_set_types(hess_matcher* m, int index, const uint16_t* types, size_t stride_bytes) {
  if (!m) return HESS_ERR_ARG;
  if (index < 0 || index > 1) { m->err = "set_types: index must be 0 or 1, not " + std::to_string(index); return HESS_ERR_ARG; }
  if (const int rc = types_args(m, m->slot[index], types, stride_bytes, "set_types")) return rc;
  M_TRY(m, hipSetDevice(m->device));
  return sets_types_host(m, m->slot[index], types, stride_bytes);
}

int hess_matcher_bank_set_types(hess_matcher* m, const uint16_t* types, size_t stride_bytes) {
  if (!m) return HESS_ERR_ARG;
  if (const int rc = types_args(m, m->bank, types, stride_bytes, "bank_set_types")) return rc;
  M_TRY(m, hipSetDevice(m->device));
  return sets_types_host(m, m->bank, types, stride_bytes);
}

int hess_matcher_bank_set_types_device(hess_matcher* m, const void* dev_types, size_t stride_bytes) {
  if (!m) return HESS_ERR_ARG;
  if (const int rc = types_args(m, m->bank, dev_types, stride_bytes, "bank_set_types_device")) return rc;
  M_TRY(m, hipSetDevice(m->device));
  size_t rows = 0;
  for (int c : m->bank.cnt) rows += (size_t)c;
  if (dev_types && rows) {
    if ((uintptr_t)dev_types % 2) { m->err = "bank_set_types_device: dev_types must be 2-byte aligned"; return HESS_ERR_ARG; }
    if (const int rc = device_range(m, dev_types, (rows - 1) * stride_bytes + 2, "bank_set_types_device", "types")) return rc;
  }
  return sets_regroup(m, m->bank, dev_types, stride_bytes);
}

// ---- the bank's locations, for guided pair lists and the estimator: they stay with the bank's descriptors -------------

int hess_matcher_bank_set_locations(hess_matcher* m, const float* loc, size_t stride_bytes) {
  if (!m) return HESS_ERR_ARG;
  if (!loc) { sets_drop_locations(m->bank); return 0; }
  size_t rows = 0;
  if (const int rc = bank_locations_args(m, stride_bytes, "bank_set_locations", &rows)) return rc;
  M_TRY(m, hipSetDevice(m->device));
  // the (x, y) pairs packed on the host, staged on the device, then the device form's gather
  std::vector<float2> h(rows ? rows : 1);
  for (size_t i = 0; i < rows; i++) memcpy(&h[i], reinterpret_cast<const char*>(loc) + i * stride_bytes, sizeof(float2));
  DeviceBuf<float2> d;
  M_TRY(m, stage(d, h.data(), h.size()));
  return bank_locations(m, d.p, sizeof(float2));
}

int hess_matcher_bank_set_locations_device(hess_matcher* m, const void* dev_loc, size_t stride_bytes) {
  if (!m) return HESS_ERR_ARG;
  if (!dev_loc) { sets_drop_locations(m->bank); return 0; }
  size_t rows = 0;
  if (const int rc = bank_locations_args(m, stride_bytes, "bank_set_locations_device", &rows)) return rc;
  M_TRY(m, hipSetDevice(m->device));
  if (rows) {
    if ((uintptr_t)dev_loc % 4) { m->err = "bank_set_locations_device: dev_loc must be 4-byte aligned"; return HESS_ERR_ARG; }
    if (const int rc = device_range(m, dev_loc, (rows - 1) * stride_bytes + 8, "bank_set_locations_device", "locations"))
      return rc;
  }
  return bank_locations(m, dev_loc, stride_bytes);
}

int hess_matcher_match_pairs(hess_matcher* m, int npairs, const int* pairs_ab, int max_match, int* out_pairs,
                             int* out_counts, float distmax, float ratiomax, int mutual_best) {
  if (!m) return HESS_ERR_ARG;
  if (const int rc = pair_list_args(m, npairs, pairs_ab, max_match, out_pairs, out_counts, "match_pairs")) return rc;
  m->last_ms = 0.0f;
  if (npairs == 0) return 0;
  M_TRY(m, hipSetDevice(m->device));
  mutual_best = mutual_best ? 1 : 0;

  return run_pairs(m, m->bank, m->bank, npairs, pairs_ab, max_match, out_pairs, out_counts, distmax, ratiomax, mutual_best, "match_pairs");
}

// GetGuidedSiftMatch for every pair of a list, each with its own H, F and bounds: match_mfma_kernel<GUIDED> on the bank and
// its locations.  Everything is checked before anything is launched or changed.
int hess_matcher_match_pairs_guided(hess_matcher* m, int npairs, const int* pairs_ab, const hess_guided_pair* geo, int max_match,
                                    int* out_pairs, int* out_counts, float distmax, float ratiomax, int mutual_best) {
  if (!m) return HESS_ERR_ARG;
  if (const int rc = pair_list_args(m, npairs, pairs_ab, max_match, out_pairs, out_counts, "match_pairs_guided")) return rc;
  if (npairs > 0 && !geo) { m->err = "match_pairs_guided: geo is NULL"; return HESS_ERR_ARG; }
  if (m->bank.typed) {
    m->err = "match_pairs_guided: guided matching with feature types is not built; remove the bank's types (bank_set_types NULL) first";
    return HESS_ERR_UNSUPPORTED;
  }
  if (!m->bank.have_loc) {
    m->err = "match_pairs_guided: the bank has no locations (hess_matcher_bank_set_locations after loading the bank)";
    return HESS_ERR_STATE;
  }
  m->last_ms = 0.0f;
  if (npairs == 0) return 0;
  M_TRY(m, hipSetDevice(m->device));
  return run_pairs(m, m->bank, m->bank, npairs, pairs_ab, max_match, out_pairs, out_counts, distmax, ratiomax, mutual_best ? 1 : 0,
                   "match_pairs_guided", geo, m->bank.loc.p);
}

// Match, estimate, guided match and (optionally) estimate of every pair of a list, chained on the device: run_verify.
// Everything is checked before anything is launched or changed.
int hess_matcher_verify_pairs(hess_matcher* m, int npairs, const int* pairs_ab, const hess_verify_params* params, int max_match,
                              int* out_pairs, int* out_counts, hess_verify_result* out, unsigned char* inlier,
                              int* putative_pairs) {
  static_assert(sizeof(hess_verify_params) == 64 && sizeof(hess_verify_result) == 128, "hess_verify_params / _result are ABI");
  if (!m) return HESS_ERR_ARG;
  if (npairs > 0) {  // (stricter than pair_list_args: out_pairs may not be NULL even with max_match 0; and by name)
    const char* null = !pairs_ab ? "pairs_ab" : !params ? "params" : !out ? "out" : !out_pairs ? "out_pairs" : !out_counts ? "out_counts" : nullptr;
    if (null) { m->err = std::string("verify_pairs: ") + null + " is NULL"; return HESS_ERR_ARG; }
  }
  if (const int rc = pair_list_args(m, npairs, pairs_ab, max_match, out_pairs, out_counts, "verify_pairs")) return rc;
  if (params) {
    if (const int rc = hess_geom_params_check(m, &params->geom, "verify_pairs")) return rc;
    if (!(params->guided_bound >= 0.0f) || !std::isfinite(params->guided_bound)) {
      m->err = "verify_pairs: params.guided_bound must be finite and not negative (0: geom.bound)";
      return HESS_ERR_ARG;
    }
    if (params->final_estimate != 0 && params->final_estimate != 1) {
      m->err = "verify_pairs: params.final_estimate must be 0 or 1, not " + std::to_string(params->final_estimate);
      return HESS_ERR_ARG;
    }
    for (int k = 0; k < 3; k++)
      if (params->reserved[k]) { m->err = "verify_pairs: params.reserved[" + std::to_string(k) + "] must be zero"; return HESS_ERR_ARG; }
  }
  if (m->bank.typed) {
    m->err = "verify_pairs: guided matching with feature types is not built; remove the bank's types (bank_set_types NULL) first";
    return HESS_ERR_UNSUPPORTED;
  }
  if (!m->bank.have_loc) {
    m->err = "verify_pairs: the bank has no locations (hess_matcher_bank_set_locations after loading the bank)";
    return HESS_ERR_STATE;
  }
  m->last_ms = 0.0f;
  if (npairs == 0) return 0;
  M_TRY(m, hipSetDevice(m->device));
  return run_verify(m, npairs, pairs_ab, *params, max_match, out_pairs, out_counts, out, inlier, putative_pairs, m->bank.loc.p);
}

float hess_matcher_last_ms(hess_matcher* m) { return m ? m->last_ms : 0.0f; }
const char* hess_matcher_last_error(hess_matcher* m) { return m ? m->err.c_str() : "null matcher"; }

}  // extern "C"

// ---- hess_matcher_int.h: the estimator's (hess_geom.hip) access to a matcher ------------------------------------------

hess_matcher_view hess_matcher_view_of(hess_matcher* m) {
  const DescSets *s = m->slot, &b = m->bank;
  return {m->device, m->st, m->e0, m->e1, m->err, &m->last_ms, {s[0].loc.p, s[1].loc.p},
          {s[0].have_loc ? s[0].count(0) : -1, s[1].have_loc ? s[1].count(0) : -1},
          b.built, &b.num, &b.cnt, &b.first, b.loc.p, b.have_loc, &m->geom};
}
