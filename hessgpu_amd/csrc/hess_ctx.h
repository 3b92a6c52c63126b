// hess_ctx.h -- the context behind the C ABI (include/hess_abi.h) and what its host-side parts share.
//
// Host side of the hot path, one file per concern:
//   hess_plan.hip      parameters -> sigma schedule and taps (SiftParam::ParseSiftParam, SiftGPU.cpp:491-563), octave geometry
//                      and the grow-only HBM / pinned buffers of a batch shape (PyramidCU::InitPyramid / ResizePyramid /
//                      FitPyramid, PyramidCU.cpp:113-489; CuTexImage::InitTexture)
//   hess_schedule.hip  the launch order of one batch on the context's stream (SiftPyramid::RunSIFT, SiftPyramid.cpp:53-198, and
//                      the PyramidCU stages under it), the table of its thresholds, per-kernel hipEvent profiling
//   hess_copier.hip    pixels in / results out: the input routes of hess_submit_host, the copier thread + SDMA delivery, submit / wait
//   hess_stager.cpp    the helper threads that stage pageable pixels (hess_stager.h; standard headers only)
//   hess_shared.hip    result buffers in node-shared memory (hess_share_results)
//   hess_abi.hip       the extern "C" entry points
#pragma once
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <limits.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/vfs.h>
#include <unistd.h>

#include "../../include/hess_abi.h"
#include "hess_dev.h"
#include "hess_owned.h"
#include "hess_stager.h"

namespace hess {

struct Schedule {
  int detector;                // HESS_DETECTOR_*: levels 0..dog+1 (Hessian) or 0..dog+2 (DoG) per octave
  int dog, level_max, level_num, level_ds;
  float sigma[kMaxLev];        // inter-level blur (SiftGPU.cpp:547-552)
  float level_sigma[kMaxLev];  // GetLevelSigma (SiftGPU.cpp:1422-1425)
  float norm[kMaxLev];         // level_sigma^4 as the ComputeHessian wrapper forms it
  float sigma_step, ln_sigma_step;
  Taps taps[kMaxLev];          // taps[l] produces level l from level l-1 (l >= 1)
};

// A grow-only allocation that knows its kind and frees itself (ensure / release, hess_plan.hip).  Not the matcher's
// DeviceBuf<T>: that one has one kind and frees before it allocates (what must survive there, a descriptor set, is built in a
// second DeviceBuf and swapped in); here the new allocation is made before the old one is freed, so that a context survives a
// refused hess_reserve, and the kinds differ in how they are freed.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  const bool pinned;  // hipHostMalloc / hipHostFree, else hipMalloc / hipFree
  char shared = 0;    // 'k' / 'd': a pinned result buffer that grows in node-shared memory (set by hess_share_results; ensure_shared)
  std::string shm;  // non-empty: p is a registered mapping of this POSIX shared memory object ("/name") or, when /dev/shm
                    // had no room, of this file (an absolute path: it has further slashes) -- hess_share_results
  explicit DevBuf(bool pinned_host = false) : pinned(pinned_host) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf();  // release()
  void forget() { p = nullptr; bytes = 0; shm.clear(); }  // the memory is given up without being freed (a lost copy may still write it)
};
struct PinnedBuf : DevBuf { PinnedBuf() : DevBuf(true) {} };

// Owned<>, Stream and Event: hess_owned.h (the matcher has them too).  The completion signal needs the ROCr headers.
using Signal = Owned<hsa_signal_t, hsa_status_t, hsa_signal_destroy>;

struct EventPair {
  hipEvent_t a, b;
  int kernel;
  double bytes;
  int kernel2 = -1;  // a second accumulator for the same launch (HESS_K_GAUSS_OCT0), or -1
  double in_lds = 0.0;  // bytes of the reference's array layout this launch neither writes nor reads: the array lives in LDS only
  int count = 1;     // launches between the two events (ProfRun: a run of consecutive launches of one kernel family)
};

// The schedule's thresholds, in one place.  Each was set by a same-call A/B on MI355X; the measurement is named beside it
// (files under profiles/, sections of DESIGN.md).  The developer build can override the ones marked (dev).
namespace policy {
// Batches up to this many images handed over by a caller who WAITS (hess_run_*) are latency cases: they take the chain
// launches for the small octaves, the short scan segments and the descriptor kernel's own host stores.  A pair SUBMITTED
// asynchronously (hess_submit_*) counts as a throughput batch: 17.0 - 17.3 against 12.3 - 12.6 Gpix/s for six pipelined
// contexts (round 5, DESIGN.md "Latency and throughput settings").
constexpr int kLatencyBatch = 2;            // (dev: HESS_MIRROR_MAX_BATCH)
// ... and only while the results of the context's last batch stayed within this: beyond it the kernel's stores wait for the
// host link (a 4096^2 image's 28 MB: 0.77 ms for the mirroring launch against 0.47 for the plain one + DMA, round 6).
constexpr size_t kMirrorMaxBytes = (size_t)16 << 20;   // (dev: HESS_MIRROR_MAX_MB)
// Octaves whose planes of the whole batch are at most this many pixels get levels 1..3 from ONE chain launch (latency
// batches only): below two 960 x 540 planes a level launch is a few dozen workgroups that mostly wait -- one 1080p image 0.400
// -> 0.334 ms; for larger batches the chain loses 2 - 4 % pipelined (profiles/r05_experiments/chain_stamps_pipelined.txt).
constexpr long long kChainMaxPixels = 2LL * 960 * 540;   // (dev: HESS_CHAIN_FROM forces the first chained octave)
// Rows per wavefront segment of the streaming extrema scan: kStreamRows (24, hess_dev.h) for throughput batches, half of it
// for latency batches (twice the wavefronts, each half as long: the scan of one image is a few hundred wavefronts).
constexpr int kLatencyStreamRowsDiv = 2;    // (dev: HESS_STREAM_ROWS)
// A batch of at least this many images delivered by the copier gets its descriptors in two launches over halves of the
// images: the first half's results cross the host link under the second half's kernel (0.53 ms of transfer for eight
// 1080p images leaves the critical path; four groups: -1 % pipelined).  profiles/r03_experiments, DESIGN.md "Result delivery".
constexpr int kSplitDescriptorsFrom = 4;    // (dev: HESS_DESC_PARTS)
// ONE image delivered by the copier (a large one) gets four launches over quarters of its feature list, for the same
// reason: 2.09 -> 1.7 ms per 4096^2 image (profiles/r05_experiments/large_image_delivery.txt).
constexpr int kLargeImageParts = 4;
// Pinned result buffers hold the worst case up front while that stays below this; beyond it they grow by need.
constexpr size_t kHostWorstCaseMax = (size_t)512 << 20;
// Pageable input of at least this size is staged into pinned memory with the helper threads (hess_submit_host): below it
// starting the helpers costs more than the copy (profiles/r03_f_host_path.json).
constexpr size_t kStagerHelpFrom = (size_t)8 << 20;
}  // namespace policy

}  // namespace hess

using namespace hess;

// One batch's pixels and their layout, built with designated initialisers (what is not named is zero).
struct PendingRun {
  const void* dev = nullptr;
  int width = 0, height = 0, pitch = 0, batch = 0, format = 0, pixtype = 0;
  size_t image_stride = 0;
  int desc_format = HESS_DESC_FORMAT_F32;  // of this batch's descriptors: what the kernels store, the copier carries, hess_wait
                                           // sizes and re-runs with, and -- of hess_ctx::run -- what the results are fetched as
  double t_load_ms = 0.0;
  bool active = false;      // submitted and not yet waited for
  bool timed_load = false;  // ev_load[] bracket a host->device transfer of this batch
};

// Result delivery ("Result delivery").  Three ways for the packed keypoints and
// descriptors of a batch to reach pinned host memory:
//   kDeliverMirror  the descriptor kernel stores them into the pinned buffers as well (posted PCIe writes out of the
//                   kernel): no command after the kernels, the shortest path for one image -- but a kernel that waits
//                   for the link holds up the memory path of whatever runs beside it;
//   kDeliverDma     a per-context copier thread waits on the host for the event behind the descriptor kernel, reads
//                   the exact byte count from the pinned count block and hands the copy to an SDMA engine through
//                   ROCr itself (hsa_amd_memory_async_copy_on_engine), then waits for its completion signal; hess_wait
//                   waits for the thread.  Not hipMemcpyAsync: HIP streams share four hardware queues, so a "copy-only"
//                   stream lands on the queue of some context's kernels, where this runtime executes the copy as a
//                   blit kernel behind them (profiles/r03_*: __amd_rocclr_copyBuffer from the copier's stream) -- the
//                   same PCIe-bound shader copy as the mirror.  hipMemcpyAsync on a copy stream remains the fallback
//                   when ROCr refuses (HESS_COPIER=hip selects it for A/B runs);
//   kDeliverBlit    hipMemcpyAsync on the context's stream after hess_wait has read the counts (the fallback, and
//                   what the reference does per level, PyramidCU.cpp:509-532).
enum { kDeliverMirror = 0, kDeliverDma = 1, kDeliverBlit = 2 };

struct Copier {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  bool stop = false, has_job = false, done = true;
  int rc = 0;            // result of the last job (hess_status)
  bool overflow = false; // the batch overflowed its feature storage: nothing was copied
  char err[320] = "";    // message of the last failed job (a fixed array: the copier thread must not throw)
  Stream cs;             // copy-only stream (fallback path)
  Event ev_done;         // recorded on the context's stream behind the last kernel of a batch
  // A batch's descriptors may come from up to kMaxParts launches (hess_ctx::parts); ev_part[k] is recorded behind launch k, ev_done behind the last.
  static constexpr int kMaxParts = 4;
  Event ev_part[kMaxParts - 1];
  // ROCr side (SDMA): agents owning the device / pinned host buffers, engine, completion signal
  bool hsa_ready = false, hsa_failed = false;
  hsa_agent_t gpu_agent{}, cpu_agent{};
  uint32_t engine = 0;          // hsa_amd_sdma_engine_id_t bit, 0 = let ROCr choose
  uint32_t engine_in = 0;       // the same for the host->device upload of pinned pixels
  Signal sig, sig2;             // one completion signal per copy in flight (keypoints, descriptors), each armed with 1: tools that
                                // interpose on ROCr (rocprofv3 --memory-copy-trace) expect exactly that of a copy's signal
  // hsa_ready and have_sig_in say whether the signals may be USED.  Where a copy is lost its signal is forgotten on the spot
  // (Signal::forget: a late copy may still write it), so what the Copier still owns at its end is safe to destroy.
  // The job (copier_post): the run to deliver and whether it begins with the batch's pixels still on their way
  // (hess_submit_host, pinned input).  Then the upload is an SDMA copy started by the submitting thread with sig_in as
  // its completion signal; the copier thread waits for it ON THE HOST and only then enqueues the kernels -- no command
  // that waits for the transfer ever sits in a hardware queue, which the context's stream shares with other contexts.
  PendingRun* run = nullptr;
  bool upload_first = false;
  bool have_sig_in = false;
  Signal sig_in;
};

// The descriptor launches of the batch being enqueued (choose_parts, hess_schedule.hip): n groups of images, end[k] = first
// image after group k -- or, for ONE image, n ranges of its features (part k ends at feature total (k + 1) / n, DescParams::part).
struct Parts {
  int n = 1, end[Copier::kMaxParts] = {0, 0, 0, 0};
  bool features = false;
};

// The developer switches of one context, as read_switches() (hess_abi.hip) found them in the environment when hess_create ran:
// per context, since tests set and clear them between contexts of one process.  HESS_DELIVERY is read with getenv (the shipped
// library has it), the rest with dev_env().  Read once per process or at first use, where they act: HESS_NO_PRIME_BATCH, HESS_COPIER,
// HESS_COPIER_ENGINE, HESS_UPLOAD_ENGINE, HESS_COPIER_FAULT, HESS_CHAIN_STAMPS, HESS_SHARE_FORCE_FILE; HESS_COPY_TIMEOUT_S (shipped).
struct Switches {
  int delivery_pref = -1;          // HESS_DELIVERY=mirror|dma|blit: a kDeliver* value (-1: by batch size, choose_delivery)
  int mirror_max_batch = policy::kLatencyBatch;       // HESS_MIRROR_MAX_BATCH: largest batch that takes the latency settings
  size_t mirror_max_bytes = policy::kMirrorMaxBytes;  // HESS_MIRROR_MAX_MB: largest results the descriptor kernel mirrors (floored at 0)
  int cap_init = 0;                // HESS_INITIAL_CAP: initial raw / feature capacity, so that the grow path runs (0: by image size)
  bool no_pair = false;            // HESS_NO_PAIR: one launch per pyramid level
  bool no_top_fusion = false;      // HESS_NO_TOP_FUSION: the top level is stored and its det-H made by a launch of its own
  bool no_first_fusion = false;    // HESS_NO_FIRST_FUSION: level 0 of octave 0 from a launch of its own, written to HBM
  int chain_from = 0;              // HESS_CHAIN_FROM: first octave produced by one level-chain launch (0: by batch size; 99: none)
  bool no_host_upload = false;     // HESS_NO_SIDE_UPLOAD: pinned input is uploaded by a copy on the context's stream
  int desc_parts = 0;              // HESS_DESC_PARTS: descriptor launches / result transfers per batch (0: by batch size)
  int stream_rows = 0;             // HESS_STREAM_ROWS: rows per wavefront segment of the extrema scan, a multiple of 3 (0: by batch size)
  int desc_px_band = 4096;         // HESS_PX_BAND: pixels per raster band of descriptor_pixel_kernel, 64 .. 4096 (small bands at ordinary footprints)
  int desc_xcd_block = 64;         // HESS_DESC_XCD: features per XCD block of the descriptor launch (0: plain order)
};

struct ProfEvents {  // the profiling events of a context
  std::vector<EventPair> pending;  // pairs recorded and not yet read (drain_profile)
  std::vector<hipEvent_t> pool;    // events free for reuse
  ~ProfEvents() { for (auto& ep : pending) pool.insert(pool.end(), {ep.a, ep.b}); for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};

// Members are destroyed in reverse order (hess_destroy ends in `delete c`): the buffers first, then the copier's stream, events
// and signals, the context's events, and the stream last.  A member that owns a runtime object needs no line anywhere else.
struct hess_ctx {
  int device = 0;
  Stream st;
  Event ev[8], ev_load[2];         // between the stages of a batch; around the host->device transfer of the pixels
  ProfEvents prof_ev;
  Copier cp;
  Switches sw;
  hess_params p{};
  Schedule sch{};
  // geometry of the current plan
  bool planned = false;
  int in_w = 0, in_h = 0;   // caller's image size
  int ds = 0;               // input decimation (first_octave / auto down-scaling)
  int img_w = 0, img_h = 0; // after decimation and width truncation
  Geom g{};
  Taps taps0{};              // initial smoothing
  bool has_taps0 = false;
  int cap_raw = 0, cap_sel = 0, cap_feat = 0;
  bool use_topk = false, multi = false;
  int dim = 0;
  // hess_set_descriptor_format: the format of the runs to come.  Every run record is built with it (PendingRun::desc_format)
  // and the setter refuses while one is pending, so for the length of a run -- plan(), enqueue(), the copier thread, hess_wait
  // and its overflow re-run -- it equals the run's.  Afterwards the run record alone says what the results are.
  int desc_format = HESS_DESC_FORMAT_F32;
  int planned_format = HESS_DESC_FORMAT_F32;  // the format the current plan's result buffers are sized for
  // device buffers (grow-only, like CuTexImage::InitTexture)
  int found_tasks = 0;  // scan tasks per image the detection store is laid out for (plan)
  DevBuf gauss, deth, got, input_f32, upsampled, stage, rowoff, level_count, raw_total, found, task_count, raw, sel,
      sel_total, recs, ocount, foffset, fsrc, feat_total, feat_first, img_base, keys, desc;
  // Everything the detection stages expect zeroed lives in one allocation and is cleared by one fill per batch:
  // overflow flags, detection counters, per-row counts, the top-K histogram, the extrema bit masks (views into `zeroed`).
  DevBuf zeroed;
  size_t zeroed_used = 0;
  bool zero_filled = false;  // the running batch's det-H launch has cleared `zeroed`
  struct View { void* p = nullptr; } rowmask, rowcnt, overflow, hist, tk,  // tk: tickets, chunk words, per-level counts of the top-K launch
      found_count, place_ticket, place_flag;                                // detections found per image; extrema_place_kernel's ticket and flag per image
  // host results
  int batch = 0;          // images whose results the context holds (0 after a failed or while a pending run: hess_count /
                          // hess_fetch / hess_device_results refuse instead of handing out the run before)
  int pyramid_batch = 0;  // images whose pyramid is resident (hess_run_keypoints on the current image)
  std::vector<int> counts;
  std::vector<size_t> offs;
  PinnedBuf h_keys, h_desc, h_small;
  // hess_share_results: the two result buffers live in shared memory objects "/<share>.k<n>" / "/<share>.d<n>" that
  // another process of the node can map; a 4 KB directory object "/<share>.h" says which ones are current
  std::string share;
  // (directory layout = hessgpu_amd/dist.py SharedResultsReader._HDR: generations, sizes and the absolute paths of the
  // current buffers -- under /dev/shm, or under HESS_SHARE_DIR / TMPDIR when /dev/shm has no room for them)
  struct ShareDir {
    uint32_t magic, gen_keys, gen_desc, pad;
    uint64_t keys_bytes, desc_bytes;
    char keys_path[1024], desc_path[1024];
  }* share_dir = nullptr;
  bool share_by_need = false;      // the shared result buffers are sized by the batches seen, not for the worst case
  PinnedBuf h_stage;               // pinned staging of pageable input pixels (hess_submit_host)
  double stamp_submit0 = 0.0, stamp_submit1 = 0.0;  // HESS_CHAIN_STAMPS
  bool level0_in_lds = false;      // the last run's level 0 of octave 0 was not written to HBM (FIRST tiles)
  size_t last_input_bytes = 0;     // bytes of the last batch handed over by hess_submit_host (still in `stage`)
  // results written by the descriptor kernel straight into the pinned host buffers (no D2H pass after it)
  bool host_direct = false;        // delivery == kDeliverMirror for the submitted batch
  bool host_fits = false;          // the pinned result buffers hold the worst case of the current plan
  int delivery = kDeliverMirror;   // of the submitted batch (choose_delivery)
  // The one copy; the copier thread reads it without a lock.  enqueue() writes it: on the submitting thread BEFORE that thread
  // takes cp.mu to post the job (copier_post), or on the copier thread itself when the job uploads first.  Nothing writes it
  // while a job is posted: every entry that enqueues refuses while run.active, hess_reserve's dry batch returns early then,
  // and wait_inner's regrow loop resubmits only after it has seen cp.done under cp.mu.
  Parts parts;
  size_t last_result_bytes = 0;    // keypoints + descriptors the last batch delivered, and its size
  int last_result_batch = 0;
  std::atomic<bool> caller_waits{false};  // inside hess_run_* (submit + wait in one call; read by the copier thread, too)
  int regrown = 0;                 // times the feature storage was grown after an overflow (hess_debug_regrown)
  int seen_features = 0;           // largest per-image feature count of the last finished batch (0: none yet): sizes the descriptor grid
  bool keep_levels = false;        // hess_debug_keep_levels: the top Gaussian level of every octave is written to HBM as well
  Stager sg;                       // hess_stager.h
  // A DMA copy that did not complete in time (or that ROCr reported as failed) may still be in flight, or land later:
  // its targets -- the pinned result buffers, the pixel staging area -- must neither be reused nor freed.  The context
  // refuses every further run (HESS_ERR_DEVICE) and hess_destroy leaves those buffers alone (abandon_lost_copy_targets).
  std::atomic<bool> poisoned{false};
  long long primed_shapes[4] = {-1, -1, -1, -1};  // shapes (width, height, batch) hess_reserve has run a dry batch for
  unsigned primed_next = 0;
  DevBuf prime_px;                 // the dry batch's scratch image (zero pixels)
  PendingRun run;                  // the batch submitted last: pending while run.active, then the current image's geometry (width 0: none)
  bool accepted_submit = false;    // hess_submit_* has accepted a batch at least once (hess_share_results comes before that)
  // user-supplied keypoint lists (SiftPyramid::SetKeypointList), one per image of the next run: used by it, then cleared.
  // The keys of all images lie back to back at the start of the pinned block h_user since the set call; enqueue_user
  // appends what else key_bin_kernel reads (UserBlock) and uploads the block to d_user with one copy.
  PinnedBuf h_user;
  DevBuf d_user;
  std::vector<int> user_counts;     // keys per image; empty: no list is pending
  int user_total = 0, user_max = 0; // their sum (> 0 while a list is pending) and the largest of them
  bool user_have_orientation = false;
  bool user_rect = false;           // HESS_KEYS_RECTANGLES: the keys are rectangles (x, y, width, height); implies user_have_orientation
  bool user_on_current = false;     // RunSIFT(num, keys, flag): skip filtering, reuse the resident pyramid
  std::vector<int> user_levels;     // parity hook: explicit level index per user keypoint (hess_debug_key_levels; one image)
  DevBuf kmember;                   // key_bin_kernel's scratch: [B][user_max] levels of every key
  DevBuf kmap;                      // [B][cap_list] list position -> input index (_keypoint_index); h_kmap: pinned, filled by
  PinnedBuf h_kmap;                 // the route the results take (the kernel's own stores, the copier thread, hess_wait's copy)
  bool user_result = false;         // last results are in u_keys / u_desc (input order, the images back to back)
  std::vector<hess_keypoint> u_keys;
  std::vector<unsigned char> u_desc;  // [sum of counts][run_desc_bytes]: floats or bytes, as the run's format says
  std::vector<size_t> u_first;      // [batch + 1] first key of every image in u_keys / u_desc
  std::vector<int> u_order;         // the lists of the last keypoint-list run, list position -> input index, the images back to
                                    // back as the device records are: image b's list is entries [offs[b], offs[b + 1]) (hess_key_list_order)
  const RawKey* d_list = nullptr;  // list fed to the orientation stage in the last run
  const int* d_list_total = nullptr;
  int cap_list = 0;
  float timing[HESS_T_COUNT] = {};
  bool stage_events = false;  // events between the stages of the running batch (each costs a ~6 us bubble on the stream)
  std::string err;
  // profiling
  bool prof = false;
  double k_ms[HESS_K_COUNT] = {};
  long long k_n[HESS_K_COUNT] = {};
  double k_bytes[HESS_K_COUNT] = {};
  double k_in_lds[HESS_K_COUNT] = {};   // hess_profile_get_in_lds
};

// ---- shared by the host-side files (namespace hess) ----
namespace hess {

void set_err(hess_ctx* c, const char* fmt, ...);

// Bytes of one descriptor of a run in format `format` (HESS_DESC_FORMAT_*): the one place that knows the element size.
inline size_t run_desc_bytes(const hess_ctx* c, int format) { return desc_bytes(c->dim, format); }

// A caller's keypoint lists are pending for the next run; the records an image's list may take (GenerateFeatureListTex
// reserves 2 * num + 8, PyramidCU.cpp:575; here for the largest list of the batch: key_level_kernel says why no list gets
// there); the list is consumed or dropped.
inline bool user_mode(const hess_ctx* c) { return c->user_total > 0; }
inline int user_cap(const hess_ctx* c) { return 2 * c->user_max + 8; }
inline void clear_user_list(hess_ctx* c) {
  c->user_counts.clear();
  c->user_total = c->user_max = 0;
  c->user_on_current = false;
}

// Environment switches.  The shipped library reads four: HESS_SHARE_DIR (and TMPDIR) -- where node-shared result buffers go
// when /dev/shm has no room --, HESS_COPY_TIMEOUT_S -- how long a result copy may take before the context is poisoned --
// and HESS_DELIVERY (how results reach the host).  Everything else (struct Switches and the list above it) exists only in the
// DEVELOPER build (-DHESS_DEV_SWITCHES: hessgpu_amd/dev/libhessgpu.so, built beside the product by hessgpu_amd/build.py;
// hess_dev_switches() tells which one is loaded).  The tests that need a switch and tools/robustness.sh load that build.
#ifdef HESS_DEV_SWITCHES
inline const char* dev_env(const char* name) { return getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

#define HIP_TRY(c, expr)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      set_err(c, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return e_ == hipErrorOutOfMemory ? HESS_ERR_NOMEM : HESS_ERR_DEVICE;                \
    }                                                                                     \
  } while (0)

// hess_plan.hip
int ensure(hess_ctx* c, DevBuf& b, size_t bytes);
void release(DevBuf& b);
void default_params(hess_params* p);
bool accept_params(hess_params* p);
void make_taps(const hess_params& p, float sigma, Taps* t);
void resolve(hess_ctx* c);
int fmt_channels(int format);
int plan(hess_ctx* c, int width, int height, int batch);
// hess_shared.hip
int ensure_shared(hess_ctx* c, DevBuf& b, size_t bytes);
// hess_schedule.hip
void drain_profile(hess_ctx* c);
int enqueue(hess_ctx* c, const PendingRun& r);
size_t user_block_bytes(int total, int nimg);  // bytes of the pinned block h_user for `total` keys of `nimg` images
// hess_copier.hip
int upload_beside_queues(hess_ctx* c, const void* pixels, size_t bytes, bool* taken);
int upload_on_stream(hess_ctx* c, const void* pixels, size_t bytes, bool pinned);
void copier_warm_up(hess_ctx* c);
int copier_start(hess_ctx* c);
void copier_stop(hess_ctx* c);
void choose_delivery(hess_ctx* c, int batch);
int check_user_batch(hess_ctx* c, int batch);
int submit_impl(hess_ctx* c, PendingRun& r);
int wait_impl(hess_ctx* c, PendingRun& r);

}  // namespace hess
