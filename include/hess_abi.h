/*
 * hess_abi.h -- C ABI of the MI355X-native Hessian + SIFT-descriptor hot path.
 *
 * This is the drop-in boundary of the build: plain C types, pointers and sizes only.
 * It is what the host-side `SiftGPU` class (include/SiftGPU.h, libsiftgpu.so) binds in
 * place of the reference's CUDA backend objects.  Each entry point cites the reference
 * interface it replaces (paths relative to the reference tree, src/SiftGPU/...).
 *
 * The same signatures, prefixed `hess_cpu_`, are implemented by the CPU oracle
 * (oracle/hess_oracle.c) so that the parity tests are backend-agnostic.  The oracle is
 * test infrastructure only; nothing in the product links it.
 *
 * Error convention: functions returning int return 0 (HESS_OK) on success and a negative
 * hess_status on failure; no exceptions cross this boundary; hess_last_error() gives text.
 * One context per host thread / per device (reference: one SiftGPU instance per thread per
 * device, TestWin/MultiThreadSIFT.cpp:90-133).
 */
#ifndef HESS_ABI_H
#define HESS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: hess_params.reserved[] must be zero (the oracle-only `detector` word of version 1 is gone from the product's
 *    struct); hess_submit_host, hess_device_count, hess_debug_key_levels (now covering one run), hess_debug_regrown.
 * 3: hess_share_results / hess_shared_results_info (added during version 2 without a bump: round 3);
 *    hess_params.descriptor_order (the first of the reserved words: a version-2 struct, all zero there, asks for
 *    the default); hess_count / hess_fetch / hess_device_results refuse (HESS_ERR_ARG / _STATE) after a failed run
 *    instead of handing out the results of the run before.
 * 4: HESS_DESC_ORDER_PIXEL, the order hess_default_params now chooses (a version-3 struct keeps what it asks for: 0 is
 *    the interleaved order); hess_debug_keep_levels (the top Gaussian level of an octave is no longer written to HBM
 *    unless asked for); a context whose DMA copy was lost refuses further runs (HESS_ERR_DEVICE, "poisoned").
 * 5: hess_params.detector (word 0 of reserved[], which a version-2, -3 or -4 struct leaves zero: the Hessian detector):
 *    HESS_DETECTOR_DOG runs the difference-of-Gaussians detector of the reference's build without GPU_HESSIAN.
 *    hess_matcher_bank_set / _set_f32 / _set_device / _read and hess_matcher_match_pairs (added during version 5
 *    without a bump).  hess_set_descriptor_format / hess_desc_format / hess_fetch_u8 and
 *    hess_matcher_bank_set_device_u8 (byte descriptors; added during version 5 without a bump: hess_params keeps its
 *    layout, and a context that never calls the setter behaves as before).  hess_matcher_set_dim / hess_matcher_dim
 *    (64-d descriptors of a half_sift run in the matcher; added during version 5 without a bump: a matcher that never
 *    calls the setter is 128-d as before).  hess_set_keypoints_batch / hess_run_keypoints_batch / hess_key_list_order
 *    (keypoint lists for every image of a batch; added during version 5 without a bump: hess_set_keypoints and
 *    hess_run_keypoints are the same calls with one image and answer as before, except that hess_set_keypoints now
 *    refuses while a submitted batch is pending, where it used to corrupt that batch's results).
 *    hess_matcher_set_types / _bank_set_types / _bank_set_types_device (the feature-type gate of the matcher; added
 *    during version 5 without a bump: a matcher that never calls them matches as before).
 *    hess_geom_sample, hess_matcher_estimate / _estimate_pairs, hess_matcher_bank_set_locations(_device) (H or F from
 *    matches on the device; added during version 5 without a bump: a matcher that never calls them behaves as before).
 *    hess_geom_params.refit, hess_geom_result.refits / .ransac_inliers (the least-squares refit on the inliers, words
 *    of the reserved arrays; added during version 5 without a bump: `refit` 0 behaves as before).
 *    hess_matcher_match_pairs_guided / hess_guided_pair (guided matching for bank pairs; added during version 5 without a
 *    bump: a matcher that never calls it behaves as before).
 *    hess_matcher_verify_pairs / hess_verify_params / hess_verify_result (match, estimate, guided match and estimate for
 *    bank pairs in one call; added during version 5 without a bump: a matcher that never calls it behaves as before). */
#define HESS_ABI_VERSION 5

/* Detectors (hess_params.detector).  The reference picks one at compile time (#define GPU_HESSIAN, config.h:36):
 *   HESSIAN  determinant of the Hessian * sigma^4 of levels 1..dog, extrema with sign conditions (the default)
 *   DOG      differences of adjacent Gaussian levels D_l = G_l - G_(l-1) (levels 0..dog+2, sigma0 * 2^(1/dog) per the
 *            reference's _level_min = -1), extrema without sign conditions, type = sign of the extremum, and with
 *            max_orientation > 1 the two strongest histogram peaks as 16-bit angles (ProgramCU.cu:598-637, 680-699,
 *            853-854, 1493-1548; SiftGPU.cpp:466-556) -- classic SiftGPU. */
enum { HESS_DETECTOR_HESSIAN = 0, HESS_DETECTOR_DOG = 1 };

typedef enum hess_status {
  HESS_OK = 0,
  HESS_ERR_ARG = -1,      /* bad argument (null pointer, non-positive size, bad index)   */
  HESS_ERR_TOO_BIG = -2,  /* image exceeds tex_max_dim and auto_downscale is off
                             (reference: exit() in PyramidCU.cpp:170-174 -> error return)  */
  HESS_ERR_DEVICE = -3,   /* HIP runtime error (reference: CheckErrorCUDA -> RunSIFT 0)  */
  HESS_ERR_NOMEM = -4,    /* allocation failed                                           */
  HESS_ERR_STATE = -5,    /* call out of order (fetch before run, ...)                   */
  HESS_ERR_UNSUPPORTED = -6
} hess_status;

/* Feature types, reference config.h:45-50. */
enum { HESS_TYPE_DARK_BLOB = 0, HESS_TYPE_BRIGHT_BLOB = 1, HESS_TYPE_SADDLE = 2, HESS_TYPE_NONE = 3 };

/* Truncation methods, reference SiftPyramid.h:73-77 (-tc/-tc1, -tc2, -tc3, -topk). */
enum { HESS_TRUNC_HIGHEST_0 = 0, HESS_TRUNC_HIGHEST_1 = 1, HESS_TRUNC_LOWEST = 2, HESS_TRUNC_TOPK = 3 };

/* Order in which the samples of a descriptor cell are added into its orientation bins (ComputeDescriptor_Kernel,
 * ProgramCU.cu:1723-1774: one thread per cell walks the cell's box row by row and adds as it goes).
 *   SEQUENTIAL             the reference's own order, sample after sample: bit-identical to a sequential scan
 *   INTERLEAVED            four partial sums per bin -- the samples at positions 0, 1, 2, 3 modulo 4 of that walk --
 *                          added as (p0 + p1) + (p2 + p3): every lane of the kernel keeps its own samples' sums, no
 *                          cross-lane exchange per sample; differs from the sequential sum by rounding only (<= 3e-7
 *                          on unit-norm descriptors, measured; the tests bound it by 1e-6; north star: 1e-4);
 *                          descriptor kernel 16 % faster than SEQUENTIAL
 *   PIXEL (default)        every pixel of the footprint is evaluated ONCE (gather, Gaussian weight, bin split in the
 *                          keypoint's frame: the reference re-evaluates it for each of the up to four cells it belongs
 *                          to) and adds its weight to <= 2 x 2 cells x 2 bins in 32-bit fixed point with a per-keypoint
 *                          power-of-two scale -- integer sums, so the result does not depend on the order of the
 *                          additions (any parallel schedule gives the same bits; the oracle's plain loop does).
 *                          Distance to SEQUENTIAL on unit-norm descriptors, measured per BASELINE config
 *                          (tests/test_gpu_parity.py): 640x480 (configs[2]) 2.5e-6, 1920x1080 (configs[1]) 6e-6, 4096x4096
 *                          (configs[4]) 1.6e-5 -- ONE bound for all of them in the tests, TOL_ORDER = 3e-5 (bench.py checks
 *                          its 1080p image against 1e-5); north star 1e-4.  Most of the distance is SEQUENTIAL's own float
 *                          rounding (it rounds every cell centre at the magnitude of the image coordinate: 1e-5 relative
 *                          at x = 4000): a float64 evaluation of the reference's formula is within 2.5e-7 of PIXEL on all
 *                          three (TOL_EXACT = 1e-6).  Descriptor kernel a further 21 % faster, whole path + 9 %.
 *                          Needs luminance in [0, 1] for its overflow bound, so two inputs keep the INTERLEAVED order --
 *                          permanently, not as a transition: float pixels (HESS_PIX_F32, taken as they are) and user
 *                          keypoint lists (hess_set_keypoints: any scale at any level).  All three orders have a bitwise
 *                          oracle restatement and stay in tools/fuzz_parity.py and the robustness matrix.
 * Rectangles (HESS_KEYS_RECTANGLES at hess_set_keypoints) take none of the three: descriptor_rect_kernel has one order
 * of its own -- per raster column, then a fixed order over the lanes -- stated at that enum and in the kernel's header. */
enum { HESS_DESC_ORDER_INTERLEAVED = 0, HESS_DESC_ORDER_SEQUENTIAL = 1, HESS_DESC_ORDER_PIXEL = 2 };

/* Pixel formats accepted by hess_run_* (the GL enums of SiftGPU::RunSIFT(w,h,data,fmt,type)
 * are mapped onto these by the C++ class; reference GLTexImage.cpp:918-1036). */
enum { HESS_FMT_LUM = 1, HESS_FMT_LUM_ALPHA = 2, HESS_FMT_RGB = 3, HESS_FMT_RGBA = 4,
       HESS_FMT_BGR = 5, HESS_FMT_BGRA = 6 };
enum { HESS_PIX_U8 = 1, HESS_PIX_U16 = 2, HESS_PIX_F32 = 3 };

/*
 * Tunables.  Replaces the process-global GlobalParam statics (GlobalUtil.cpp:51-144) and
 * the SiftParam members (SiftGPU.h:59-86) that the hot path reads.  A zero in a field
 * marked (0=default) selects the reference default, as SiftParam::ParseSiftParam
 * (SiftGPU.cpp:491-563) does.
 */
typedef struct hess_params {
  int32_t abi_version;          /* must be HESS_ABI_VERSION                                   */
  int32_t dog_level_num;        /* -d   (0=default 3)      scales per octave                  */
  float sigma0;                 /*      (0=default 1.6)                                       */
  float sigman;                 /*      (0=default 0.5)                                       */
  float dog_threshold;          /* -t   (0=default 0.02/dog_level_num)                        */
  float edge_threshold;         /* -e   (0=default 10)                                        */
  float filter_width_factor;    /* -f   (0=default 4.0)   GlobalUtil.cpp:62                   */
  float orient_window_factor;   /* -w   (0=default 2.0)   GlobalUtil.cpp:134                  */
  float orient_gaussian_factor; /*      (0=default 1.5)   GlobalUtil.cpp:135                  */
  float desc_window_factor;     /* -dw  (0=default 3.0)   GlobalUtil.cpp:63                   */
  int32_t first_octave;         /* -fo  (default 0)  SiftGPU.cpp:1166-1175: the reference's Hessian build
                                   takes only >= 0 at its option parser (and so does this build's
                                   SiftGPU::ParseParam); -1..-3 = first octave up-sampled by 2^-fo
                                   (PyramidCU.cpp:120-138,1517-1525, ProgramCU.cu:233-310), kept below the
                                   parser in the reference and reachable here through this struct only */
  int32_t octave_num;           /* -no  (<=0 = no limit)  GlobalUtil.cpp:123                  */
  int32_t subpixel;             /* -s   (default 1)                                           */
  int32_t max_orientation;      /* -m   (default 2; clamped to 1..4 by ParseParam)            */
  int32_t fixed_orientation;    /* -ofix                                                      */
  int32_t lowe_origin;          /* -loweo                                                     */
  int32_t half_sift;            /* -half  64-d descriptor, unsigned gradient                  */
  int32_t compute_descriptors;  /* 0 with -sd                                                 */
  int32_t normalize;            /* 1 (GlobalUtil::_NormalizedSIFT)                            */
  int32_t truncate_method;      /* HESS_TRUNC_*                                               */
  int32_t feature_count_threshold; /* -tc* / -topk value (<=0 = off)                          */
  int32_t tex_max_dim;          /* -maxd (0=default 3200)                                     */
  int32_t auto_downscale;       /* -ads                                                       */
  int32_t verbose;              /* bit 0: messages on stderr; bit 1: stage timers (hess_timing entries 2..10; the
                                   reference's _timingS, SiftGPU.cpp:433-464).  0 = silent, total time only: the
                                   events between stages cost about 6 us each on the device                  */
  int32_t dynamic_indexing;     /* -di  descriptor bins indexed dynamically (GlobalUtil.cpp:108,
                                   ProgramCU.cu:1755-1771): a sample whose bin coordinate rounds up to
                                   exactly 8.0 is then added to bin 8 (folded into bin 0), not dropped */
  int32_t descriptor_order;     /* HESS_DESC_ORDER_*: how a descriptor bin's samples are added up (see the enum)  */
  union {
    int32_t reserved[6];        /* words 1..5 must be zero: hess_create refuses anything else                     */
    struct {
      int32_t detector;         /* HESS_DETECTOR_* (word 0 of reserved[]; also the test oracle's detector switch,
                                   oracle/hess_oracle.h, whose values 0 and 1 are these two)                      */
      int32_t reserved_tail[5];
    };
  };
} hess_params;

/* Binary-identical to SiftGPU::SiftKeypoint (SiftGPU.h:108-116): 24 bytes. */
typedef struct hess_keypoint {
  float x, y, s, o;
  float response;
  uint16_t level;
  uint16_t type;
} hess_keypoint;

/* Stage timers in the order of SiftGPU::_timing[12] (config.h:17-31), milliseconds. */
enum { HESS_T_LOAD = 0, HESS_T_ALLOC, HESS_T_PYRAMID, HESS_T_DETECT, HESS_T_LIST, HESS_T_ORIENT,
       HESS_T_MULTI_ORIENT, HESS_T_DOWNLOAD, HESS_T_DESCRIPTOR, HESS_T_VBO, HESS_T_REDUCTION,
       HESS_T_TOTAL, HESS_T_COUNT };

/* Stage dumps for the parity tests (hess_debug_level `what`). */
enum { HESS_DBG_GAUSS = 0,  /* Gaussian level, wa*h floats                                   */
       HESS_DBG_DETH = 1,   /* the detector's response plane, wa*h floats: det-Hessian * sigma^4 (levels
                               0..dog+1), or with HESS_DETECTOR_DOG G_l - G_(l-1) (levels 1..dog+2; level 0
                               holds det-H * sigma^4 of G_0, as in the test oracle)               */
       HESS_DBG_GOT = 2     /* (|grad|/2, theta) interleaved, 2*wa*h floats, levels 1..dog   */ };

/* One raw detection (before top-K / orientation), for hess_debug_list. 32 bytes. */
typedef struct hess_rawkey {
  int32_t level_index;  /* octave*dog_level_num + (level-1)                                  */
  int32_t col, row;
  uint32_t packed;      /* half(response)<<16 | 0x4 | type  (key-map pixel .x, ProgramCU.cu:865) */
  float dx, dy, ds;     /* sub-pixel offsets (ProgramCU.cu:868)                              */
  uint32_t pad;
} hess_rawkey;

typedef struct hess_ctx hess_ctx; /* opaque */

/* Fill *p with the reference defaults (all "0=default" fields resolved). */
void hess_default_params(hess_params* p);

/* Number of usable HIP devices (0 without a GPU): what the reference's callers hard-code as "device 0 and 1"
 * (TestWin/MultiThreadSIFT.cpp:233-234; ProgramCU::CheckCudaDevice, ProgramCU.cu:3386-3440, rejects the rest). */
int hess_device_count(void);

/* 1 when the loaded library is the DEVELOPER build (-DHESS_DEV_SWITCHES: schedule A/B switches, fault injection and the
 * other test hooks read from the environment, hessgpu_amd/csrc/hess_ctx.h), 0 for the shipped library, which reads
 * HESS_SHARE_DIR / TMPDIR, HESS_COPY_TIMEOUT_S and HESS_DELIVERY only.  No reference counterpart.  (Added in version 4.) */
int hess_dev_switches(void);

/* Replaces SiftGPU::CreateContextGL/VerifyContextGL -> InitSiftGPU -> new PyramidCU
 * (SiftGPU.cpp:149-227,1516-1539) and ProgramCU::CheckCudaDevice (ProgramCU.cu:3386-3440).
 * `device` is the HIP device ordinal.  Returns NULL on failure. */
hess_ctx* hess_create(int device, const hess_params* params);
void hess_destroy(hess_ctx* ctx);

/* Replaces PyramidCU::InitPyramid/ResizePyramid/ResizeFeatureStorage (PyramidCU.cpp:113-489)
 * and SiftGPU::AllocatePyramid: pre-allocates pyramids for `batch` images of w*h so that
 * hess_run_* does no allocation (grow-only, like the reference).  It also creates the runtime objects a batch of that
 * size uses (result copier thread and its DMA queue, the stream's hardware queue): the first batch does not pay for them. */
int hess_reserve(hess_ctx* ctx, int width, int height, int batch);

/* Replaces SiftGPU::RunSIFT(w,h,data,fmt,type) -> GLTexInput::SetImageData (CUDA branch,
 * GLTexImage.cpp:918-1036) -> SiftPyramid::RunSIFT (SiftPyramid.cpp:53-198) for `batch`
 * independent images of identical size (`image_stride` bytes apart, rows `pitch` bytes apart).
 * Host pointer version: pixels are copied to the device.
 *
 * Layout (the same for all four hess_run_* / hess_submit_* entry points).  Pixel (x, y) of image b starts at byte
 * b * image_stride + y * pitch + x * channels * bytes_per_channel of `pixels`; the pixels of a row are contiguous.
 *   - pitch >= width * channels * bytes_per_channel.  Anything beyond the row's bytes is padding: never read by a kernel,
 *     and -- with host pixels -- not copied beyond the last pixel.  The span the library touches is exactly
 *     (batch - 1) * image_stride + (height - 1) * pitch + width * channels * bytes_per_channel  bytes from `pixels`, so a
 *     region of interest may end in the last row of the caller's allocation.  hess_last_input retains that span.
 *   - image_stride is free otherwise: 0 (one image `batch` times), below pitch (images side by side in one row of `pitch`
 *     bytes), pitch * height (back to back) or larger (frames with a gap, a region of interest of larger frames).
 *   - for 16-bit and float pixels pitch and image_stride are multiples of the channel type's size, and a DEVICE pointer is
 *     aligned to it (a host pointer need not be: host pixels are copied bytewise first).
 * HESS_ERR_ARG with a hess_last_error text naming the argument for: a pitch below the row's bytes; a pitch, image_stride
 * or device pointer that breaks the rule for 16-bit and float pixels.  Refused before anything is read or enqueued.
 * Alignment beyond that is a matter of speed, not of results: u8 luminance whose pitch, image_stride and device address
 * are multiples of 4 is read by the first Gaussian kernel directly; every other layout goes through one conversion pass. */
int hess_run_host(hess_ctx* ctx, const void* pixels, int width, int height, int pitch,
                  size_t image_stride, int batch, int format, int pixtype);
/* Asynchronous pair: hess_submit_device enqueues the whole path on the context's stream and returns;
 * hess_wait blocks until the results are in host memory.  Two contexts used alternately overlap the
 * result transfer of one batch with the kernels of the next.  One submitted batch per context. */
int hess_submit_device(hess_ctx* ctx, const void* dev_pixels, int width, int height, int pitch,
                       size_t image_stride, int batch, int format, int pixtype);
/* The same from host memory: the pixels cross with one asynchronous transfer on the context's stream (straight
 * from the caller's buffer when it is pinned, through the context's pinned staging buffer otherwise; the buffer
 * may be reused as soon as the call returns in the second case, after hess_wait in the first). */
int hess_submit_host(hess_ctx* ctx, const void* pixels, int width, int height, int pitch,
                     size_t image_stride, int batch, int format, int pixtype);
int hess_wait(hess_ctx* ctx);
/* Same, pixels already resident in device memory (HBM) of ctx's device. */
int hess_run_device(hess_ctx* ctx, const void* dev_pixels, int width, int height, int pitch,
                    size_t image_stride, int batch, int format, int pixtype);

/* The pixels of the last batch handed over with hess_submit_host / hess_run_host, as they were handed over (the
 * context keeps them in its staging area until the next batch).  Replaces GLTexInput keeping the converted image in
 * _pixel_data between calls (GLTexImage.cpp:918-1036, PyramidCU.cpp:1458-1462), which is what lets the reference's
 * SiftGPU::RunSIFT() run the current image again: this build's SiftGPU class borrows the caller's pointer for the call
 * and only comes back for the pixels if the image is run again without being handed over again. */
int hess_last_input(hess_ctx* ctx, void* out, size_t bytes);

/* What keys_have_orientation of hess_set_keypoints / hess_run_keypoints says about the caller's keys.  The reference
 * tests the flag's truth for "oriented" and the value -1 for rectangles (SiftPyramid.cpp:349-354): any other non-zero
 * value means ORIENTED here as well.
 *   NONE        (x, y, s): the strongest orientation is found on the device
 *   ORIENTED    (x, y, s, o): no orientation pass
 *   RECTANGLES  (x, y) is the top-left corner of an axis-aligned rectangle, s its width and o its height, in image
 *               pixels; the result is a 4 x 4-cell, 8-bin gradient histogram over the rectangle -- the reference's way of
 *               describing regions with the SIFT machinery (SiftPyramid.cpp:345-354, PyramidCU.cpp:522, 591-666,
 *               ProgramCU.cu:1806-1948, 2105-2143):
 *               level     the binning of every caller key, applied to min(s, o) / 12.0f instead of s (the catch-all
 *                         first and last levels as always; hess_debug_key_levels overrides as always);
 *               record    corner as any key's position ((v - origin offset) / scale + 0.5 in 14.10 fixed point,
 *                         masked); W = s / scale in 8.8 fixed point masked to 16 bits (256 level pixels wrap);
 *                         H = o / scale as the binary32 quotient; response and type bits zero;
 *               samples   from the level's (gradient, theta) plane: sptx = W/4, spty = H/4; cell (ix, iy), 0..3 each,
 *                         has its centre c at (X + sptx (ix + 0.5), Y + spty (iy + 0.5)) and the pixel centres from
 *                         floor(c - spt) + 0.5 to floor(c + spt) + 0.5 per axis, clipped to [1.5, width - 1.5] x
 *                         [1.5, height - 1.5]; a sample counts where |nx| < 1 and |ny| < 1, nx = (x - cx)/sptx,
 *                         ny = (y - cy)/spty, with weight (1 - |nx|)(1 - |ny|) gradient -- no Gaussian weight, no
 *                         rotation, desc_window_factor unread (the reference passes it and never reads it);
 *               bins      t = -theta 4/pi, + 8 where negative; the weight is split between bin floor(t) and the next
 *                         by the fractional part, bin 8 is bin 0; t == 8.0 as a binary32 number is dropped, or goes to
 *                         bin 8 with dynamic_indexing (the rule of hess_params.dynamic_indexing); half_sift folds bin
 *                         k + 4 into bin k; components as in every descriptor: cell iy 4 + ix, then bin;
 *               W quantised to 0 or H equal to 0: every test is false, the empty window;
 *               normalisation and HESS_DESC_FORMAT_U8 as for every descriptor (the empty window: 1/sqrt(dim), or
 *               zeros with normalize = 0);
 *               returned: hess_count == num, the caller's keys byte for byte in input order (no orientation pass and no
 *               download, whatever max_orientation and fixed_orientation say), descriptors in input order.
 *               hess_params.descriptor_order selects nothing in this mode.  One kernel for every pixel type
 *               (descriptor_rect_kernel, csrc/k_feature.hip, whose header states the binary32 expressions): a bin's sum
 *               is formed per raster column first (columns xlo + 64 k + lane of the rectangle's box, band k after band
 *               k - 1, rows downwards), then over the 64 lanes in a fixed order (two sequential 32-lane sums starting
 *               at lane (8 ix + bin) mod 32 of each half, added) -- a function of the rectangle and the plane alone,
 *               the same bits whatever the list's length or order. */
enum { HESS_KEYS_NONE = 0, HESS_KEYS_ORIENTED = 1, HESS_KEYS_RECTANGLES = -1 };

/* Replaces SiftGPU::SetKeypointList -> SiftPyramid::SetKeypointList (SiftPyramid.cpp:326-355): the
 * NEXT hess_run_* call (one image) skips detection and computes orientation (unless
 * keys_have_orientation) and descriptors for these keypoints (PyramidCU::GenerateFeatureListTex,
 * PyramidCU.cpp:555-718); results come back in input order; the list is cleared afterwards.
 * HESS_ERR_STATE while a submitted batch is pending.
 * keys_have_orientation: HESS_KEYS_NONE, HESS_KEYS_ORIENTED (any non-zero value but -1) or HESS_KEYS_RECTANGLES. */
int hess_set_keypoints(hess_ctx* ctx, const hess_keypoint* keys, int num, int keys_have_orientation);
/* Replaces SiftGPU::RunSIFT(num, keys, keys_have_orientation) (SiftGPU.cpp:307-315): the same on the
 * CURRENT image (first image of the last run) without rebuilding the pyramid. */
int hess_run_keypoints(hess_ctx* ctx, const hess_keypoint* keys, int num, int keys_have_orientation);

/* Keypoint lists for every image of a batch (no reference counterpart: its list belongs to the one image it holds).
 * keys: the lists back to back, counts[b] >= 0 keys for image b (0: that image has no results), nimg images.  The NEXT
 * hess_run_host / hess_run_device / hess_submit_host / hess_submit_device must have batch == nimg: any other batch fails
 * with HESS_ERR_ARG and a text naming both numbers before anything is enqueued, and the lists stay pending.  The keys are
 * copied by the call; they are binned to levels on the device (key_bin_kernel, csrc/k_feature.hip: the scale rule of
 * hess_set_keypoints, the same bits), so a submitted list batch overlaps with the batches of other contexts like any
 * other.  Per image everything is as after hess_set_keypoints with that image alone: hess_count(b) == counts[b], keys
 * and descriptors in input order (zeros for a key whose scale is NaN), keys_have_orientation as there
 * (HESS_KEYS_RECTANGLES included); the lists are cleared by the run.  A total of 0 keys clears pending lists.
 *   HESS_ERR_ARG    ctx or counts NULL, nimg <= 0, a negative count, keys NULL with a total above 0
 *   HESS_ERR_STATE  a submitted batch is pending, or a hess_debug_key_levels override is (the hook covers the list of a
 *                   single image: hess_set_keypoints) */
int hess_set_keypoints_batch(hess_ctx* ctx, const hess_keypoint* keys, const int* counts, int nimg, int keys_have_orientation);
/* The same on the CURRENT batch, whose pyramids are resident, without rebuilding them (hess_run_keypoints for every image
 * of the last run): nimg must equal the batch of the last run (HESS_ERR_ARG otherwise; HESS_ERR_STATE without a current
 * batch), the total must be above 0.  The descriptor format is the one set now, as for hess_run_keypoints. */
int hess_run_keypoints_batch(hess_ctx* ctx, const hess_keypoint* keys, const int* counts, int nimg, int keys_have_orientation);
/* After a keypoint-list run (any of the four calls above): the LIST of image img -- its keys in the order the device holds
 * their records: level index ascending, then input index ascending; a key is listed once, twice where the rounded bounds
 * of two neighbouring levels overlap at its scale, or not at all (a NaN scale).  Returns the list's length and writes up
 * to cap entries of the map list position -> input index (0 .. count - 1 of that image) to out (out may be NULL with
 * cap == 0).  hess_device_results after such a run hands out list-order records, which this map assigns to the caller's
 * keys.  HESS_ERR_STATE when the last run had no list. */
int hess_key_list_order(hess_ctx* ctx, int img, int* out, int cap);

/* Replaces SiftGPU::GetFeatureNum (SiftGPU.cpp:1551-1554) for image `img` of the last batch. */
int hess_count(hess_ctx* ctx, int img);
/* Descriptor length of the last run in ELEMENTS, whatever the format: 128, 64 (-half) or 0 (-sd). */
int hess_desc_dim(hess_ctx* ctx);
/* Replaces SiftGPU::GetFeatureVector -> SiftPyramid::CopyFeatureVector (SiftPyramid.cpp:313-324).
 * Either output may be NULL.  keys: hess_count() records; desc: hess_count()*hess_desc_dim() floats.
 * After a HESS_DESC_FORMAT_U8 run: HESS_ERR_STATE, nothing written (hess_fetch_u8 is the call; nothing converts). */
int hess_fetch(hess_ctx* ctx, int img, hess_keypoint* keys, float* desc);

/* Descriptor output format of a context.  F32 (the default): float[dim] per feature, as always.  U8: the descriptor
 * kernels store dim BYTES per feature -- what the matcher, SiftMatchGPU::SetDescriptors and the .sift files take -- and
 * everything behind them carries bytes: device and pinned result buffers, every delivery, hess_fetch_u8,
 * hess_device_results, hess_matcher_bank_set_device_u8.  A quarter of the result bytes in HBM and over the host link.
 *   byte = low byte of (int)((double)(512.0f * d) + 0.5)      (product in float, sum in double, truncation)
 * -- the matcher's own rule (hess_matcher_set_descriptors_f32, SiftMatchCU.cpp:88-100), so a bank built from byte
 * results is byte-equal to the bank built from the float results of the same images.  The low byte WRAPS, as it does
 * there: d >= 0.49902 (512 d + 0.5 >= 256) wraps, d = 1.0 gives byte 0; normalised descriptors are clamped to 0.2
 * before the second normalisation and stay far below that in practice.
 * hess_set_descriptor_format applies to the FOLLOWING runs (keypoint-list runs included) and may be changed between
 * runs in both directions; the results of the run before stay fetchable in their own format.
 *   HESS_ERR_ARG          ctx NULL, or a format that is neither
 *   HESS_ERR_STATE        a submitted batch is pending (call hess_wait first)
 *   HESS_ERR_UNSUPPORTED  U8 with hess_params.normalize == 0 (unbounded values), or on a context whose results are
 *                         shared (hess_share_results, which in turn refuses a U8 context)
 * hess_desc_format: the format of the last run (of the following runs while the context has not run yet).
 * hess_fetch_u8: as hess_fetch after a U8 run; desc gets exactly hess_count() * hess_desc_dim() bytes.  After an F32
 * run: HESS_ERR_STATE, nothing written. */
enum { HESS_DESC_FORMAT_F32 = 0, HESS_DESC_FORMAT_U8 = 1 };
int hess_set_descriptor_format(hess_ctx* ctx, int format);
int hess_desc_format(hess_ctx* ctx);
int hess_fetch_u8(hess_ctx* ctx, int img, hess_keypoint* keys, unsigned char* desc);

/* Device-resident results of the last run, for consumers that stay on the GPU (the multi-GPU
 * gather over RCCL): keys = [total] hess_keypoint, desc = [total][dim] float -- unsigned char [total][dim] after a
 * HESS_DESC_FORMAT_U8 run (hess_desc_format tells) --, the images of the
 * batch back to back (image b starts at hess_count(0)+..+hess_count(b-1)); *total = records in use.
 * After a keypoint-list run the records are in LIST order, not in the caller's: image b starts at the sum of the list
 * lengths of the images before it, and hess_key_list_order gives each list's length and its map to the caller's keys
 * (hess_count and hess_fetch speak of the input order).
 * Pointers stay valid until the next run. */
int hess_device_results(hess_ctx* ctx, const void** keys, const void** desc, int* total);

/* Pyramid geometry of the last run (PyramidCU.cpp:238-245,274-309): number of octaves, and per
 * octave the aligned width / height. Arrays must hold >= 32 entries. Returns octave count. */
int hess_geometry(hess_ctx* ctx, int* widths, int* heights);

/* Parity hooks (no reference counterpart; reference has only the GL viewer's level display). */
int hess_debug_level(hess_ctx* ctx, int img, int octave, int level, int what, float* out);
/* Parity hook for the reference's feature file (tests/test_reference_fixture.py): describe user keypoint k
 * at level index levels[k] = octave*dog_level_num + (level-1) instead of the level the scale rule of
 * GenerateFeatureListTex picks (-1 keeps the rule; NULL/0 clears).  Applies to the NEXT keypoint-list run only
 * (hess_set_keypoints + hess_run_*, or hess_run_keypoints) and is cleared by it. */
int hess_debug_key_levels(hess_ctx* ctx, const int* levels, int num);
/* Robustness hook: how many times this context has grown its feature storage after an overflow and run a batch
 * again (the reference grows its lists per image, PyramidCU.cpp:393-397).  In the developer build the environment
 * variable HESS_INITIAL_CAP=<n> makes a new context start with room for n detections per image so that tests can force it. */
int hess_debug_regrown(hess_ctx* ctx);
/* Parity hook: the top Gaussian level of every octave (level dog+1) is nobody's input -- the launch that produces it
 * computes its det-Hessian from the output tile and does NOT write the level to HBM (the reference materialises it,
 * PyramidCU.cpp:1486-1558, and reads it back once, :1576-1591).  on != 0: the following runs of this context store it
 * as well, so that hess_debug_level(HESS_DBG_GAUSS, level dog+1) can return it (HESS_ERR_STATE otherwise).  With
 * HESS_DETECTOR_DOG the top level is dog+2 and the same rule applies to it. */
int hess_debug_keep_levels(hess_ctx* ctx, int on);

/* Multi-process jobs on one node (one process per GPU): keep this context's pinned host result buffers in
 * POSIX shared memory so that another process of the node -- the rank that collects the global batch -- reads them in
 * place.  Every GPU then delivers over its own host link; nothing is funnelled through the collecting rank's.
 *   "/<name>.h"      4096-byte directory: { u32 magic 'HESS', u32 gen_keys, u32 gen_desc, u32 pad, u64 keys_bytes, u64 desc_bytes }
 *   "/<name>.k<gen>" keypoint records of the last batch, images back to back (hess_keypoint[total])
 *   "/<name>.d<gen>" descriptors of the last batch (float[total][dim])
 * A generation number grows when a buffer is reallocated (a reader re-maps when it changes; the old object is
 * unlinked).  The per-image counts travel by the job's own control channel (hess_count); the data of a batch is
 * complete when hess_wait / hess_run_* has returned and stays until the context's next batch is submitted.
 * Call after hess_create, before the first batch; the objects are unlinked by hess_destroy.  name: no '/'.
 * Float descriptors only: HESS_ERR_UNSUPPORTED on a context set to HESS_DESC_FORMAT_U8. */
int hess_share_results(hess_ctx* ctx, const char* name);
int hess_shared_results_info(hess_ctx* ctx, unsigned* gen_keys, unsigned* gen_desc, size_t* keys_bytes, size_t* desc_bytes);
/* Raw detections of image `img` in list order; returns the count (<= cap written). */
int hess_debug_list(hess_ctx* ctx, int img, hess_rawkey* out, int cap);

/* Stage times of the last hess_run_* in ms, HESS_T_COUNT floats (SiftGPU::_timing, config.h:17-31). */
const float* hess_timing(hess_ctx* ctx);
const char* hess_last_error(hess_ctx* ctx);

/* Per-kernel device-time accounting (hipEvents on the context's stream) for bench.py's
 * roofline leg.  Off by default.  Kernel ids: HESS_K_*.  HESS_K_GAUSS_OCT0 repeats the Gaussian launches that work on
 * octave 0 (they are counted in HESS_K_GAUSS as well): the launches large enough to be bound by memory bandwidth
 * rather than by the latency of the dependent chain. */
enum { HESS_K_GAUSS = 0, HESS_K_DOWNSAMPLE, HESS_K_HESSIAN, HESS_K_EXTREMA, HESS_K_TOPK,
       HESS_K_ORIENT, HESS_K_DESCRIPTOR, HESS_K_INPUT, HESS_K_GAUSS_OCT0, HESS_K_COUNT };
int hess_profile_enable(hess_ctx* ctx, int on);
/* Accumulated since the last hess_profile_reset: total ms, launches, algorithmic bytes. */
int hess_profile_get(hess_ctx* ctx, int kernel, double* ms, long long* launches, double* bytes);
int hess_profile_reset(hess_ctx* ctx);
/* Bytes of the REFERENCE's array layout (every array written once and read once) that the launches counted
 * under `kernel` neither wrote nor read because the array never left LDS: the octave's top Gaussian level (its det-H
 * comes out of the launch that produces it) and level 0 of octave 0 of a u8 image -- 8 bytes per pixel each.
 * hess_profile_get's bytes are what the launches have to move; bytes + this = the layout's figure. */
int hess_profile_get_in_lds(hess_ctx* ctx, int kernel, double* bytes);

/* ---- Descriptor matcher: replaces SiftMatchGPU's CUDA flavour, SiftMatchCU
 * (SiftMatchCU.cpp:71-176) and MultiplyDescriptor(_G)_Kernel / RowMatch_Kernel / ColMatch_Kernel
 * (ProgramCU.cu:3455-3843).  Descriptors: num x dim unsigned bytes (512*d rounded), dim = 128 unless
 * hess_matcher_set_dim says 64; locations: (x,y). */
typedef struct hess_matcher hess_matcher;
hess_matcher* hess_matcher_create(int device, int max_sift);          /* SiftMatchGPU(max_sift) */
void hess_matcher_destroy(hess_matcher* m);
int hess_matcher_set_max(hess_matcher* m, int max_sift);              /* SetMaxSift */
/* Descriptor length: 128 (a new matcher) or 64, the unsigned-gradient descriptors of a half_sift (-half) run.  From then
 * on EVERY descriptor argument of every matcher entry point is [n][dim]: hess_matcher_set_descriptors / _f32,
 * hess_matcher_bank_set / _set_f32 / _set_device / _set_device_u8 (at 64 exactly what hess_device_results hands out after
 * a half_sift run: 64 floats or 64 bytes per feature) and hess_matcher_bank_read.  Pointer checks, truncation to
 * max_sift, the quantisation rule, matching (unguided, guided, match_pairs) and locations are the same at either length;
 * the result for 64-d sets is what the 128-d matcher returns for the same rows with 64 zero columns appended.
 * Setting the current dim is a no-op and the sets stay.  Setting the other one EMPTIES the bank, both single-pair slots
 * and their locations (their rows have the other pitch): load them again.  Any other value: HESS_ERR_ARG, with
 * hess_matcher_last_error naming it, and the matcher unchanged.  NULL matcher: HESS_ERR_ARG. */
int hess_matcher_set_dim(hess_matcher* m, int dim);
int hess_matcher_dim(hess_matcher* m);                                /* 128 or 64; NULL: HESS_ERR_ARG */
int hess_matcher_set_descriptors(hess_matcher* m, int index, int num, const unsigned char* des);
int hess_matcher_set_descriptors_f32(hess_matcher* m, int index, int num, const float* des);
int hess_matcher_set_locations(hess_matcher* m, int index, const float* locations, int gap);
/* GetSiftMatch (H = F = NULL) / GetGuidedSiftMatch; pairs: max_match x 2 ints; returns #matches. */
int hess_matcher_match(hess_matcher* m, int max_match, int* pairs, const float* H, const float* F,
                       float distmax, float ratiomax, float hdistmax, float fdistmax, int mutual_best);

/* Batched matching (no reference counterpart): a BANK of descriptor sets stays on the device and one call matches a
 * list of (a, b) pairs of it.  Independent of the two single-pair slots above.  Loading a bank replaces the previous
 * one; each set is truncated to max_sift as hess_matcher_set_descriptors does (at load time).  Rows of dim bytes or floats (hess_matcher_set_dim;
 * "128" below is the default dim).  counts[s]: descriptors of set s; the sets lie back to back in `des` (u8 or host floats, quantised as _f32 does). */
int hess_matcher_bank_set(hess_matcher* m, int nsets, const int* counts, const unsigned char* des);
int hess_matcher_bank_set_f32(hess_matcher* m, int nsets, const int* counts, const float* des);
/* dev_desc: float [sum of counts][128] in device memory of the matcher's device -- e.g. what hess_device_results hands
 * out, with counts from hess_count.  Quantised on the device, bit-identical to the host conversion.  The caller must have
 * waited for the run that produced the descriptors (hess_wait / hess_run_*); the call returns when the bank is built,
 * so the context's next run may start at once.  A pointer that is not device memory of that device: HESS_ERR_ARG. */
int hess_matcher_bank_set_device(hess_matcher* m, int nsets, const int* counts, const float* dev_desc);
/* The same from device BYTES, unsigned char [sum of counts][128] (hess_device_results after a HESS_DESC_FORMAT_U8 run):
 * stored as they are.  Same pointer check (4-byte alignment here), truncation to max_sift and return-when-built. */
int hess_matcher_bank_set_device_u8(hess_matcher* m, int nsets, const int* counts, const unsigned char* dev_desc);
/* The stored bytes of set `set` (its count x 128; out may be NULL).  Returns the count. */
int hess_matcher_bank_read(hess_matcher* m, int set, unsigned char* out);
/* Unguided GetSiftMatch for every pair p: set 1 = bank[pairs_ab[2p]], set 2 = bank[pairs_ab[2p+1]].  Pair p's result is
 * what hess_matcher_match(max_match, H = F = NULL, distmax, ratiomax, mutual_best) returns for those two sets:
 * out_counts[p] matches in out_pairs[p][0 .. out_counts[p]) of the caller's [npairs][max_match][2] ints.  Pairs may
 * repeat, be reversed or (a, a).  A set index outside the bank: HESS_ERR_ARG, nothing launched.  Returns 0 or a
 * negative hess_status; hess_matcher_last_ms: device time of all the call's kernels. */
int hess_matcher_match_pairs(hess_matcher* m, int npairs, const int* pairs_ab, int max_match, int* out_pairs,
                             int* out_counts, float distmax, float ratiomax, int mutual_best);
/* GetGuidedSiftMatch for every pair p of a list, each with its own geometry geo[p] (3x3 row-major H and F and their bounds:
 * what hess_matcher_estimate_pairs returns goes straight in).  Pair p = (a, b) returns, bit for bit, what
 * hess_matcher_match(max_match, geo[p].H, geo[p].F, distmax, ratiomax, geo[p].hdistmax, geo[p].fdistmax, mutual_best)
 * returns with slot 0 = bank[a] and slot 1 = bank[b], each with its locations (hess_matcher_bank_set_locations*) --
 * the rule of the 8-row blocks, the clamp at 0, the tie order and the truncation to max_match included.  Output as for
 * hess_matcher_match_pairs.  Pairs may repeat, be reversed or (a, a); the geometry belongs to the position p, not to
 * (a, b).  A matrix that is all zero gives its pair no match, as in the single-pair call; so does, here, a matrix with a
 * non-finite entry; neither disturbs another pair.  A caller with one matrix passes the identity with a bound of 1e20 for
 * the other (SiftMatchGPU::GetGuidedSiftMatch's rule).
 * Errors launch nothing and leave the matcher as it was: the bank has no locations: HESS_ERR_STATE; the bank has
 * feature types: HESS_ERR_UNSUPPORTED (guided matching with types is not built); geo NULL with npairs > 0, or a set
 * index outside the bank: HESS_ERR_ARG.  hess_matcher_last_ms: device time of all the call's kernels.
 * Added during version 5 without a bump: a matcher that never calls it behaves as before. */
typedef struct hess_guided_pair { float H[9], F[9]; float hdistmax, fdistmax; } hess_guided_pair;  /* 80 bytes */
int hess_matcher_match_pairs_guided(hess_matcher* m, int npairs, const int* pairs_ab, const hess_guided_pair* geo,
                                    int max_match, int* out_pairs, int* out_counts,
                                    float distmax, float ratiomax, int mutual_best);

/* Feature types (no reference counterpart in the matcher; the detector's README: "features of different types should
 * not be considered for a correspondence").  Class of a feature = type & 3 (hess_keypoint.type: 0 dark, 1 bright,
 * 2 saddle, 3 none; higher bits are ignored).  With types on both single-pair slots hess_matcher_match (H = F = NULL),
 * and with types on the bank hess_matcher_match_pairs, return the GATED match G of a pair:
 *   1. per class c, the ungated match (same thresholds, no limit) of the rows of set 1 of class c against the rows of
 *      set 2 of class c, each in ascending original order;
 *   2. the indices mapped back to the original rows, the union in ascending row of set 1;
 *   3. the first max_match of them.
 * Best, second best, the ratio test and mutual best see same-class features only, and the reference's tie order applies
 * to a column's position within its class subset.  This is not what discarding mixed pairs from the ungated result
 * gives.  A typed set is stored grouped by class on the device; hess_matcher_bank_read returns the caller's order.
 *
 * types: one value per descriptor, stride_bytes apart (&keys[0].type with sizeof(hess_keypoint), or a packed array with
 * 2), as the caller counted them when the descriptors were loaded: for the bank the sets back to back, each truncated
 * to max_sift as its descriptors were.  NULL removes the types (results are the ungated ones again).  Loading
 * descriptors (hess_matcher_set_descriptors* on a slot, hess_matcher_bank_set* on the bank) removes that slot's or the
 * bank's types; hess_matcher_set_dim to the other length removes everything.  A matcher that never calls these
 * behaves as before.  The device form takes device memory of the matcher's device, 2-byte aligned, with the pointer
 * check and error of hess_matcher_bank_set_device -- meant for (const char*)keys + offsetof(hess_keypoint, type) of
 * hess_device_results with stride sizeof(hess_keypoint).  All three return when the sets are ready.
 *   HESS_ERR_STATE        types before the descriptors they belong to; hess_matcher_match with exactly one slot typed
 *   HESS_ERR_ARG          stride_bytes odd or below 2; index not 0 or 1; a bad device pointer
 *   HESS_ERR_UNSUPPORTED  hess_matcher_match with H or F while either slot has types: guided matching with types is
 *                         NOT built (the types are never ignored silently: remove them first)
 * hess_matcher_last_error names the argument; the matcher is unchanged after an error. */
int hess_matcher_set_types(hess_matcher* m, int index, const uint16_t* types, size_t stride_bytes);
int hess_matcher_bank_set_types(hess_matcher* m, const uint16_t* types, size_t stride_bytes);
int hess_matcher_bank_set_types_device(hess_matcher* m, const void* dev_types, size_t stride_bytes);

/* ---- Two-view geometry from matches (no reference counterpart): the step between GetSiftMatch and GetGuidedSiftMatch.
 * A deterministic RANSAC with a fixed budget of T hypotheses for a homography H or a fundamental matrix F, on the
 * matcher's device and stream.  The result is a function of the inputs alone (locations, matches, params):
 *   1 sample   mix(x) on uint32: x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16.
 *              base = mix(seed ^ 0x9E3779B9), h_t = mix(base + t).  Draw j (0 <= j < k) of hypothesis t from n matches:
 *              c = (uint64(mix(h_t + j)) * (n - j)) >> 32, then for every earlier draw in ascending value: c++ if it is
 *              <= c.  k distinct indices into the match list, in draw order; k = 4 for H, 8 for F.  hess_geom_sample is this
 *              rule on the host (the kernel calls the same function).
 *   2 solve    in float32 from the k correspondences in Hartley-normalised coordinates (centroid to the origin, mean
 *              distance sqrt 2, per image): the null vector of the 8 x 9 DLT (H) or 8-point (F) matrix by Gauss-Jordan
 *              elimination with complete pivoting (the elimination alone in double), then back to pixel coordinates.  A
 *              hypothesis with a non-finite entry scores 0.
 *   3 score    the number of the pair's correspondences (x1, y1) -> (x2, y2) that pass the guided gate of
 *              hess_matcher_match with the hypothesis and `bound` (a division-free form of the same inequalities):
 *              H: x = H (x1, y1, 1), |x0 / x2 - x2| < bound and |x1 / x2 - y2| < bound;
 *              F: Sampson error (p2^T F p1)^2 / ((F p1)_0^2 + (F p1)_1^2 + (F^T p2)_0^2 + (F^T p2)_1^2) < bound.
 *   4 winner   the largest score, among equal scores the lowest t.  A largest score below k, or n < k (an empty pair
 *              included): no model -- hypothesis -1, inliers 0, M and the mask all zero, and the call still returns 0.
 *   5 result   M: the winner's matrix, for F first made rank 2 (its smallest singular value zeroed, in double), scaled to
 *              unit Frobenius norm.  inlier[i] = 1 exactly when correspondence i passes the gate's own formulas (with the
 *              division, in float32) on the returned M: the decision hess_matcher_match makes with M and `bound` as
 *              (H, hdistmax) or (F, fdistmax).  inliers counts the mask.  No early termination.
 *   6 refit    only with params.refit > 0 and a model: a least-squares refit on the inliers, at most `refit` times.  Let
 *              M0, S0 be the matrix and the mask of step 5.  For r = 1 .. refit:
 *              a. |S(r-1)| < k: stop.
 *              b. normalise: per image, over the correspondences of S(r-1), the centroid and the mean distance d to it;
 *                 the scale is sqrt 2 / d.  All in double from the float32 locations.  Either d zero or not finite: stop.
 *              c. N (9 x 9, symmetric, double) = the sum over S(r-1) of a a^T for the DLT rows of step 2 in these
 *                 normalised coordinates: H two rows per correspondence (x, y) -> (u, v), [x y 1 0 0 0 -ux -uy -u] and
 *                 [0 0 0 x y 1 -vx -vy -v]; F one row, [ux uy u vx vy v x y 1].
 *              d. candidate C: the unit eigenvector of N's smallest eigenvalue (in double), back in pixel coordinates
 *                 (T2^-1 X T1 for H, T2^T X T1 for F), made rank 2 (F) and of unit norm as in step 5, with the sign for
 *                 which sum_i C_i M(r-1)_i >= 0, rounded to float32.  A non-finite entry: stop.
 *              e. Sc = the gate's own decision on C (the formulas of step 5).  |Sc| < |S(r-1)|: C is discarded, stop.
 *                 Otherwise M(r) = C, S(r) = Sc; if Sc = S(r-1) as a set, stop after accepting (a further refit would
 *                 repeat it).
 *              The call returns the last accepted M and S: inliers counts that mask and is never below what refit = 0
 *              returns for the same inputs; hypothesis stays the RANSAC winner's index; the mask is still exactly what
 *              hess_matcher_match decides with the returned M and `bound`.  refits = the accepted refits, ransac_inliers
 *              = |S0|; both are zero with refit = 0 or without a model.  No floating-point atomics: every sum over the
 *              inliers is taken in one fixed order that depends on the match list and the mask alone, so the same inputs
 *              give the same bytes, run to run, alone or as a pair of a list.  Against exact arithmetic the candidate is
 *              promised within 8 x 2^-24 in Frobenius norm where lambda_9 / (lambda_2 - lambda_1) of N is at most 1e6;
 *              the bits of a particular order of summation are not part of the ABI.
 * Added during version 5 without a bump: a matcher that never calls these behaves as before.  `refit`, `refits` and
 * `ransac_inliers` were added during version 5 without a bump: `refit` 0 behaves as before. */
enum { HESS_GEOM_HOMOGRAPHY = 1, HESS_GEOM_FUNDAMENTAL = 2 };
typedef struct hess_geom_params {
  int32_t model;        /* HESS_GEOM_* */
  int32_t hypotheses;   /* T, 1..65536; 0 = 2048 */
  uint32_t seed;
  float bound;          /* HOMOGRAPHY: hdistmax of the guided gate; FUNDAMENTAL: fdistmax */
  union {
    int32_t reserved[4];  /* words 1..3 must be zero */
    struct {
      int32_t refit;      /* 0..8 refits on the inliers at the most (step 6; word 0 of reserved[]); 0: steps 1-5 alone */
      int32_t reserved_tail[3];
    };
  };
} hess_geom_params;
typedef struct hess_geom_result {
  float M[9];           /* row-major, unit Frobenius norm; all zero when there is no model */
  int32_t inliers;      /* set bytes of the mask */
  int32_t hypothesis;   /* index t of the winner, -1: no model */
  union {
    int32_t reserved[2];
    struct {
      int32_t refits;          /* accepted refits (word 0 of reserved[]) */
      int32_t ransac_inliers;  /* the inliers of step 5, before any refit (word 1); 0 with refit = 0 */
    };
  };
} hess_geom_result;

/* Host only: the k (1..8) indices of hypothesis t (>= 0) among n (>= k) matches into out[k].  0, or HESS_ERR_ARG. */
int hess_geom_sample(uint32_t seed, int t, int k, int n, int* out);
/* The two single-pair slots: pairs[i] = (row of slot 0, row of slot 1) as hess_matcher_match writes them, located by
 * hess_matcher_set_locations of both slots.  out: one result; inlier: nmatch bytes or NULL. */
int hess_matcher_estimate(hess_matcher* m, int nmatch, const int* pairs, const hess_geom_params* params,
                          hess_geom_result* out, unsigned char* inlier);
/* Locations of the bank's descriptors: one (x, y) float pair per descriptor, stride_bytes apart (a multiple of 4, at
 * least 8), the sets back to back as the caller counted them at load; each set is truncated to max_sift like its
 * descriptors.  They are kept in the caller's row order whatever hess_matcher_bank_set_types does to the storage: match
 * indices are the caller's.  The _device form reads device memory of the matcher's device (the key records of
 * hess_device_results with stride sizeof(hess_keypoint)) under the pointer check of hess_matcher_bank_set_device.
 * NULL removes them; so do hess_matcher_bank_set* and hess_matcher_set_dim to the other length. */
int hess_matcher_bank_set_locations(hess_matcher* m, const float* loc, size_t stride_bytes);
int hess_matcher_bank_set_locations_device(hess_matcher* m, const void* dev_loc, size_t stride_bytes);
/* Many pairs of the bank per call: pairs_ab[p] = (a, b), matches [npairs][max_match][2] and counts [npairs] exactly as
 * hess_matcher_match_pairs wrote them for those pairs.  Pair p uses seed + p (mod 2^32): out[p] and inlier[p][0..counts[p])
 * are what hess_matcher_estimate returns for that pair's locations, matches and seed; the rest of inlier[p] is zero.
 * One set of launches per chunk of pairs.
 *   HESS_ERR_STATE  a slot or the bank has no locations; bank locations before the bank's descriptors are loaded
 *   HESS_ERR_ARG    NULL params or out; an unknown model; hypotheses outside 0..65536; refit outside 0..8; non-zero
 *                   reserved words; bound not greater than 0 or not finite; a match index outside its set; a set index
 *                   outside the bank; counts[p] outside 0..max_match; a bad stride or device pointer
 * Nothing is launched on an error, the matcher is unchanged and hess_matcher_last_error names the argument.
 * hess_matcher_last_ms: device time of the call's kernels. */
int hess_matcher_estimate_pairs(hess_matcher* m, int npairs, const int* pairs_ab, int max_match, const int* matches,
                                const int* counts, const hess_geom_params* params, hess_geom_result* out,
                                unsigned char* inlier);

/* Geometrically verified matches for a list of bank pairs in one call: the unguided match, the estimate, the guided match
 * with each pair's own estimate and, optionally, the estimate on the guided matches -- per group of up to 256 pairs in
 * stream order on the device, with no host wait in between; only the results the caller asks for cross the host link.
 * THE RULE: for pair p = (a, b) the call returns, byte for byte, what this sequence of calls returns on the same matcher
 * state -- truncation to max_match, tie order, the rule of the 8-row blocks, seed + p and "never fewer inliers after a
 * refit" included:
 *   1. hess_matcher_match_pairs(pairs_ab, max_match, distmax, ratiomax, mutual_best): P_p with n_p matches
 *      (putative_pairs[p][0 .. n_p), out[p].nputative);
 *   2. hess_matcher_estimate_pairs(pairs_ab, max_match, P, n, &params->geom): out[p].putative;
 *   3. geo[p] from out[p].putative.M, the one-matrix rule of hess_matcher_match_pairs_guided: model HOMOGRAPHY H = M,
 *      hdistmax = guided_bound, F = identity, fdistmax = 1e20; model FUNDAMENTAL F = M, fdistmax = guided_bound,
 *      H = identity, hdistmax = 1e20 (guided_bound 0 stands for geom.bound).  A pair without a model has M all zero and
 *      therefore no guided match;
 *   4. hess_matcher_match_pairs_guided(pairs_ab, geo, max_match, distmax, ratiomax, mutual_best): out_pairs[p],
 *      out_counts[p] (= out[p].nguided);
 *   5. final_estimate 1: hess_matcher_estimate_pairs(pairs_ab, max_match, out_pairs, out_counts, &params->geom):
 *      out[p].final and inlier[p][0 .. out_counts[p]), the rest of inlier[p] zero.  final_estimate 0: out[p].final is the
 *      no-model result (M zero, inliers 0, hypothesis -1) and inlier is all zero.
 * inlier ([npairs][max_match] bytes) and putative_pairs ([npairs][max_match][2] ints) may be NULL: they are then not copied
 * and nothing else changes.  Pairs may repeat, be reversed or (a, a); p is the position in the list.
 * Errors launch nothing and leave the matcher as it was; hess_matcher_last_error names the argument:
 *   HESS_ERR_STATE        the bank has no locations
 *   HESS_ERR_UNSUPPORTED  the bank has feature types (guided matching with types is not built)
 *   HESS_ERR_ARG          NULL params, out, out_pairs or out_counts with npairs > 0; anything hess_matcher_estimate_pairs
 *                         refuses in params->geom; guided_bound negative or not finite; final_estimate not 0 or 1;
 *                         non-zero reserved words; a set index outside the bank; npairs or max_match < 0
 *   HESS_ERR_TOO_BIG      the scratch of one pair overflows, as in hess_matcher_match_pairs
 * npairs == 0 returns 0.  hess_matcher_last_ms: the sum of the kernel intervals of all chunks.
 * Added during version 5 without a bump: a matcher that never calls it behaves as before. */
typedef struct hess_verify_params {
  hess_geom_params geom;   /* model, hypotheses, seed, bound, refit: exactly as hess_matcher_estimate_pairs takes them */
  float distmax, ratiomax; /* both matches */
  int32_t mutual_best;
  float guided_bound;      /* bound of the guided gate for the estimated matrix; 0 = geom.bound */
  int32_t final_estimate;  /* 1: estimate again (same geom params, same seed + p) on the guided matches */
  int32_t reserved[3];     /* must be zero */
} hess_verify_params;      /* 64 bytes */
typedef struct hess_verify_result {
  hess_geom_result putative;  /* the estimate on the unguided matches */
  hess_geom_result final;     /* final_estimate = 1: the estimate on the returned matches; else all zero, hypothesis -1 */
  int32_t nputative;          /* matches of the unguided step (after the truncation to max_match) */
  int32_t nguided;            /* == out_counts[p] */
  int32_t reserved[4];
} hess_verify_result;         /* 128 bytes */
int hess_matcher_verify_pairs(hess_matcher* m, int npairs, const int* pairs_ab, const hess_verify_params* params,
                              int max_match, int* out_pairs, int* out_counts, hess_verify_result* out,
                              unsigned char* inlier /* [npairs][max_match] or NULL */,
                              int* putative_pairs /* [npairs][max_match][2] or NULL */);
float hess_matcher_last_ms(hess_matcher* m);   /* device time of the last match's kernels */
const char* hess_matcher_last_error(hess_matcher* m);

/* Test hook: evaluate one of the device's elementary functions (hess_devmath.h) on n inputs.
 * which: 0 exp(a) 1 atan2(a,b) 2 sin(a) 3 cos(a) 4 float->half bits 5 half bits->float 6 a/b 7 sqrt(a)
 * 8 the u8 -> [0,1] conversion a/255 for integer a in 0..255. */
int hess_math_probe(hess_ctx* ctx, int which, const float* a, const float* b, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* HESS_ABI_H */
