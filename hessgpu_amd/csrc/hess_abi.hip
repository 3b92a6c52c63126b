// hess_abi.hip -- the extern "C" entry points of include/hess_abi.h (see hess_ctx.h).
#include "hess_ctx.h"

// ================================== C ABI ====================================================

extern "C" {

void hess_default_params(hess_params* p) { if (p) default_params(p); }

int hess_dev_switches(void) {
#ifdef HESS_DEV_SWITCHES
  return 1;
#else
  return 0;
#endif
}

int hess_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// The environment of this moment into a context's switches (struct Switches says what each one means).
static void read_switches(Switches& sw) {
  if (const char* d = getenv("HESS_DELIVERY")) {
    if (!strcmp(d, "mirror")) sw.delivery_pref = kDeliverMirror;
    else if (!strcmp(d, "dma")) sw.delivery_pref = kDeliverDma;
    else if (!strcmp(d, "blit")) sw.delivery_pref = kDeliverBlit;
  }
  if (const char* m = dev_env("HESS_MIRROR_MAX_BATCH")) sw.mirror_max_batch = atoi(m);
  if (const char* e = dev_env("HESS_MIRROR_MAX_MB")) sw.mirror_max_bytes = (size_t)std::max(0, atoi(e)) << 20;
  if (const char* ci = dev_env("HESS_INITIAL_CAP")) sw.cap_init = atoi(ci) > 0 ? atoi(ci) : 0;
  sw.no_pair = dev_env("HESS_NO_PAIR") != nullptr;
  sw.no_top_fusion = dev_env("HESS_NO_TOP_FUSION") != nullptr;
  sw.no_first_fusion = dev_env("HESS_NO_FIRST_FUSION") != nullptr;
  if (const char* cf = dev_env("HESS_CHAIN_FROM")) sw.chain_from = atoi(cf);
  sw.no_host_upload = dev_env("HESS_NO_SIDE_UPLOAD") != nullptr;
  if (const char* dpn = dev_env("HESS_DESC_PARTS")) sw.desc_parts = atoi(dpn);
  if (const char* sr = dev_env("HESS_STREAM_ROWS")) sw.stream_rows = atoi(sr) > 0 ? (atoi(sr) / 3) * 3 : 0;
  if (const char* pb = dev_env("HESS_PX_BAND")) sw.desc_px_band = std::min(4096, std::max(64, atoi(pb)));
  if (const char* dx = dev_env("HESS_DESC_XCD")) sw.desc_xcd_block = atoi(dx) > 0 ? atoi(dx) : 0;
}

hess_ctx* hess_create(int device, const hess_params* params) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fprintf(stderr, "hessgpu: no usable HIP device %d (found %d)\n", device, ndev);
    return nullptr;
  }
  hess_ctx* c = new (std::nothrow) hess_ctx();
  if (!c) return nullptr;
  if (params) c->p = *params; else default_params(&c->p);
  c->device = device;
  bool ok = accept_params(&c->p);
  if (!ok) fprintf(stderr, "hessgpu: bad hess_params (abi_version %d)\n", c->p.abi_version);
  if (ok && !(ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->st.h, hipStreamNonBlocking) == hipSuccess))
    fprintf(stderr, "hessgpu: cannot create stream on device %d\n", device);
  if (ok) {
    for (Event& e : c->ev) ok = ok && hipEventCreate(&e.h) == hipSuccess;
    for (Event& e : c->ev_load) ok = ok && hipEventCreate(&e.h) == hipSuccess;
    if (!ok) fprintf(stderr, "hessgpu: cannot create events on device %d\n", device);
  }
  if (!ok) {  // the one way out: whatever exists by now frees itself
    delete c;
    return nullptr;
  }
  resolve(c);
  read_switches(c->sw);
  return c;
}

// A poisoned context (a DMA copy that was lost may still be in flight or land late) deliberately leaks the copy's
// sources and targets -- result buffers on both sides and the pixel staging area -- rather than hand memory that may
// still be written back to the allocator; a shared result buffer stays mapped for the same reason.
static void abandon_lost_copy_targets(hess_ctx* c) {
  for (DevBuf* b : {&c->keys, &c->desc, &c->stage, (DevBuf*)&c->h_keys, (DevBuf*)&c->h_desc, (DevBuf*)&c->h_kmap}) b->forget();
}

void hess_destroy(hess_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->st) (void)hipStreamSynchronize(c->st);
  copier_stop(c);
  stager_stop(c->sg);
  if (c->poisoned.load()) abandon_lost_copy_targets(c);
  if (c->share_dir) {
    (void)munmap(c->share_dir, 4096);
    char dir[256];
    snprintf(dir, sizeof(dir), "/%s.h", c->share.c_str());
    (void)shm_unlink(dir);
  }
  delete c;  // every buffer, event, signal and stream goes with its member (hess_ctx says in which order)
}

static int refuse_pending(hess_ctx* c) {
  if (c->run.active) { set_err(c, "a submitted batch is still pending: call hess_wait first"); return HESS_ERR_STATE; }
  return 0;
}

static int refuse_poisoned(hess_ctx* c) {
  if (!c->poisoned.load()) return 0;
  set_err(c, "the context is poisoned: a DMA copy did not complete and may still write its buffers; destroy the context");
  return HESS_ERR_DEVICE;
}

// The runtime objects a batch of this size will need are created by hess_reserve, not by the first batch: the copier
// thread and its binding to ROCr incl. the SDMA engine's queue (a 64-byte copy into each result buffer, only while the
// context holds no results), the hardware queue behind the context's stream -- and, once per reserved shape, ONE DRY
// BATCH of that shape on zeroed pixels, so that the first real batch finds the context in the state its second batch
// would (round 4's driver run: two of seven contexts ran their first batch inside a 20-step timed region; a first batch
// took 1.95 ms against 0.9).  The reference keeps allocation out of its steady-state numbers the same way
// (hessgpucmd.cpp:137-138,172: the first run is the allocating one).  The dry batch runs on a scratch image of its
// own (the staging area may hold the caller's last input, hess_last_input) and leaves no results behind.
// HESS_NO_PRIME_BATCH=1 switches it off (A/B).
static int prime(hess_ctx* c, int width, int height, int batch) {
  if (c->run.active) return 0;
  choose_delivery(c, batch);
  copier_warm_up(c);
  if (c->zeroed.p && c->zeroed.bytes >= 64) {
    HIP_TRY(c, hipMemsetAsync(c->zeroed.p, 0, 64, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
  }
  static const bool no_dry = dev_env("HESS_NO_PRIME_BATCH") != nullptr;
  const long long shape = ((long long)width << 40) ^ ((long long)height << 16) ^ batch;
  const bool primed = std::find(std::begin(c->primed_shapes), std::end(c->primed_shapes), shape) != std::end(c->primed_shapes);
  if (!no_dry && c->batch == 0 && !user_mode(c) && !primed) {
    // The scratch image belongs to the context (grow-only, freed with it): a hipMalloc / hipFree pair per call would
    // synchronise the whole device under the other contexts of a pipelining process.  The dry batch takes the settings of a
    // SUBMITTED batch (what a caller who reserves and then pipelines gets); a caller of hess_run_* with one or two images
    // takes the latency settings, whose first batch is then primed only as far as the two forms share launches.
    const size_t bytes = (size_t)batch * width * height;
    if (ensure(c, c->prime_px, bytes + 16)) { (void)hipGetLastError(); c->err.clear(); return 0; }  // no room for the scratch image: no dry batch
    void* const px = c->prime_px.p;
    int rc = 0;
    if (hipMemsetAsync(px, 0, bytes, c->st) != hipSuccess) rc = HESS_ERR_DEVICE;
    PendingRun r{.dev = px, .width = width, .height = height, .pitch = width, .batch = batch, .format = HESS_FMT_LUM,
                 .pixtype = HESS_PIX_U8, .image_stride = (size_t)width * height, .desc_format = c->desc_format};  // (a local: the stored run keeps its geometry)
    if (!rc) rc = submit_impl(c, r);
    if (!rc) rc = wait_impl(c, r);
    (void)hipStreamSynchronize(c->st);
    c->batch = c->pyramid_batch = 0;  // a dry batch leaves neither results nor a current image
    memset(c->timing, 0, sizeof(c->timing));
    // A dry batch that fails does not fail the reservation (the buffers exist; the first real batch will say what is
    // wrong, if anything still is) -- unless it poisoned the context, which refuse_poisoned() reports on the next call.
    if (rc) { (void)hipGetLastError(); return 0; }
    c->primed_shapes[c->primed_next++ % 4] = shape;  // the last four shapes: alternating shapes are primed once each
  }
  return 0;
}

int hess_reserve(hess_ctx* c, int width, int height, int batch) {
  if (!c || width <= 0 || height <= 0 || batch <= 0) return HESS_ERR_ARG;
  if (refuse_poisoned(c)) return HESS_ERR_DEVICE;
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = plan(c, width, height, batch);
  if (rc) return rc;
  return prime(c, width, height, batch);
}

static size_t pix_bytes(int pixtype) { return pixtype == HESS_PIX_U8 ? 1 : pixtype == HESS_PIX_U16 ? 2 : 4; }

// Everything a layout can be refused for is refused here, before anything is read or enqueued (include/hess_abi.h, above
// hess_run_host).  `device`: the pointer is dereferenced by the kernels themselves, so it must be aligned to the channel
// type; host pixels are copied bytewise into the context's own (aligned) staging area first.
static int check_run_args(hess_ctx* c, const void* pixels, int width, int height, int pitch, size_t image_stride, int batch,
                          int format, int pixtype, bool device) {
  if (!c) return HESS_ERR_ARG;
  if (refuse_poisoned(c)) return HESS_ERR_DEVICE;
  if (!pixels || width <= 0 || height <= 0 || batch <= 0 || pitch <= 0 || !fmt_channels(format) ||
      pixtype < HESS_PIX_U8 || pixtype > HESS_PIX_F32) {
    set_err(c, "bad argument");
    return HESS_ERR_ARG;
  }
  const size_t esz = pix_bytes(pixtype), row = (size_t)width * fmt_channels(format) * esz;
  if ((size_t)pitch < row) {
    set_err(c, "pitch %d is below the %zu bytes of one row (width * channels * bytes per channel): rows would overlap", pitch, row);
    return HESS_ERR_ARG;
  }
  if ((size_t)pitch % esz) {
    set_err(c, "pitch %d is not a multiple of the channel type's size %zu", pitch, esz);
    return HESS_ERR_ARG;
  }
  if (image_stride % esz) {
    set_err(c, "image_stride %zu is not a multiple of the channel type's size %zu", image_stride, esz);
    return HESS_ERR_ARG;
  }
  if (device && (uintptr_t)pixels % esz) {
    set_err(c, "dev_pixels %p is not aligned to the channel type's size %zu", pixels, esz);
    return HESS_ERR_ARG;
  }
  return 0;
}

// HESS_CHAIN_STAMPS=1 (diagnostics, stderr): per finished batch the device interval of its launch chain (first event to
// last event of the context's stream) and the host times of submit / wait return, all in ms since one base that is taken
// on both clocks when the first batch is submitted -- where do the contexts of a pipelined loop spend their time?
namespace {
struct ChainStamps {
  bool on = dev_env("HESS_CHAIN_STAMPS") && atoi(dev_env("HESS_CHAIN_STAMPS")) != 0;
  std::mutex mu;
  hipEvent_t base = nullptr;
  std::chrono::steady_clock::time_point host0;
  double now() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host0).count(); }
} g_stamps;
void chain_stamp_submit(hess_ctx* c, bool before) {
  if (!g_stamps.on) return;
  std::lock_guard<std::mutex> lk(g_stamps.mu);
  if (!g_stamps.base) {
    if (hipEventCreate(&g_stamps.base) != hipSuccess || hipEventRecord(g_stamps.base, c->st) != hipSuccess ||
        hipEventSynchronize(g_stamps.base) != hipSuccess) { g_stamps.on = false; return; }
    g_stamps.host0 = std::chrono::steady_clock::now();
  }
  (before ? c->stamp_submit0 : c->stamp_submit1) = g_stamps.now();
}
void chain_stamp_done(hess_ctx* c, double wait0) {
  if (!g_stamps.on || !g_stamps.base) return;
  float a = 0.0f, b = 0.0f;
  if (hipEventElapsedTime(&a, g_stamps.base, c->ev[0]) != hipSuccess || hipEventElapsedTime(&b, g_stamps.base, c->ev[7]) != hipSuccess) return;
  fprintf(stderr, "hess chain ctx %p: host submit %.3f - %.3f  device %.3f - %.3f  host wait %.3f - %.3f\n", (void*)c,
          c->stamp_submit0, c->stamp_submit1, (double)a, (double)b, wait0, g_stamps.now());
}
}  // namespace

// What hess_submit_* begin with: the checks; then the results and the pyramid of the run before are gone.
static int begin_submit(hess_ctx* c, const void* pixels, int width, int height, int pitch, size_t image_stride, int batch,
                        int format, int pixtype, bool device) {
  if (int rc = check_run_args(c, pixels, width, height, pitch, image_stride, batch, format, pixtype, device)) return rc;
  if (int rc = refuse_pending(c)) return rc;
  if (int rc = check_user_batch(c, batch)) return rc;  // (before anything is enqueued)
  HIP_TRY(c, hipSetDevice(c->device));
  c->batch = c->pyramid_batch = 0;
  c->accepted_submit = true;
  return 0;
}

int hess_submit_device(hess_ctx* c, const void* dev_pixels, int width, int height, int pitch, size_t image_stride,
                       int batch, int format, int pixtype) {
  int rc = begin_submit(c, dev_pixels, width, height, pitch, image_stride, batch, format, pixtype, true);
  if (rc) return rc;
  c->run = PendingRun{.dev = dev_pixels, .width = width, .height = height, .pitch = pitch, .batch = batch, .format = format,
                      .pixtype = pixtype, .image_stride = image_stride, .desc_format = c->desc_format};
  chain_stamp_submit(c, true);
  rc = submit_impl(c, c->run);
  chain_stamp_submit(c, false);
  if (rc) return rc;
  c->run.active = true;
  return 0;
}

int hess_wait(hess_ctx* c) {
  if (!c) return HESS_ERR_ARG;
  if (!c->run.active) { set_err(c, "nothing submitted"); return HESS_ERR_STATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  c->run.active = false;
  const double wait0 = g_stamps.on && g_stamps.base ? g_stamps.now() : 0.0;
  const int rc = wait_impl(c, c->run);
  if (!rc) chain_stamp_done(c, wait0);
  return rc;
}

int hess_run_device(hess_ctx* c, const void* dev_pixels, int width, int height, int pitch, size_t image_stride,
                    int batch, int format, int pixtype) {
  if (c) c->caller_waits = true;
  int rc = hess_submit_device(c, dev_pixels, width, height, pitch, image_stride, batch, format, pixtype);
  if (!rc) rc = hess_wait(c);
  if (c) c->caller_waits = false;
  return rc;
}

// Host pixels: one asynchronous host->device transfer on the context's stream, then the path.  Pinned caller
// memory (hipHostMalloc / hipHostRegister) is read by the copy engine directly; pageable memory is first copied
// into the context's pinned staging buffer by the calling thread -- while the device still works on the batches
// of other contexts -- so that the transfer itself never blocks the host or the other streams of the device
// (a hipMemcpyAsync from pageable memory does both).
int hess_submit_host(hess_ctx* c, const void* pixels, int width, int height, int pitch, size_t image_stride, int batch,
                     int format, int pixtype) {
  int rc = begin_submit(c, pixels, width, height, pitch, image_stride, batch, format, pixtype, false);
  if (rc) return rc;
  // From the first pixel to the last one and not a byte more: the last row's padding is not the caller's to give (a ROI
  // that ends in the last row of a frame, images side by side in one row of pitch bytes).  No kernel reads a row's padding.
  const size_t bytes = (size_t)(batch - 1) * image_stride + (size_t)(height - 1) * pitch +
                       (size_t)width * fmt_channels(format) * pix_bytes(pixtype);
  rc = ensure(c, c->stage, bytes + 16);
  if (rc) return rc;
  c->run = PendingRun{.dev = c->stage.p, .width = width, .height = height, .pitch = pitch, .batch = batch, .format = format,
                      .pixtype = pixtype, .image_stride = image_stride, .desc_format = c->desc_format};  // (the pixels will be in the staging area)
  hipPointerAttribute_t at;
  const bool pinned = hipPointerGetAttributes(&at, pixels) == hipSuccess && at.type == hipMemoryTypeHost;
  // The route (hess_copier.hip): pinned pixels of a batch the copier thread delivers are uploaded beside the queues, and that
  // thread submits the batch; everything else crosses on the context's stream, pageable pixels through the stager's threads.
  bool taken = false;
  if (pinned && (rc = upload_beside_queues(c, pixels, bytes, &taken))) return rc;
  if (taken) return 0;
  if ((rc = upload_on_stream(c, pixels, bytes, pinned))) return rc;
  rc = submit_impl(c, c->run);
  if (rc) return rc;
  c->run.active = true;
  return 0;
}

int hess_run_host(hess_ctx* c, const void* pixels, int width, int height, int pitch, size_t image_stride, int batch,
                  int format, int pixtype) {
  if (c) c->caller_waits = true;   // (a synchronous call has nothing to overlap the delivery with: choose_delivery, enqueue)
  int rc = hess_submit_host(c, pixels, width, height, pitch, image_stride, batch, format, pixtype);
  if (!rc) rc = hess_wait(c);      // (the flag stays up: pinned pixels are enqueued by the copier thread, during the wait)
  if (c) c->caller_waits = false;
  return rc;
}

int hess_last_input(hess_ctx* c, void* out, size_t bytes) {
  if (!c || !out) return HESS_ERR_ARG;
  if (refuse_pending(c)) return HESS_ERR_STATE;
  if (!c->last_input_bytes || bytes > c->last_input_bytes) { set_err(c, "no host input of that size is retained"); return HESS_ERR_STATE; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(out, c->stage.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The caller's key list for the next run (nothing thrown crosses the C ABI).
// The keys of `nimg` images, back to back, into the context's pinned block (the copy that the run uploads); a total of 0
// clears a pending list.  The stream is idle or busy with an earlier batch whose upload is long done: a run that uses the
// block is waited for before the next list can be set (the batch entries refuse while one is pending).
static int store_user_keys(hess_ctx* c, const hess_keypoint* keys, const int* counts, int nimg, int keys_have_orientation,
                           bool on_current) {
  long long total = 0;
  int most = 0;
  for (int b = 0; b < nimg; b++) { total += counts[b]; most = std::max(most, counts[b]); }
  if (total > (INT_MAX - 8) / 2) { set_err(c, "too many keypoints (%lld)", total); return HESS_ERR_ARG; }
  clear_user_list(c);
  if (total == 0) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure(c, c->h_user, user_block_bytes((int)total, nimg))) return rc;
  try {
    c->user_counts.assign(counts, counts + nimg);
  } catch (...) { c->user_counts.clear(); set_err(c, "out of host memory"); return HESS_ERR_NOMEM; }
  memcpy(c->h_user.p, keys, (size_t)total * sizeof(hess_keypoint));
  c->user_total = (int)total;
  c->user_max = most;
  c->user_have_orientation = keys_have_orientation != 0;  // the reference tests the flag's truth (PyramidCU.cpp:522) ...
  c->user_rect = keys_have_orientation == HESS_KEYS_RECTANGLES;  // ... and -1 alone for rectangles (SiftPyramid.cpp:345-354)
  c->user_on_current = on_current;
  return 0;
}

int hess_set_keypoints(hess_ctx* c, const hess_keypoint* keys, int num, int keys_have_orientation) {
  if (!c || num < 0 || (num > 0 && !keys)) return HESS_ERR_ARG;
  if (refuse_pending(c)) return HESS_ERR_STATE;  // (hess_wait tells a list run by the pending list, and its upload reads the block)
  return store_user_keys(c, keys, &num, 1, keys_have_orientation, false);
}

static int check_key_batch(hess_ctx* c, const hess_keypoint* keys, const int* counts, int nimg) {
  if (!c) return HESS_ERR_ARG;
  if (!counts || nimg <= 0) { set_err(c, "keypoint lists: counts of %d images", nimg); return HESS_ERR_ARG; }
  long long total = 0;
  for (int b = 0; b < nimg; b++) {
    if (counts[b] < 0) { set_err(c, "keypoint lists: image %d has a negative count (%d)", b, counts[b]); return HESS_ERR_ARG; }
    total += counts[b];
  }
  if (total > 0 && !keys) { set_err(c, "keypoint lists: no keys"); return HESS_ERR_ARG; }
  if (refuse_pending(c)) return HESS_ERR_STATE;
  if (!c->user_levels.empty()) {
    set_err(c, "a hess_debug_key_levels override is pending: it covers the list of a single image (hess_set_keypoints)");
    return HESS_ERR_STATE;
  }
  return 0;
}

int hess_set_keypoints_batch(hess_ctx* c, const hess_keypoint* keys, const int* counts, int nimg, int keys_have_orientation) {
  if (int rc = check_key_batch(c, keys, counts, nimg)) return rc;
  return store_user_keys(c, keys, counts, nimg, keys_have_orientation, false);
}

// The pending lists on the current batch's pyramid: `batch` images, no filtering.
static int run_on_current(hess_ctx* c, int batch) {
  PendingRun r = c->run;  // geometry of the current image (a local: the stored run keeps its batch)
  if (r.width <= 0) { clear_user_list(c); set_err(c, "no current image"); return HESS_ERR_STATE; }
  r.batch = batch; r.t_load_ms = 0.0;
  r.desc_format = c->desc_format;  // (the list's run takes the format set now, not the image's)
  const int keep_pyramid = c->pyramid_batch;
  c->batch = 0;  // results of the run before: gone; the pyramid stays (that is the point of this entry)
  int rc = submit_impl(c, r);
  if (rc) { clear_user_list(c); return rc; }
  rc = wait_impl(c, r);
  c->pyramid_batch = keep_pyramid;
  if (rc) clear_user_list(c);
  else c->run.desc_format = r.desc_format;  // the results the context now holds are this run's
  return rc;
}

int hess_run_keypoints(hess_ctx* c, const hess_keypoint* keys, int num, int keys_have_orientation) {
  if (!c || num <= 0 || !keys) return HESS_ERR_ARG;
  if (refuse_poisoned(c)) return HESS_ERR_DEVICE;
  if (!c->planned || c->pyramid_batch < 1) { set_err(c, "no current image: run an image first"); return HESS_ERR_STATE; }
  if (refuse_pending(c)) return HESS_ERR_STATE;
  if (int rc = store_user_keys(c, keys, &num, 1, keys_have_orientation, true)) return rc;
  return run_on_current(c, 1);
}

int hess_run_keypoints_batch(hess_ctx* c, const hess_keypoint* keys, const int* counts, int nimg, int keys_have_orientation) {
  if (int rc = check_key_batch(c, keys, counts, nimg)) return rc;
  if (refuse_poisoned(c)) return HESS_ERR_DEVICE;
  if (!c->planned || c->pyramid_batch < 1) { set_err(c, "no current batch: run a batch first"); return HESS_ERR_STATE; }
  if (nimg != c->pyramid_batch) {
    set_err(c, "keypoint lists for %d images, the current batch has %d", nimg, c->pyramid_batch);
    return HESS_ERR_ARG;
  }
  if (int rc = store_user_keys(c, keys, counts, nimg, keys_have_orientation, true)) return rc;
  if (!user_mode(c)) { set_err(c, "keypoint lists: no keys"); return HESS_ERR_ARG; }
  return run_on_current(c, nimg);
}

int hess_key_list_order(hess_ctx* c, int img, int* out, int cap) {
  if (!c || img < 0 || img >= c->batch || cap < 0 || (cap > 0 && !out)) return HESS_ERR_ARG;
  if (!c->user_result) { set_err(c, "the last run had no keypoint list"); return HESS_ERR_STATE; }
  const size_t first = c->offs[img], len = c->offs[img + 1] - first;
  const size_t m = std::min(len, (size_t)cap);
  if (m) memcpy(out, c->u_order.data() + first, m * sizeof(int));
  return (int)len;
}

int hess_debug_key_levels(hess_ctx* c, const int* levels, int num) {
  if (!c || num < 0) return HESS_ERR_ARG;
  c->user_levels.clear();
  try {
    if (levels && num > 0) c->user_levels.assign(levels, levels + num);
  } catch (...) { c->user_levels.clear(); set_err(c, "out of host memory"); return HESS_ERR_NOMEM; }
  return 0;
}

int hess_count(hess_ctx* c, int img) {
  if (!c || img < 0 || img >= c->batch) return HESS_ERR_ARG;
  return c->counts[img];
}

int hess_desc_dim(hess_ctx* c) { return c ? c->dim : HESS_ERR_ARG; }

static const char* desc_format_name(int format) { return format == HESS_DESC_FORMAT_U8 ? "u8" : "f32"; }

// hess_fetch / hess_fetch_u8: the results in the format they were made in, or nothing.
static int fetch_as(hess_ctx* c, int format, int img, hess_keypoint* keys, void* desc) {
  if (!c || img < 0 || img >= c->batch) return HESS_ERR_ARG;
  if (c->run.desc_format != format) {
    set_err(c, "the last run's descriptors are %s: fetch them with %s (nothing is converted)", desc_format_name(c->run.desc_format),
            c->run.desc_format == HESS_DESC_FORMAT_U8 ? "hess_fetch_u8" : "hess_fetch");
    return HESS_ERR_STATE;
  }
  const size_t n = (size_t)c->counts[img], db = run_desc_bytes(c, format);
  if (c->user_result) {
    const size_t first = c->u_first[img];  // (input order, the images back to back)
    if (keys && n) memcpy(keys, c->u_keys.data() + first, n * sizeof(hess_keypoint));
    if (desc && c->dim && n) memcpy(desc, c->u_desc.data() + first * db, n * db);
    return 0;
  }
  if (keys && n) memcpy(keys, (HostKeypoint*)c->h_keys.p + c->offs[img], n * sizeof(HostKeypoint));
  if (desc && c->dim && n) memcpy(desc, (const char*)c->h_desc.p + c->offs[img] * db, n * db);
  return 0;
}

int hess_fetch(hess_ctx* c, int img, hess_keypoint* keys, float* desc) { return fetch_as(c, HESS_DESC_FORMAT_F32, img, keys, desc); }
int hess_fetch_u8(hess_ctx* c, int img, hess_keypoint* keys, unsigned char* desc) { return fetch_as(c, HESS_DESC_FORMAT_U8, img, keys, desc); }

int hess_set_descriptor_format(hess_ctx* c, int format) {
  if (!c) return HESS_ERR_ARG;
  if (format != HESS_DESC_FORMAT_F32 && format != HESS_DESC_FORMAT_U8) {
    set_err(c, "hess_set_descriptor_format: %d is neither HESS_DESC_FORMAT_F32 nor HESS_DESC_FORMAT_U8", format);
    return HESS_ERR_ARG;
  }
  if (refuse_pending(c)) return HESS_ERR_STATE;
  if (format == HESS_DESC_FORMAT_U8 && !c->p.normalize) {
    set_err(c, "byte descriptors need normalised values (hess_params.normalize): unnormalised ones are unbounded");
    return HESS_ERR_UNSUPPORTED;
  }
  if (format == HESS_DESC_FORMAT_U8 && c->share_dir) {
    set_err(c, "byte descriptors are not available on a context whose results are shared (hess_share_results)");
    return HESS_ERR_UNSUPPORTED;
  }
  if (format != c->desc_format) {
    c->desc_format = format;  // (plan() sizes the result buffers of the next run by it: hess_ctx::planned_format)
    if (!c->batch) c->run.desc_format = format;  // no results to describe: hess_desc_format reports the runs to come
  }
  return 0;
}

int hess_desc_format(hess_ctx* c) { return c ? c->run.desc_format : HESS_ERR_ARG; }

int hess_device_results(hess_ctx* c, const void** keys, const void** desc, int* capacity) {
  if (!c || !c->batch) return HESS_ERR_STATE;
  if (keys) *keys = c->keys.p;
  if (desc) *desc = c->dim ? c->desc.p : nullptr;
  // records in use; image b starts at sum of counts < b (after a keypoint-list run: of the list lengths, hess_key_list_order)
  if (capacity) *capacity = (int)c->offs[c->batch];
  return 0;
}

int hess_geometry(hess_ctx* c, int* widths, int* heights) {
  if (!c || !c->planned) return HESS_ERR_STATE;
  for (int o = 0; o < c->g.noct; o++) {
    if (widths) widths[o] = c->g.o[o].wa;
    if (heights) heights[o] = c->g.o[o].h;
  }
  return c->g.noct;
}

int hess_debug_level(hess_ctx* c, int img, int octave, int level, int what, float* out) {
  if (!c || !c->planned || !out || img < 0 || img >= c->batch || octave < 0 || octave >= c->g.noct || level < 0 ||
      level > c->sch.level_max)
    return HESS_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  const OctGeom& og = c->g.o[octave];
  if (what == HESS_DBG_GAUSS && !c->keep_levels &&
      ((level == c->sch.level_max && !c->sw.no_top_fusion) || (level == 0 && octave == 0 && c->level0_in_lds))) {
    set_err(c, "this Gaussian level is not materialised (the octave's top level; level 0 of octave 0): call hess_debug_keep_levels before the run");
    return HESS_ERR_STATE;
  }
  if (what == HESS_DBG_GAUSS || what == HESS_DBG_DETH) {
    const float* base = (const float*)(what == HESS_DBG_GAUSS ? c->gauss.p : c->deth.p);
    const float* src = base + og.lvl_off + ((long long)level * c->g.B + img) * og.plane;
    HIP_TRY(c, hipMemcpy(out, src, (size_t)og.plane * 4, hipMemcpyDeviceToHost));
    return 0;
  }
  if (what == HESS_DBG_GOT) {
    if (level < 1 || level > c->g.dog) return HESS_ERR_ARG;
    const float* src = (const float*)c->got.p + 2 * (og.got_off + ((long long)(level - 1) * c->g.B + img) * og.plane);
    HIP_TRY(c, hipMemcpy(out, src, (size_t)og.plane * 8, hipMemcpyDeviceToHost));
    return 0;
  }
  return HESS_ERR_ARG;
}

int hess_debug_regrown(hess_ctx* c) { return c ? c->regrown : HESS_ERR_ARG; }

int hess_debug_keep_levels(hess_ctx* c, int on) {
  if (!c) return HESS_ERR_ARG;
  c->keep_levels = on != 0;
  return 0;
}

int hess_share_results(hess_ctx* c, const char* name) {
  if (!c) return HESS_ERR_ARG;
  if (!name || !name[0] || strlen(name) > 200 || strchr(name, '/')) {
    set_err(c, "hess_share_results: the name must be 1..200 characters without '/'");
    return HESS_ERR_ARG;
  }
  if (c->accepted_submit) { set_err(c, "hess_share_results: call before the context's first batch"); return HESS_ERR_ARG; }
  if (c->share_dir) { set_err(c, "the results of this context are shared already (as %s)", c->share.c_str()); return HESS_ERR_ARG; }
  if (c->desc_format == HESS_DESC_FORMAT_U8) {
    set_err(c, "hess_share_results: shared result buffers carry float descriptors; this context is set to byte descriptors");
    return HESS_ERR_UNSUPPORTED;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  char dir[256];
  snprintf(dir, sizeof(dir), "/%s.h", name);
  try {
    c->share = name;  // (nothing thrown crosses the C ABI)
  } catch (...) { set_err(c, "out of memory"); return HESS_ERR_NOMEM; }
  (void)shm_unlink(dir);
  for (unsigned gen = 1; gen <= 64; gen++) {  // buffers a crashed job of the same name left behind (the generations start at 1)
    char stale[256];
    snprintf(stale, sizeof(stale), "/%s.k%u", name, gen); (void)shm_unlink(stale);
    snprintf(stale, sizeof(stale), "/%s.d%u", name, gen); (void)shm_unlink(stale);
  }
  const int fd = shm_open(dir, O_CREAT | O_EXCL | O_RDWR, 0600);
  if (fd < 0) { set_err(c, "shm_open(%s) failed: %s", dir, strerror(errno)); c->share.clear(); return HESS_ERR_NOMEM; }
  void* m = ftruncate(fd, 4096) == 0 ? mmap(nullptr, 4096, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
  close(fd);
  if (m == MAP_FAILED) { set_err(c, "cannot map %s: %s", dir, strerror(errno)); shm_unlink(dir); c->share.clear(); return HESS_ERR_NOMEM; }
  memset(m, 0, 4096);
  c->share_dir = static_cast<hess_ctx::ShareDir*>(m);
  c->share_dir->magic = 0x48455353u;  // "HESS"
  c->h_keys.shared = 'k';  // from now on the two result buffers grow in shared memory (ensure -> ensure_shared)
  c->h_desc.shared = 'd';
  // results of an earlier run stay readable through hess_fetch only until the next run: the buffers move now
  if (c->st) HIP_TRY(c, hipStreamSynchronize(c->st));
  release(c->h_keys);
  release(c->h_desc);
  c->planned = false;
  c->batch = 0;
  return 0;
}

int hess_shared_results_info(hess_ctx* c, unsigned* gen_keys, unsigned* gen_desc, size_t* keys_bytes, size_t* desc_bytes) {
  if (!c || !c->share_dir) return HESS_ERR_ARG;
  if (gen_keys) *gen_keys = c->share_dir->gen_keys;
  if (gen_desc) *gen_desc = c->share_dir->gen_desc;
  if (keys_bytes) *keys_bytes = (size_t)c->share_dir->keys_bytes;
  if (desc_bytes) *desc_bytes = (size_t)c->share_dir->desc_bytes;
  return 0;
}

int hess_debug_list(hess_ctx* c, int img, hess_rawkey* out, int cap) {
  if (!c || !c->d_list || img < 0 || img >= c->batch) return HESS_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  int n = 0;
  HIP_TRY(c, hipMemcpy(&n, c->d_list_total + img, 4, hipMemcpyDeviceToHost));
  const int m = n < cap ? n : cap;
  static_assert(sizeof(hess_rawkey) == sizeof(RawKey), "raw key layout");
  if (out && m > 0)
    HIP_TRY(c, hipMemcpy(out, c->d_list + (size_t)img * c->cap_list, (size_t)m * sizeof(RawKey), hipMemcpyDeviceToHost));
  return n;
}

const float* hess_timing(hess_ctx* c) { return c ? c->timing : nullptr; }
const char* hess_last_error(hess_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hess_profile_enable(hess_ctx* c, int on) { if (!c) return HESS_ERR_ARG; c->prof = on != 0; return 0; }
int hess_profile_reset(hess_ctx* c) {
  if (!c) return HESS_ERR_ARG;
  memset(c->k_ms, 0, sizeof(c->k_ms));
  memset(c->k_n, 0, sizeof(c->k_n));
  memset(c->k_bytes, 0, sizeof(c->k_bytes));
  memset(c->k_in_lds, 0, sizeof(c->k_in_lds));
  return 0;
}
int hess_profile_get(hess_ctx* c, int kernel, double* ms, long long* launches, double* bytes) {
  if (!c || kernel < 0 || kernel >= HESS_K_COUNT) return HESS_ERR_ARG;
  if (ms) *ms = c->k_ms[kernel];
  if (launches) *launches = c->k_n[kernel];
  if (bytes) *bytes = c->k_bytes[kernel];
  return 0;
}

int hess_profile_get_in_lds(hess_ctx* c, int kernel, double* bytes) {
  if (!c || !bytes || kernel < 0 || kernel >= HESS_K_COUNT) return HESS_ERR_ARG;
  *bytes = c->k_in_lds[kernel];
  return 0;
}

// Device evaluation of the elementary functions (tests only; see hess_devmath.h).
int hess_math_probe(hess_ctx* c, int which, const float* a, const float* b, float* out, int n) {
  if (!c || !a || !out || n <= 0) return HESS_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  DevBuf da, db, dout;  // (freed on every way out)
  for (DevBuf* d : {&da, &db, &dout}) if (int rc = ensure(c, *d, (size_t)n * 4)) return rc;
  HIP_TRY(c, hipMemcpy(da.p, a, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(db.p, b ? b : a, (size_t)n * 4, hipMemcpyHostToDevice));
  launch_math_probe(c->st, which, (float*)da.p, (float*)db.p, (float*)dout.p, n);
  HIP_TRY(c, hipStreamSynchronize(c->st));
  HIP_TRY(c, hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
