// hess_copier.hip -- pixels in, results out: the input routes, the copier thread, submit / wait (see hess_ctx.h).
#include "hess_ctx.h"

namespace hess {

// ---- copier thread (kDeliverDma) ----
// One job at a time: wait on the host for the event behind the batch's last kernel, read the packed total from the
// pinned count block (stored there by feature_scan_kernel), copy exactly that many records on the copy-only stream.
std::atomic<int> g_copier_count{0};  // contexts with a copier, for spreading them over the preferred engines

// Bind the copier to ROCr: the agents that own the result buffers (from the pointers themselves), an SDMA engine of
// the set ROCr recommends for device->host on this pair of agents (contexts take turns), a completion signal.
static bool copier_hsa_setup(hess_ctx* c) {
  Copier& cp = c->cp;
  if (cp.hsa_ready) return true;
  if (cp.hsa_failed) return false;
  cp.hsa_failed = true;
  if (const char* m = dev_env("HESS_COPIER")) if (!strcmp(m, "hip")) return false;
  if (hsa_init() != HSA_STATUS_SUCCESS) return false;  // reference-counted: HIP has initialised ROCr already
  hsa_amd_pointer_info_t pi;
  memset(&pi, 0, sizeof(pi));
  pi.size = sizeof(pi);
  if (hsa_amd_pointer_info(c->keys.p, &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || pi.type == HSA_EXT_POINTER_TYPE_UNKNOWN) return false;
  cp.gpu_agent = pi.agentOwner;
  memset(&pi, 0, sizeof(pi));
  pi.size = sizeof(pi);
  // (the host side from the count block: always the runtime's own pinned allocation, also when the result buffers
  // are registered shared memory, whose owner ROCr reports differently)
  if (hsa_amd_pointer_info(c->h_small.p, &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || pi.type == HSA_EXT_POINTER_TYPE_UNKNOWN) return false;
  cp.cpu_agent = pi.agentOwner;
  if (hsa_signal_create(0, 0, nullptr, &cp.sig.h) != HSA_STATUS_SUCCESS) return false;
  if (hsa_signal_create(0, 0, nullptr, &cp.sig2.h) != HSA_STATUS_SUCCESS) return false;
  uint32_t pref = 0;
  if (hsa_amd_memory_get_preferred_copy_engine(cp.cpu_agent, cp.gpu_agent, &pref) == HSA_STATUS_SUCCESS && pref) {
    const int n = __builtin_popcount(pref), k = g_copier_count.fetch_add(1) % n;
    uint32_t m = pref;
    for (int i = 0; i < k; i++) m &= m - 1;
    cp.engine = m & (~m + 1);
  }
  // ... and an engine of the host->device set for the pixel uploads (left to ROCr, an upload sometimes lands on an engine
  // that copies at a quarter of the rate: the host-to-host figure varied 15 - 21 Gpix/s from run to run)
  uint32_t pref_in = 0;
  if (hsa_amd_memory_get_preferred_copy_engine(cp.gpu_agent, cp.cpu_agent, &pref_in) == HSA_STATUS_SUCCESS && pref_in) {
    const int n = __builtin_popcount(pref_in), k = g_copier_count.load() % n;
    uint32_t m = pref_in;
    for (int i = 0; i < k; i++) m &= m - 1;
    cp.engine_in = m & (~m + 1);
  }
  if (const char* e = dev_env("HESS_COPIER_ENGINE")) cp.engine = (uint32_t)strtoul(e, nullptr, 0);
  if (const char* e = dev_env("HESS_UPLOAD_ENGINE")) cp.engine_in = (uint32_t)strtoul(e, nullptr, 0);
  cp.hsa_failed = false;
  cp.hsa_ready = true;
  return true;
}

// Host wait for a copy's completion signal to drop below `below`, in slices of a second up to HESS_COPY_TIMEOUT_S
// (default 10): a lost completion must not hang hess_wait / hess_destroy (the reference returns 0 on device errors,
// SiftPyramid.h:162-163, it never hangs).  Returns 0 when the copies completed, 1 when the limit expired, 2 when ROCr
// reported a failed copy (it then leaves a NEGATIVE value in the signal); *last = the value seen.
// HESS_COPIER_FAULT=timeout|error makes the next wait of the process report that outcome (fault injection for the
// tests; the real signal is still waited for, so nothing is left in flight).  *real (if given) says whether the outcome
// is the signal's own: then the copy may still be in flight and the context is poisoned (HESS_COPIER_FAULT=poisoned
// reports a timeout as if it were real, after the copy has in fact completed).
std::atomic<int> g_copier_fault{-1};  // -1: not read yet, 0: none, 1: timeout, 2: error, 3: poisoned (consumed by the first wait)
static int wait_copy_signal(hsa_signal_t sig, hsa_signal_value_t below, hsa_signal_value_t* last, bool injectable, bool* real) {
  if (real) *real = false;
  static const double limit_s = [] { const char* e = getenv("HESS_COPY_TIMEOUT_S"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 10.0; }();
  static const uint64_t ticks_per_s = [] {
    uint64_t f = 0;
    return (hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &f) == HSA_STATUS_SUCCESS && f) ? f : (uint64_t)100000000;
  }();
  int inject = injectable ? g_copier_fault.load() : 0;
  if (injectable && inject < 0) {
    const char* e = dev_env("HESS_COPIER_FAULT");
    int want = !e ? 0 : (!strcmp(e, "timeout") ? 1 : (!strcmp(e, "error") ? 2 : (!strcmp(e, "poisoned") ? 3 : 0)));
    int expect = -1;
    if (!g_copier_fault.compare_exchange_strong(expect, want)) want = expect;
    inject = want;
  }
  const auto t0 = std::chrono::steady_clock::now();
  hsa_signal_value_t v;
  for (;;) {
    v = hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, below, ticks_per_s, HSA_WAIT_STATE_BLOCKED);
    if (v < below) break;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
      if (last) *last = v;
      if (real) *real = true;
      return 1;
    }
  }
  if (last) *last = v;
  if (inject > 0) {
    int expect = inject;
    if (g_copier_fault.compare_exchange_strong(expect, 0)) {
      if (inject == 3 && real) *real = true;
      return inject == 3 ? 1 : inject;
    }
  }
  if (v < 0 && real) *real = true;
  return v < 0 ? 2 : 0;
}

// ---- one SDMA copy through ROCr: start it, finish it ----
// Start: arm the copy's own signal with 1 (Copier::sig says why exactly that) and hand the copy to `engine` (0 = let ROCr
// choose).  Returns whether ROCr took the copy.
static bool sdma_start(uint32_t engine, void* dst, hsa_agent_t dst_agent, const void* src, hsa_agent_t src_agent, size_t bytes,
                       hsa_signal_t sig) {
  hsa_signal_store_relaxed(sig, 1);
  hsa_status_t st = engine ? hsa_amd_memory_async_copy_on_engine(dst, dst_agent, src, src_agent, bytes, 0, nullptr, sig,
                                                                 (hsa_amd_sdma_engine_id_t)engine, false)
                           : HSA_STATUS_ERROR;
  if (st != HSA_STATUS_SUCCESS)  // no engine chosen, or busy / not available: let ROCr choose
    st = hsa_amd_memory_async_copy(dst, dst_agent, src, src_agent, bytes, 0, nullptr, sig);
  return st == HSA_STATUS_SUCCESS;
}

// What a step of the copier thread returns: a hess_status and, unless that is 0, the message for hess_last_error.
struct Step {
  int rc = 0;
  char msg[256] = "";
};

static Step hip_failed(const char* what, hipError_t e) {
  Step s;
  snprintf(s.msg, sizeof(s.msg), "%s failed: %s (copier)", what, hipGetErrorString(e));
  s.rc = e == hipErrorOutOfMemory ? HESS_ERR_NOMEM : HESS_ERR_DEVICE;
  return s;
}

// Finish: wait for the copy.  0: it is done; 2: it did not complete (timeout or error; `msg` -- a Step's, or null -- says
// which of `what`, with `detail` behind the signal's value) -- and when that is the signal's own outcome the copy may still
// land: the context is poisoned (hess_ctx::poisoned).  What else a lost copy costs is the caller's to mark.
static int sdma_finish(hess_ctx* c, hsa_signal_t sig, const char* what, bool injectable, char* msg, const char* detail = "") {
  hsa_signal_value_t seen = 0;
  bool real = false;
  const int w = wait_copy_signal(sig, 1, &seen, injectable, &real);
  if (!w) return 0;
  if (msg) snprintf(msg, sizeof(Step::msg), "%s %s (signal value %lld%s)", what, w == 1 ? "did not complete in time" : "failed", (long long)seen, detail);
  if (real) c->poisoned.store(true);
  return 2;
}

// One or two blocks of device memory that travel together (keypoints and their descriptors; the lists' order).
struct HostBlock {
  void* dst;
  const void* src;
  size_t bytes;
  const char* hip_call;  // the name the stream copy fails under
};

// Bring the blocks to the pinned host buffers: by SDMA -- a copy that was taken and does not complete fails the batch; only
// the first wait can be `injectable` (HESS_COPIER_FAULT) -- or, where ROCr refuses a copy, by copies on the copy-only stream,
// which is then waited for.
static Step bring_to_host(hess_ctx* c, const HostBlock* b, int n, uint32_t engine, const char* what, const char* detail, bool injectable) {
  Copier& cp = c->cp;
  Step s;
  if (copier_hsa_setup(c) && sdma_start(engine, b[0].dst, cp.cpu_agent, b[0].src, cp.gpu_agent, b[0].bytes, cp.sig)) {
    const bool second = n > 1 && sdma_start(engine, b[1].dst, cp.cpu_agent, b[1].src, cp.gpu_agent, b[1].bytes, cp.sig2);
    // (both copies are in flight on the same engine; each has its own signal, and the second is waited for whatever the first did)
    int lost = sdma_finish(c, cp.sig, what, injectable, s.msg, detail);
    if (second && sdma_finish(c, cp.sig2, what, false, lost ? nullptr : s.msg, detail)) lost = 2;
    if (lost) {
      cp.hsa_ready = false; cp.hsa_failed = true;  // later batches take the stream copy; the signals are not reused,
      cp.sig.forget(); cp.sig2.forget();           // nor destroyed: a late copy may still write them
      s.rc = HESS_ERR_DEVICE;
    }
    if (lost || n == 1 || second) return s;  // failed, or the blocks are in host memory
    // ROCr took the first copy (done by now) and refused the second: the fallback copies both
  }
  hipError_t e;
  for (int i = 0; i < n; i++)
    if ((e = hipMemcpyAsync(b[i].dst, b[i].src, b[i].bytes, hipMemcpyDeviceToHost, cp.cs)) != hipSuccess) return hip_failed(b[i].hip_call, e);
  if ((e = hipStreamSynchronize(cp.cs)) != hipSuccess) return hip_failed("hipStreamSynchronize(copy stream)", e);
  return s;
}

// hess_reserve: the SDMA engine's queue is created by a 64-byte copy into each result buffer now, not by the first batch
// (only while the context holds no results and no job is posted).
void copier_warm_up(hess_ctx* c) {
  Copier& cp = c->cp;
  if (c->delivery != kDeliverDma || c->batch != 0 || !c->keys.p || !c->h_keys.p || c->h_keys.bytes < 64 || cp.has_job) return;
  if (!copier_hsa_setup(c)) return;
  auto tiny = [&](hsa_signal_t sig, void* dst, const void* src) {
    if (sdma_start(cp.engine, dst, cp.cpu_agent, src, cp.gpu_agent, 64, sig) && sdma_finish(c, sig, "", false, nullptr)) {
      cp.hsa_ready = false; cp.hsa_failed = true;
      cp.sig.forget(); cp.sig2.forget();
    }
  };
  tiny(cp.sig, c->h_keys.p, c->keys.p);
  if (cp.hsa_ready && c->dim && c->desc.p && c->h_desc.p && c->h_desc.bytes >= 64) tiny(cp.sig2, c->h_desc.p, c->desc.p);
}

// ---- the copier thread's steps (none touches cp.mu: copier_main holds the job between its unlock and lock) ----
// A batch whose pixels are still on their way (Copier::upload_first): wait for them on the host, then enqueue the batch.
static Step await_upload_and_enqueue(hess_ctx* c) {
  Copier& cp = c->cp;
  Step s;
  const auto t0 = std::chrono::steady_clock::now();
  // (a lost upload may still write the staging area: hess_ctx::poisoned)
  if (sdma_finish(c, cp.sig_in, "host->device upload of the pixels", true, s.msg)) {
    // the pixels never arrived (or arrived wrong): the kernels are NOT run on them
    snprintf(s.msg + strlen(s.msg), sizeof(s.msg) - strlen(s.msg), " (copier)");
    s.rc = HESS_ERR_DEVICE;
    cp.have_sig_in = false;  // (a signal that may still be written is left alone, not reused)
    cp.sig_in.forget();
  }
  PendingRun& r = *cp.run;
  r.t_load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (s.rc) return s;
  try {
    s.rc = enqueue(c, r);
  } catch (...) { s.rc = HESS_ERR_NOMEM; snprintf(s.msg, sizeof(s.msg), "out of host memory (copier)"); }
  if (!s.rc) {
    const hipError_t e = hipEventRecord(cp.ev_done, c->st);
    if (e != hipSuccess) return hip_failed("hipEventRecord", e);
  }
  if (s.rc && !s.msg[0]) snprintf(s.msg, sizeof(s.msg), "%s", c->err.c_str());
  return s;
}

// Room for `total` records in the pinned buffers (they hold the worst case unless that exceeds 512 MB: then they grow here, rarely).
static Step make_room(hess_ctx* c, size_t total, size_t db) {
  Step s;
  DevBuf &hk = c->h_keys, &hd = c->h_desc;
  if (hk.bytes >= total * sizeof(HostKeypoint) && (!c->dim || hd.bytes >= total * db)) return s;
  if (ensure(c, hk, total * sizeof(HostKeypoint)) || (c->dim && ensure(c, hd, total * db))) {
    snprintf(s.msg, sizeof(s.msg), "pinned result buffers: %s (copier)", c->err.empty() ? "allocation failed" : c->err.c_str());
    s.rc = HESS_ERR_NOMEM;
  }
  return s;
}

// A caller's keypoint lists: the results are in list order, and hess_wait needs the lists' map to input order beside
// them -- key_bin_kernel wrote it before any of the events.  Every image's rows at once: 4 bytes per record.
static Step deliver_list_order(hess_ctx* c, int batch) {
  const HostBlock b{c->h_kmap.p, c->kmap.p, (size_t)batch * c->cap_list * 4, "hipMemcpyAsync(list order)"};
  return bring_to_host(c, &b, 1, 0, "device->host copy of the keypoint lists' order", "", false);
}

// The results, part by part as the parts' events arrive; `s` is the status so far: a batch that has failed copies nothing
// more, but its events are still waited for.  The first wait of a part's copies is the injectable one.
static Step deliver_parts(hess_ctx* c, size_t total, bool overflow, size_t db, Step s) {
  Copier& cp = c->cp;
  const Parts& parts = c->parts;
  const int* hs = (const int*)c->h_small.p;
  const size_t kb = sizeof(HostKeypoint);
  char engine[32];
  snprintf(engine, sizeof(engine), ", engine 0x%x", cp.engine);
  size_t done_feats = 0;
  for (int k = 0; k < parts.n; k++) {
    hipError_t e;
    if (k > 0 && (e = hipEventSynchronize(k < parts.n - 1 ? cp.ev_part[k] : cp.ev_done)) != hipSuccess) s = hip_failed("hipEventSynchronize", e);
    // features of the images so far -- or, of one image's list, the bound the part's launch formed (k_feature.hip, desc_image)
    const size_t upto = overflow ? 0 : (k == parts.n - 1 ? total : parts.features ? (size_t)((long long)total * (k + 1) / parts.n)
                                                                                  : (size_t)hs[parts.end[k]]);
    const size_t first = done_feats, n = upto - done_feats;
    done_feats = upto;
    if (s.rc || !n) continue;
    const HostBlock b[2] = {{(char*)c->h_keys.p + first * kb, (const char*)c->keys.p + first * kb, n * kb, "hipMemcpyAsync(keys)"},
                            {(char*)c->h_desc.p + first * db, (const char*)c->desc.p + first * db, n * db, "hipMemcpyAsync(desc)"}};
    s = bring_to_host(c, b, c->dim ? 2 : 1, cp.engine, "device->host copy of the results", engine, true);
  }
  return s;
}

static void copier_main(hess_ctx* c) {
  Copier& cp = c->cp;
  (void)hipSetDevice(c->device);
  std::unique_lock<std::mutex> lk(cp.mu);
  for (;;) {
    cp.cv.wait(lk, [&] { return cp.stop || cp.has_job; });
    if (cp.stop) return;
    const int batch = cp.run->batch;
    const size_t db = run_desc_bytes(c, cp.run->desc_format);  // (plan() ran before the job was posted)
    lk.unlock();
    bool overflow = false;
    Step s;
    if (cp.upload_first) s = await_upload_and_enqueue(c);
    // Several parts when the batch's descriptors were launched in groups of images (nparts > 1): a group's results
    // cross while the next group is computed; else one part behind the last kernel.  The counts (and the overflow
    // words) are in the pinned count block since feature_scan_kernel, i.e. before any of the events.
    // (hess_ctx::parts says why no lock is needed; after a failed upload or a half-run enqueue rc is set: no parts to wait for)
    if (!s.rc) {
      const hipError_t e = hipEventSynchronize(c->parts.n > 1 ? cp.ev_part[0] : cp.ev_done);
      if (e != hipSuccess) s = hip_failed("hipEventSynchronize", e);
    }
    if (!s.rc) {
      const int* hs = (const int*)c->h_small.p;
      overflow = hs[batch + 1] != 0 || hs[batch + 2] != 0 || hs[batch + 3] != 0;  // (word 3: a device-side error, nothing to copy)
      const size_t total = overflow ? 0 : (size_t)hs[batch];
      if (total) s = make_room(c, total, db);
      if (!s.rc && total && user_mode(c)) s = deliver_list_order(c, batch);
      s = deliver_parts(c, total, overflow, db, s);
    }
    lk.lock();
    cp.rc = s.rc;
    cp.overflow = overflow;
    snprintf(cp.err, sizeof(cp.err), "%s", s.msg);
    cp.has_job = false;
    cp.done = true;
    cp.cv.notify_all();
  }
}

int copier_start(hess_ctx* c) {
  Copier& cp = c->cp;
  if (cp.th.joinable()) return 0;
  HIP_TRY(c, hipStreamCreateWithFlags(&cp.cs.h, hipStreamNonBlocking));
  HIP_TRY(c, hipEventCreateWithFlags(&cp.ev_done.h, hipEventDisableTiming));
  for (Event& ev : cp.ev_part) HIP_TRY(c, hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
  try {
    cp.th = std::thread(copier_main, c);
  } catch (...) {
    set_err(c, "cannot start the copier thread");
    return HESS_ERR_NOMEM;
  }
  return 0;
}

void copier_stop(hess_ctx* c) {
  Copier& cp = c->cp;
  if (!cp.th.joinable()) return;
  {
    std::unique_lock<std::mutex> lk(cp.mu);
    cp.cv.wait(lk, [&] { return cp.done; });
    cp.stop = true;
    cp.cv.notify_all();
  }
  cp.th.join();
}

// How the results of a batch of `batch` images reach the host (see the kDeliver* comment): small batches through the
// descriptor kernel's own stores (lowest latency), larger ones by the copier thread's DMA copy (no kernel waits for
// PCIe).  HESS_DELIVERY overrides.
void choose_delivery(hess_ctx* c, int batch) {
  // Small batches keep the in-kernel mirror (latency: no event wake-up, no copy behind the last kernel) -- unless their
  // results are large: a kernel that stores tens of megabytes into host memory waits for the link (one 4096^2 image with
  // 102 k half descriptors, 28 MB: 0.76 ms against 0.47), while the copier's DMA copy of a part runs beside the next
  // part's launch -- 15 % more images per second on three pipelined contexts.  That needs a caller who overlaps: a batch
  // handed over by hess_submit_* (hess_run_*, i.e. submit + wait in one call, keeps the mirror: nothing to overlap with,
  // and through the class with pageable pixels the copier's route is 15 % slower for a 4096^2 image).  "Large" is judged by
  // what the context's last batch of this size delivered (the capacity is a worst case many times the typical count): the
  // first batch of a context uses the mirror.  HESS_MIRROR_MAX_MB (16) is the limit.
  const size_t expect = (c->last_result_batch == batch && !c->caller_waits) ? c->last_result_bytes : 0;
  const bool small = batch <= c->sw.mirror_max_batch && !(batch >= 2 && !c->caller_waits);  // (a submitted pair: see enqueue())
  int d = c->sw.delivery_pref >= 0 ? c->sw.delivery_pref : (small && expect <= c->sw.mirror_max_bytes ? kDeliverMirror : kDeliverDma);
  if (d == kDeliverMirror && !c->host_fits) d = kDeliverDma;  // the mirror needs the worst case pinned up front
  if (d == kDeliverDma && copier_start(c) != 0) d = kDeliverBlit;
  c->delivery = d;
  c->host_direct = d == kDeliverMirror;
}

// The one hand-off to the copier thread: `run` (which outlives the job: hess_ctx::run, or a local of a caller that waits
// before it returns) and whether the thread is to wait for the pixels' upload and enqueue the batch itself.
static void copier_post(hess_ctx* c, PendingRun* run, bool upload_first) {
  Copier& cp = c->cp;
  std::lock_guard<std::mutex> lk(cp.mu);
  cp.run = run;
  cp.upload_first = upload_first;
  cp.done = false;
  cp.has_job = true;
  cp.cv.notify_all();
}

// ---- input routes (hess_submit_host: the pixels into the staging area c->stage, c->run describes them) ----
// Pinned pixels of a batch that the copier thread will deliver: the upload goes to an SDMA engine directly and
// the copier thread enqueues the kernels once it has landed (Copier::upload_first).  A copy command on the
// context's stream would hold its hardware queue -- shared with other contexts -- for the length of the
// transfer: 15.9 - 16.2 against 17.0 Gpix/s for six pipelined contexts, while the same bytes uploaded on the side
// cost nothing (tools/r03/r03_h2d_bg.py).  *taken: the batch is submitted; else nothing is in flight, take the stream.
int upload_beside_queues(hess_ctx* c, const void* pixels, size_t bytes, bool* taken) {
  *taken = false;
  if (c->sw.no_host_upload) return 0;
  if (int rc = plan(c, c->run.width, c->run.height, c->run.batch)) return rc;
  choose_delivery(c, c->run.batch);
  Copier& cp = c->cp;
  hsa_amd_pointer_info_t pi;
  memset(&pi, 0, sizeof(pi));
  pi.size = sizeof(pi);
  if (c->delivery != kDeliverDma || !copier_hsa_setup(c) ||
      hsa_amd_pointer_info(const_cast<void*>(pixels), &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS ||
      pi.type == HSA_EXT_POINTER_TYPE_UNKNOWN ||
      !(cp.have_sig_in || hsa_signal_create(1, 0, nullptr, &cp.sig_in.h) == HSA_STATUS_SUCCESS))
    return 0;
  cp.have_sig_in = true;
  if (!sdma_start(cp.engine_in, c->stage.p, cp.gpu_agent, pixels, pi.agentOwner, bytes, cp.sig_in)) return 0;
  c->last_input_bytes = bytes;
  copier_post(c, &c->run, true);
  c->run.active = true;
  *taken = true;
  return 0;
}

// Pageable memory: copied into the pinned staging buffer in chunks, each chunk's transfer enqueued as soon as
// it is staged, so the copy engine works while the next chunks are being copied (one core copies at about
// 17 GB/s, a third of what the link takes: the context's helper threads share the work, see Stager).
// 4 MB chunks; a small input (one image) is cut in four so that its transfer, too, overlaps its staging, and is
// staged by the calling thread alone: waking the helpers costs more than they save below about 8 MB (one 1080p
// image: 0.544 ms per call alone, 0.58 ms with helpers; profiles/r03_host_path.json).
// Nothing here allocates or throws once the helpers exist (nothing thrown crosses the C ABI).
static int upload_staged(hess_ctx* c, const void* pixels, size_t bytes) {
  if (int rc = ensure(c, c->h_stage, bytes)) return rc;
  const size_t chunk = std::min<size_t>((size_t)4 << 20, std::max<size_t>((size_t)256 << 10, ((bytes / 4 + 65535) >> 16) << 16));
  hipError_t cerr = hipSuccess;  // the first one
  const bool ran = stager_run(c->sg, pixels, c->h_stage.p, bytes, chunk, bytes >= policy::kStagerHelpFrom, [&](size_t off, size_t len) {
    if (cerr == hipSuccess)
      cerr = hipMemcpyAsync((char*)c->stage.p + off, (const char*)c->h_stage.p + off, len, hipMemcpyHostToDevice, c->st);
  });
  if (!ran) { set_err(c, "out of memory"); return HESS_ERR_NOMEM; }
  HIP_TRY(c, cerr);
  return 0;
}

// One asynchronous host->device transfer on the context's stream, between the two load events: pinned pixels are read by
// the copy engine directly, pageable ones go through the pinned staging buffer.
int upload_on_stream(hess_ctx* c, const void* pixels, size_t bytes, bool pinned) {
  HIP_TRY(c, hipEventRecord(c->ev_load[0], c->st));
  if (pinned) {
    HIP_TRY(c, hipMemcpyAsync(c->stage.p, pixels, bytes, hipMemcpyHostToDevice, c->st));
  } else {
    (void)hipGetLastError();  // an unregistered pointer is reported as an error: not one
    if (int rc = upload_staged(c, pixels, bytes)) return rc;
  }
  HIP_TRY(c, hipEventRecord(c->ev_load[1], c->st));
  c->last_input_bytes = bytes;
  c->run.timed_load = true;
  return 0;
}

// Pending keypoint lists are one per image of the batch that uses them.
int check_user_batch(hess_ctx* c, int batch) {
  if (!user_mode(c) || batch == (int)c->user_counts.size()) return 0;
  if (c->user_counts.size() == 1) set_err(c, "a keypoint list applies to a single image");
  else set_err(c, "keypoint lists were set for %d images, the batch has %d", (int)c->user_counts.size(), batch);
  return HESS_ERR_ARG;
}

// Enqueue the whole path (the per-image counts reach the pinned count block by feature_scan_kernel's own stores);
// returns without waiting.
int submit_inner(hess_ctx* c, PendingRun& r) {
  int rc = check_user_batch(c, r.batch);
  if (rc) return rc;
  rc = plan(c, r.width, r.height, r.batch);
  if (rc) return rc;
  choose_delivery(c, r.batch);
  HIP_TRY(c, hipGetLastError());
  rc = enqueue(c, r);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  if (c->delivery == kDeliverDma) {
    HIP_TRY(c, hipEventRecord(c->cp.ev_done, c->st));
    copier_post(c, &r, false);
  }
  return 0;
}

// (nothing thrown crosses the C ABI: plan() and the profiling scopes grow host vectors)
int submit_impl(hess_ctx* c, PendingRun& r) {
  try {
    return submit_inner(c, r);
  } catch (...) {
    set_err(c, "out of host memory while preparing the batch");
    return HESS_ERR_NOMEM;
  }
}

// Wait for the submitted batch, grow storage and re-run if a list overflowed; with kDeliverBlit bring the
// keypoints and descriptors of the whole batch to the host with one transfer each (the other modes have
// delivered them by now).
int wait_inner(hess_ctx* c, PendingRun& r) {
  int rc;
  int* hs = (int*)c->h_small.p;
  const int batch = r.batch;
  for (int attempt = 0;; attempt++) {
    if (c->delivery == kDeliverDma) {
      Copier& cp = c->cp;
      std::unique_lock<std::mutex> lk(cp.mu);
      cp.cv.wait(lk, [&] { return cp.done; });
      if (cp.rc) { set_err(c, "%s", cp.err); return cp.rc; }
    } else {
      HIP_TRY(c, hipStreamSynchronize(c->st));
    }
    const int of_raw = hs[batch + 1], of_feat = hs[batch + 2];
    if (hs[batch + 3]) {  // a kernel gave up a bounded wait (extrema_place_kernel: the image's flag; topk_select_kernel: its look-back): no results
      set_err(c, "device-side wait did not complete (extrema placement's flag wait or top-K look-back); the batch has no results");
      return HESS_ERR_DEVICE;
    }
    if (!of_raw && !of_feat) break;
    if (user_mode(c)) {  // (storage for a caller's lists follows from their lengths: growing it would not help)
      set_err(c, "keypoint lists (%d) exceed the reserved feature storage", of_raw > of_feat ? of_raw : of_feat);
      return HESS_ERR_NOMEM;
    }
    if (attempt >= 8) { set_err(c, "feature storage keeps overflowing"); return HESS_ERR_NOMEM; }
    // grow-only reallocation, then run the batch again (reference: SetLevelFeatureNum grows on demand,
    // PyramidCU.cpp:393-397)
    if (of_raw) c->cap_raw = of_raw + of_raw / 4;
    if (of_feat) c->cap_feat = of_feat + of_feat / 4;
    c->planned = false;
    c->regrown++;
    if (c->p.verbose & 1) fprintf(stderr, "hessgpu: feature storage grown (raw %d, features %d)\n", c->cap_raw, c->cap_feat);
    if ((rc = submit_impl(c, r))) return rc;
  }
  drain_profile(c);
  c->counts.resize(batch);
  c->offs.assign(batch + 1, 0);
  for (int b = 0; b < batch; b++) {
    c->counts[b] = hs[b + 1] - hs[b];
    c->offs[b + 1] = (size_t)hs[b + 1];
  }
  const size_t total = c->offs[batch];
  c->seen_features = batch ? *std::max_element(c->counts.begin(), c->counts.end()) : 0;
  const size_t db = run_desc_bytes(c, r.desc_format);
  c->last_result_bytes = total * (sizeof(HostKeypoint) + db);
  c->last_result_batch = batch;
  if ((rc = ensure(c, c->h_keys, (total ? total : 1) * sizeof(HostKeypoint)))) return rc;
  if (c->dim && (rc = ensure(c, c->h_desc, (total ? total : 1) * db))) return rc;
  if (total && c->delivery == kDeliverBlit) {
    HIP_TRY(c, hipMemcpyAsync(c->h_keys.p, c->keys.p, total * sizeof(HostKeypoint), hipMemcpyDeviceToHost, c->st));
    if (c->dim)
      HIP_TRY(c, hipMemcpyAsync(c->h_desc.p, c->desc.p, total * db, hipMemcpyDeviceToHost, c->st));
    if (user_mode(c))  // the lists' map to input order travels with the results
      HIP_TRY(c, hipMemcpyAsync(c->h_kmap.p, c->kmap.p, (size_t)batch * c->cap_list * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(c, hipStreamSynchronize(c->st));
  }
  c->user_result = false;
  if (user_mode(c)) {
    // Every image's results back to input order (PyramidCU.cpp:537-549,1157-1168): zeros for a key that is listed nowhere,
    // the later listing for a key listed twice, and of a list longer than the image's keys only the first `num` entries,
    // as the reference has it.  The caller's keypoints are returned unchanged unless DownloadKeypoints would run (-m 1 /
    // -ofix, SiftPyramid.cpp:160-171).  The device records stay in list order (hess_device_results, hess_key_list_order).
    const bool download = !c->user_have_orientation && ((c->p.max_orientation < 2) || c->p.fixed_orientation);
    const hess_keypoint* const given = (const hess_keypoint*)c->h_user.p;
    const int* const kmap = (const int*)c->h_kmap.p;
    c->u_keys.assign(given, given + c->user_total);
    c->u_desc.assign((size_t)c->user_total * (db ? db : 1), 0);
    c->u_order.assign(total, 0);
    c->u_first.assign(batch + 1, 0);
    for (int b = 0; b < batch; b++) {
      const int num = c->user_counts[b], len = c->counts[b];
      const size_t first = c->u_first[b], lfirst = c->offs[b];
      const int listed = std::min(len, num);
      for (int i = 0; i < len; i++) {
        const int k = kmap[(size_t)b * c->cap_list + i];
        if (k < 0 || k >= num) { set_err(c, "keypoint list of image %d: entry %d names key %d of %d", b, i, k, num); return HESS_ERR_DEVICE; }
        c->u_order[lfirst + i] = k;
        if (i >= listed) continue;
        if (download) memcpy(&c->u_keys[first + k], (HostKeypoint*)c->h_keys.p + lfirst + i, sizeof(hess_keypoint));
        if (c->dim) memcpy(&c->u_desc[(first + k) * db], (const char*)c->h_desc.p + (lfirst + i) * db, db);
      }
      c->u_first[b + 1] = first + (size_t)num;
      c->counts[b] = num;
    }
    c->user_result = true;
    clear_user_list(c);      // _existing_keypoints = 0 after RunSIFT (SiftPyramid.cpp:182-184)
    c->user_levels.clear();  // the parity hook covers one keypoint-list run
  }
  // stage times from the events of the last enqueue (config.h:17-31 order)
  memset(c->timing, 0, sizeof(c->timing));
  auto el = [&](int i, int j) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev[i], c->ev[j]); return ms; };
  c->timing[HESS_T_LOAD] = (float)r.t_load_ms;
  if (r.timed_load) { float ms = 0; (void)hipEventElapsedTime(&ms, c->ev_load[0], c->ev_load[1]); c->timing[HESS_T_LOAD] = ms; }
  if (c->stage_events) {
    c->timing[HESS_T_PYRAMID] = el(0, 1);
    c->timing[HESS_T_DETECT] = el(1, 2);
    c->timing[HESS_T_LIST] = el(2, 3);
    c->timing[HESS_T_REDUCTION] = el(3, 4);
    c->timing[HESS_T_ORIENT] = el(4, 5);
    c->timing[HESS_T_MULTI_ORIENT] = el(5, 6);
    c->timing[HESS_T_DESCRIPTOR] = el(6, 7);
  }
  c->timing[HESS_T_TOTAL] = el(0, 7) + c->timing[HESS_T_LOAD];
  c->batch = c->pyramid_batch = batch;  // only now: every error return above leaves the context without results
  return 0;
}

int wait_impl(hess_ctx* c, PendingRun& r) {
  try {
    return wait_inner(c, r);
  } catch (...) {  // the host-side count / keypoint-list vectors
    clear_user_list(c);
    set_err(c, "out of host memory while collecting the results");
    return HESS_ERR_NOMEM;
  }
}

}  // namespace hess
