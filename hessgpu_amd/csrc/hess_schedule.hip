// hess_schedule.hip -- the launch order of one batch on the context's stream (see hess_ctx.h).
#include "hess_ctx.h"

namespace hess {

// ---- profiling helpers ----
hipEvent_t get_event(hess_ctx* c) {
  if (!c->prof_ev.pool.empty()) { hipEvent_t e = c->prof_ev.pool.back(); c->prof_ev.pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) { set_err(c, "hipEventCreate failed: profiling disabled"); c->prof = false; return nullptr; }
  return e;
}
// A RUN of consecutive launches of one kernel family between ONE pair of events: an event record between two kernels leaves
// the stream idle for a few microseconds, which per-launch pairs book on 22 pyramid launches a step (the hipEvent figure of
// the Gaussian stage read 0.53 ms where the kernel trace sums 0.47).  The launches of octave 0 keep a pair each (their
// share of the stage is reported apart); the small octaves' launches, which follow them back to back, share one.
// The first add() takes two events and records `a`, close() (or the end of the scope) records `b` and queues the pair for
// drain_profile(); without profiling, or when an event cannot be had, nothing is recorded.
struct ProfRun {
  hess_ctx* c;
  EventPair ep{};
  bool open = false;
  ProfRun(hess_ctx* ctx, int kernel, int kernel2 = -1) : c(ctx) { ep.kernel = kernel; ep.kernel2 = kernel2; }
  ProfRun(const ProfRun&) = delete;
  void add(double bytes, double in_lds = 0.0) {
    if (!c->prof) return;
    if (!open) {
      ep.a = get_event(c); ep.b = get_event(c); ep.bytes = 0.0; ep.in_lds = 0.0; ep.count = 0;
      if (!ep.a || !ep.b || hipEventRecord(ep.a, c->st) != hipSuccess) {
        if (ep.a) c->prof_ev.pool.push_back(ep.a);
        if (ep.b) c->prof_ev.pool.push_back(ep.b);
        return;
      }
      open = true;
    }
    ep.bytes += bytes; ep.in_lds += in_lds; ep.count++;
  }
  void close() {
    if (!open) return;
    open = false;
    if (hipEventRecord(ep.b, c->st) != hipSuccess) { c->prof_ev.pool.push_back(ep.a); c->prof_ev.pool.push_back(ep.b); return; }
    c->prof_ev.pending.push_back(ep);
  }
  ~ProfRun() { close(); }
};
// What follows in the scope between a pair of events of its own (wanted = false: no pair, see book_pyramid).
struct ProfScope : ProfRun {
  ProfScope(hess_ctx* ctx, int kernel, double bytes, int kernel2 = -1, double in_lds = 0.0, bool wanted = true)
      : ProfRun(ctx, kernel, kernel2) {
    if (wanted) add(bytes, in_lds);
  }
};
// How every pyramid launch is booked.  One that belongs to octave 0 (the pair whose first job is octave 0's top level
// included) ends the running run and gets the returned pair of its own, on HESS_K_GAUSS and HESS_K_GAUSS_OCT0; any other
// launch joins the run.
static ProfScope book_pyramid(ProfRun& run, bool octave0, double bytes, double in_lds = 0.0) {
  if (octave0) run.close();
  else run.add(bytes, in_lds);
  return ProfScope(run.c, HESS_K_GAUSS, bytes, HESS_K_GAUSS_OCT0, in_lds, octave0);
}
void drain_profile(hess_ctx* c) {
  for (auto& ep : c->prof_ev.pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
      c->k_ms[ep.kernel] += ms;
      c->k_n[ep.kernel] += ep.count;
      c->k_bytes[ep.kernel] += ep.bytes;
      c->k_in_lds[ep.kernel] += ep.in_lds;
      if (ep.kernel2 >= 0) {
        c->k_ms[ep.kernel2] += ms; c->k_n[ep.kernel2] += ep.count; c->k_bytes[ep.kernel2] += ep.bytes; c->k_in_lds[ep.kernel2] += ep.in_lds;
      }
    }
    c->prof_ev.pool.push_back(ep.a);
    c->prof_ev.pool.push_back(ep.b);
  }
  c->prof_ev.pending.clear();
}

// 2^_octave_min: scale of the first octave relative to the input (PyramidCU.cpp:566-569,746-748,1054-1057).
static inline float first_octave_sigma(const hess_ctx* c) {
  return c->ds > 0 ? (float)(1 << c->ds) : (c->ds < 0 ? 1.0f / (float)(1 << (-c->ds)) : 1.0f);
}

int enqueue_user(hess_ctx* c, int batch, int desc_format);

// Orientation stage (GetFeatureOrientations).  existing: a caller's keypoints -- position and scale as packed, one angle written.
static OrientParams orient_params(const hess_ctx* c, bool existing) {
  const hess_params& p = c->p;
  OrientParams op;
  op.gaussian_factor = p.orient_gaussian_factor;
  op.sample_factor = p.orient_gaussian_factor * p.orient_window_factor;  // ProgramCU.cu:1638
  op.ln_sigma_step = c->sch.ln_sigma_step;
  op.num_orientation = p.fixed_orientation ? 0 : p.max_orientation;      // ProgramCU.cu:1639
  op.subpixel = existing ? 0 : p.subpixel;
  op.half_sift = p.half_sift;
  op.existing = existing ? 1 : 0;
  op.two_peaks = !existing && c->sch.detector == HESS_DETECTOR_DOG && op.num_orientation > 1;
  for (int l = 0; l < kMaxLev; l++) op.level_sigma[l] = l <= c->sch.level_max ? c->sch.level_sigma[l] : 0.0f;
  return op;
}

// Descriptor stage (GetFeatureDescriptors).  user: a caller's keypoints -- one float angle each, never the fixed-point pixel order.
static DescParams desc_params(const hess_ctx* c, int pixtype, int desc_format, bool user) {
  const hess_params& p = c->p;
  DescParams dsp;
  dsp.window_factor = p.desc_window_factor;
  dsp.half_sift = p.half_sift;
  dsp.normalize = p.normalize;
  dsp.multi = (user || !c->multi) ? 0 : (c->sch.detector == HESS_DETECTOR_DOG ? 2 : 1);
  dsp.lowe_origin = p.lowe_origin;
  dsp.octave_sigma = first_octave_sigma(c);  // PyramidCU.cpp:746-748
  dsp.dog = c->g.dog;
  dsp.dynamic_indexing = p.dynamic_indexing ? 1 : 0;
  dsp.hkeys = c->host_direct ? (HostKeypoint*)c->h_keys.p : nullptr;
  dsp.hdesc = (c->host_direct && c->dim) ? c->h_desc.p : nullptr;
  dsp.u8 = desc_format == HESS_DESC_FORMAT_U8;
  dsp.first_image = 0; dsp.part = 0; dsp.part_den = 1;  // (one launch over the whole list)
  dsp.xcd_block = c->sw.desc_xcd_block; dsp.px_band = c->sw.desc_px_band;
  dsp.sequential = p.descriptor_order == HESS_DESC_ORDER_SEQUENTIAL;
  // the pixel order's fixed point assumes luminance in [0, 1] (8- and 16-bit inputs); float pixels are taken as they are
  // and keep the interleaved order (the test oracle applies the same rule)
  dsp.pixel = !user && p.descriptor_order == HESS_DESC_ORDER_PIXEL && pixtype != HESS_PIX_F32;
  dsp.rect = (user && c->user_rect) ? 1 : 0;  // HESS_KEYS_RECTANGLES: descriptor_rect_kernel, whatever the order
  return dsp;
}

// Delivered by the copier thread, a batch of four or more images gets its descriptors in two launches (the images
// are independent and packed back to back): the first half's results cross the host link while the second half is
// computed -- half of the transfer (0.53 ms for eight 1080p images) leaves the batch's critical path.  Four groups
// shorten a lone batch a little more (1.75 / 1.58 / 1.53 ms for 1 / 2 / 4) but cost the pipelined rate 1 %:
// HESS_DESC_PARTS=n overrides (1: one launch, up to kMaxParts).
// ONE image delivered by the copier thread (a large one: choose_delivery) gets its descriptors in four launches over
// quarters of its feature list, for the same reason (a 4096^2 image with 102 k half descriptors: 28 MB, 0.58 ms on the
// link; 2.09 -> 1.7 ms per image on one context).
static void choose_parts(hess_ctx* c, int batch) {
  Parts& pt = c->parts;
  int want = batch >= policy::kSplitDescriptorsFrom ? 2 : 1;
  pt.features = false;
  static_assert(policy::kLargeImageParts <= Copier::kMaxParts, "parts of one image");
  if (batch == 1 && c->delivery == kDeliverDma) { want = policy::kLargeImageParts; pt.features = true; }
  if (c->sw.desc_parts > 0) want = std::max(1, std::min<int>(Copier::kMaxParts, pt.features ? c->sw.desc_parts : std::min(batch, c->sw.desc_parts)));
  if (c->delivery != kDeliverDma || !c->cp.ev_part[0]) want = 1;
  if (want == 1) pt.features = false;
  pt.n = want;
  for (int k = 0; k < want; k++) pt.end[k] = pt.features ? 1 : (int)((long long)batch * (k + 1) / want);
}

// ---- input + pyramid (BuildPyramid, PyramidCU.cpp:1486-1558), det-H + gradient (DetectKeypointsEX part 1, :1576-1591) ----
// From the run's `batch` images, whose pixels are at device address r.dev, to the det-H (or DoG) and gradient planes.
static int enqueue_pyramid(hess_ctx* c, const PendingRun& r) {
  const void* const dev = r.dev;
  const int pitch = r.pitch, batch = r.batch, format = r.format, pixtype = r.pixtype;
  const size_t image_stride = r.image_stride;
  const Schedule& s = c->sch;
  const Geom& g = c->g;
  hipStream_t st = c->st;
  float* gauss = (float*)c->gauss.p;
  float* deth = (float*)c->deth.p;
  float* got = (float*)c->got.p;
  auto plane_ptr = [&](float* base, int o, int l) { return base + g.o[o].lvl_off + (long long)l * g.B * g.o[o].plane; };
  const bool user_mode = hess::user_mode(c);
  const bool direct_u8 = (format == HESS_FMT_LUM && pixtype == HESS_PIX_U8 && c->ds == 0 && c->has_taps0 &&
                          (pitch % 4) == 0 && (image_stride % 4) == 0 && ((uintptr_t)dev % 4) == 0);
  const float* src_f = nullptr;
  if (!direct_u8) {
    ProfScope ps(c, HESS_K_INPUT, (double)batch * c->img_w * c->img_h * (4.0 + fmt_channels(format)));
    const int up = c->ds < 0 ? -c->ds : 0;  // up-sampled first octave: convert at full size, then SampleImageU
    launch_convert(st, dev, format, pixtype, pitch, (long long)image_stride, up ? 0 : c->ds, (float*)c->input_f32.p,
                   c->img_w >> up, c->img_h >> up, batch);
    src_f = (const float*)c->input_f32.p;
    if (up) {  // PyramidCU.cpp:1521-1522
      launch_upsample(st, src_f, c->img_w >> up, c->img_h >> up, up, (float*)c->upsampled.p, batch);
      src_f = (const float*)c->upsampled.p;
    }
  }
  // The launch that produces the down-sampling level (level_ds = dog, one of levels 1 .. level_max - 1 in both detector
  // modes: resolve()) also writes level 0 of the next octave (its even rows and columns): no decimation launches.
  // det-H of the top level by the launch that produces it (k_gauss.hip, TOP tiles); HESS_NO_TOP_FUSION=1: the round-4
  // form (the level is stored, hessian_rows4_kernel reads it back) for A/B runs
  const bool top_fused = s.level_max == g.dog + 1 && !c->sw.no_top_fusion;
  c->zero_filled = false;
  // Level l of octave o from level l-1; the same launch emits det-H (+ gradient/theta) of level l-1 from the source
  // window it stages: 8 B R+W for the blur, 4 B (+8 B) W for the fused planes (+ 4 B per pixel of the next octave's
  // level 0 when it is the down-sampling level).
  // (a fused top level reads its source and writes its own det-H instead of the level: the same 8 bytes)
  // in_lds: SURVEY 8d books every array of the reference's layout written once and read once; a level this build keeps in
  // LDS -- the octave's top level, level 0 of octave 0 -- is 8 bytes per pixel of that layout which no launch here moves.
  struct Level { GaussJob job; double bytes, in_lds; };
  auto level = [&](int o, int l) {
    const OctGeom& og = g.o[o];
    const bool src_got = (l - 1 >= 1 && l - 1 <= g.dog);
    const bool decim = l == s.level_ds && o + 1 < g.noct;
    const bool top = top_fused && l == s.level_max;
    Level lv;
    GaussJob& j = lv.job;
    j.src = plane_ptr(gauss, o, l - 1); j.dst = plane_ptr(gauss, o, l); j.wa = og.wa; j.h = og.h; j.taps = s.taps[l];
    j.deth_src = plane_ptr(deth, o, l - 1);
    j.got_src = src_got ? got + 2 * (og.got_off + (long long)(l - 2) * g.B * og.plane) : nullptr;
    j.norm_src = s.norm[l - 1];
    j.decim_dst = decim ? plane_ptr(gauss, o + 1, 0) : nullptr;
    j.decim_w = decim ? g.o[o + 1].wa : 0; j.decim_h = decim ? g.o[o + 1].h : 0;
    if (top) {
      // The octave's top level is nobody's source: its det-H comes out of the launch that produces it (from the output
      // tile in LDS) and the level itself is not written to HBM -- unless the parity tests ask (hess_debug_keep_levels).
      j.deth_dst = plane_ptr(deth, o, l);
      j.norm_dst = s.norm[l];
      if (!c->keep_levels) j.dst = nullptr;
      if (o == 0 && !user_mode) {  // octave 0's launch also clears what the detection stages expect zeroed
        j.zero = c->zeroed.p;
        j.zero_bytes = c->zeroed_used;
      }
    }
    lv.bytes = (double)batch * og.plane * (8.0 + 4.0 + (src_got ? 8.0 : 0.0)) + (decim ? (double)batch * g.o[o + 1].plane * 4.0 : 0.0);
    lv.in_lds = (top && !c->keep_levels) ? (double)batch * og.plane * 8.0 : 0.0;
    return lv;
  };
  auto launch_level = [&](const GaussJob& j) {
    if (j.zero) c->zero_filled = true;
    launch_gauss_job(st, j, batch);
  };
  // T(o, l) = 3o + l is the earliest step of level l of octave o (level 0 of octave o+1 is the decimated level_ds of
  // octave o): the top level of an octave and level 1 of the next are due together and independent, so they share a
  // launch (launch_gauss_pair) -- one launch fewer per octave in the dependent chain.
  const bool pair_levels = !c->sw.no_pair;
  // A single image (or two): octaves from 1 on get levels 1..level_ds -- what the next octave waits for -- from ONE
  // launch each (gauss_chain_kernel: 32x32 tiles computed in LDS on a shrinking halo): below 960x540 a level launch is a
  // few dozen workgroups that mostly wait, and the eighteen of them for octaves 1-6 of a 1080p image were two thirds of
  // its pyramid's time.  The top levels (nobody's input) follow in one launch for all octaves, together with det-H /
  // gradient of the chained octaves' levels 0..level_ds-1.  Same box, one 1080p image, device-resident: 0.400 -> 0.334 ms.
  // NOT for larger batches: a batch of 8 is 2 % faster on one stream with octaves >= 2 chained, but six pipelined
  // contexts lose 2 - 4 % (15.5 - 15.6 against 16.1 - 16.2 Gpix/s, same call; 15.8 - 16.0 with octaves >= 3) -- the chain
  // trades dependent launches for redundant arithmetic in 1024-thread workgroups that wait at barriers, which is what
  // an idle device wants and a saturated one does not; and not for the large octaves of a large image (a 4096^2 image's
  // octave 1 is 4 096 such workgroups: configs[4] 2.19 against 2.12 ms).  Needs the default schedule's tap counts.
  // HESS_CHAIN_FROM=n forces the first chained octave (99: never).
  int chain_from = g.noct;
  if (s.level_max == s.level_ds + 1 && gauss_chain_available(s.taps, s.level_ds)) {
    chain_from = c->sw.chain_from;
    if (chain_from <= 0) {  // by size: the first octave (>= 1) whose planes of the whole batch are at most two 960x540 planes
      chain_from = g.noct;
      // (a PAIR of images handed over by hess_submit_* -- a caller who pipelines -- gets the level-by-level launches and
      //  the copier's delivery like a larger batch: 17.0 - 17.3 against 12.3 - 12.6 Gpix/s for six pipelined contexts)
      if (batch == 1 || (batch <= policy::kLatencyBatch && c->caller_waits))
        for (int o = g.noct - 1; o >= 1 && (long long)batch * g.o[o].plane <= policy::kChainMaxPixels; o--) chain_from = o;
    }
    if (chain_from > g.noct) chain_from = g.noct;
  }
  const bool chained = chain_from < g.noct;
  // Where the top level of octave o goes: with a chain, the tops of the octave before it and of every chained one are
  // collected for one launch after the loop; otherwise it rides with level 1 of the next octave (pair_levels) or, without
  // one, gets a launch of its own.
  enum TopRoute { kTopCollected, kTopRides, kTopOwnLaunch };
  auto top_route = [&](int o) {
    return chained && o + 1 >= chain_from ? kTopCollected : (pair_levels && o + 1 < g.noct ? kTopRides : kTopOwnLaunch);
  };
  ProfRun small_octaves(c, HESS_K_GAUSS);  // one event pair for the consecutive launches of octaves >= 1 (see ProfRun)
  GaussJob top_jobs[kMaxOct];  // the collected top levels
  int ntop = 0;
  double top_bytes = 0.0, top_in_lds = 0.0;
  for (int o = 0; o < g.noct; o++) {
    const OctGeom& og = g.o[o];
    int l = 1;  // the first level that still needs a launch
    if (o >= chain_from) {  // (>= 1: its level 0 is the decimated level_ds of octave o-1, written by that launch)
      ChainJob cj;
      double bytes = 0.0;
      cj.src0 = plane_ptr(gauss, o, 0);
      for (int k = 0; k <= s.level_ds; k++) {
        cj.dst[k] = plane_ptr(gauss, o, k);
        cj.taps[k] = s.taps[k];
        // (the bytes of the fused planes are booked here although hessian_low_levels writes them: per step the sums agree)
        if (k >= 1) bytes += level(o, k).bytes;
      }
      cj.nlevels = s.level_ds; cj.wa = og.wa; cj.h = og.h;
      const bool decim = o + 1 < g.noct;
      cj.decim_dst = decim ? plane_ptr(gauss, o + 1, 0) : nullptr;
      cj.decim_w = decim ? g.o[o + 1].wa : 0; cj.decim_h = decim ? g.o[o + 1].h : 0;
      ProfScope ps = book_pyramid(small_octaves, false, bytes);
      if (!launch_gauss_chain(st, cj, batch)) { set_err(c, "level-chain launch refused"); return HESS_ERR_DEVICE; }
      l = s.level_max;
    } else if (o == 0) {
      bool first_fused = false;  // levels 0 and 1 come out of one launch (level 0 never written)
      if (direct_u8 && !c->sw.no_first_fusion && s.level_ds != 1 && gauss_first_available(c->taps0, s.taps[1])) {
        // Decided BEFORE the profile scope: a refused launch must not book bytes.  The tap counts are the one refusal of
        // launch_gauss_first that can still fire here: its alignment clauses (pitch % 4, img_stride % 4) repeat what
        // direct_u8 already requires, and level(0, 1) has the plane pointers it asks for.  An unaligned pitch, image
        // stride or base never gets this far: it goes through convert_kernel (tests/test_input_layouts_gpu.py).
        // u8 pixels -> level 0 (LDS) -> level 1, det-H of level 0: the level-0 plane is nobody's input but level 1's
        // (and, with the DoG detector, D_1's: the level is stored then)
        const bool store0 = c->keep_levels || s.detector == HESS_DETECTOR_DOG;
        ProfScope ps = book_pyramid(small_octaves, true,
                                    (double)batch * og.plane * (1.0 + 4.0 + 4.0 + (s.detector == HESS_DETECTOR_DOG ? 4.0 : 0.0)),
                                    store0 ? 0.0 : (double)batch * og.plane * 8.0);
        first_fused = launch_gauss_first(st, (const uint8_t*)dev, pitch, (long long)image_stride, c->taps0, level(0, 1).job,
                                         store0 ? plane_ptr(gauss, 0, 0) : nullptr, batch);
      }
      c->level0_in_lds = first_fused && !c->keep_levels && s.detector != HESS_DETECTOR_DOG;
      if (first_fused) {
        l = 2;
      } else if (c->has_taps0) {
        ProfScope ps = book_pyramid(small_octaves, true, (double)batch * og.plane * (direct_u8 ? 5.0 : 8.0));
        if (direct_u8)
          launch_gauss(st, nullptr, (const uint8_t*)dev, pitch, (long long)image_stride, plane_ptr(gauss, 0, 0),
                       og.wa, og.h, batch, c->taps0);
        else
          launch_gauss(st, src_f, nullptr, og.wa, og.plane, plane_ptr(gauss, 0, 0), og.wa, og.h, batch, c->taps0);
      } else {
        HIP_TRY(c, hipMemcpyAsync(plane_ptr(gauss, 0, 0), src_f, (size_t)batch * og.plane * 4, hipMemcpyDeviceToDevice, st));
      }
    }
    for (; l < s.level_max; l++) {
      const Level lv = level(o, l);
      if (l == 1 && o >= 1 && top_route(o - 1) == kTopRides) {  // with the previous octave's top level
        const Level top = level(o - 1, s.level_max);
        ProfScope ps = book_pyramid(small_octaves, o - 1 == 0, top.bytes + lv.bytes, top.in_lds);
        if (launch_gauss_pair(st, top.job, lv.job, batch)) c->zero_filled = c->zero_filled || top.job.zero != nullptr;
        else { launch_level(top.job); launch_level(lv.job); }
      } else {
        ProfScope ps = book_pyramid(small_octaves, o == 0, lv.bytes, lv.in_lds);
        launch_level(lv.job);
      }
    }
    if (top_route(o) != kTopRides) {  // (a riding one is launched by octave o + 1, above)
      const Level top = level(o, s.level_max);
      if (top_route(o) == kTopCollected) {
        top_jobs[ntop++] = top.job;
        top_bytes += top.bytes;
        top_in_lds += top.in_lds;
      } else {
        ProfScope ps = book_pyramid(small_octaves, o == 0, top.bytes, top.in_lds);
        launch_level(top.job);
      }
    }
  }
  if (ntop) {  // the top levels collected beside the chain, one launch (booked as one, whatever it takes)
    ProfScope ps = book_pyramid(small_octaves, false, top_bytes, top_in_lds);
    // (+ det-H / gradient of levels 0..level_ds-1 of the chain-launched octaves, from HBM: hessian_low_levels)
    LowLevels low{&g, gauss, deth, got, s.norm, chain_from, s.level_ds};
    if (launch_gauss_multi(st, top_jobs, ntop, batch, &low)) {
      for (int k = 0; k < ntop; k++) c->zero_filled = c->zero_filled || top_jobs[k].zero != nullptr;
    } else {
      // refused: other tap counts than 17-25, or top levels without det-H of their own (HESS_NO_TOP_FUSION with a chain)
      for (int k = 0; k < ntop; k++) launch_level(top_jobs[k]);
      for (int o = chain_from; o < g.noct; o++) launch_hessian(st, g, o, gauss, deth, got, s.norm, batch, 0, s.level_ds - 1);
    }
  }
  small_octaves.close();
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[1], st));
  // (det-H of levels 0 .. level_max-1: by the launch that reads the level as its source; of the top level: by the launch
  // that produces it, or here)
  if (!top_fused) {  // the octaves' top levels from HBM, one launch for all of them
    double px = 0;
    for (int o = 0; o < g.noct; o++) px += g.o[o].plane;
    ProfScope ps(c, HESS_K_HESSIAN, (double)batch * px * 8.0);
    // this launch also clears the buffers of the detection stages (no fill launch of its own in the chain)
    launch_hessian_level(st, g, gauss, deth, s.level_max, s.norm[s.level_max], batch, user_mode ? nullptr : c->zeroed.p,
                         c->zeroed_used);
    c->zero_filled = !user_mode;
  }
  if (s.detector == HESS_DETECTOR_DOG) {
    // ---- difference of Gaussians (ComputeDOG_Kernel): D_l = G_l - G_(l-1), levels 1..dog+2, over the det-H planes the
    // launches above wrote (level 0 keeps its det-H, as in the test oracle).  The DoG schedule is the Hessian one with one
    // more level per octave and no top-level fusion (top_fused is false: level dog+2 is stored, its det-H comes from
    // hessian_rows4 with the fill of the detection buffers) and no level chain (it needs level_max == level_ds + 1).
    double px = 0;
    for (int o = 0; o < g.noct; o++) px += g.o[o].plane;
    ProfScope ps(c, HESS_K_HESSIAN, (double)batch * px * 12.0 * s.level_max);
    launch_dog_planes(st, g, gauss, deth, s.level_max, batch);
  }
  return 0;
}

// ---- extrema + ordered list (DetectKeypointsEX part 2 + GenerateFeatureList), top-K: the list is left in c->d_list ----
static int enqueue_detection(hess_ctx* c, int batch, const LimitParams& lp) {
  const hess_params& p = c->p;
  const Schedule& s = c->sch;
  const Geom& g = c->g;
  hipStream_t st = c->st;
  const float* gauss = (const float*)c->gauss.p;
  const float* deth = (const float*)c->deth.p;
  DetectParams dp;
  dp.thr = p.dog_threshold;
  dp.thr0 = (p.subpixel ? 0.8f : 1.0f) * p.dog_threshold;                            // ProgramCU.cu:897
  dp.edge = (p.edge_threshold + 1) * (p.edge_threshold + 1) / p.edge_threshold;      // ProgramCU.cu:913
  dp.subpixel = p.subpixel;
  Geom gx = g;  // the extrema scan's segment length
  if (c->sw.stream_rows > 0) set_stream_rows(gx, c->sw.stream_rows);      // HESS_STREAM_ROWS (A/B switch; a multiple of 3)
  else if (batch <= policy::kLatencyBatch) set_stream_rows(gx, kStreamRows / policy::kLatencyStreamRowsDiv);  // shorter segments, twice the wavefronts
  if (!c->zero_filled)  // overflow flags, row counts, histogram, masks (normally cleared by octave 0's top-level launch)
    HIP_TRY(c, hipMemsetAsync(c->zeroed.p, 0, c->zeroed_used, st));
  DetectStore dstore;
  dstore.found = (RawKey*)c->found.p;
  dstore.ntask = extrema_tasks(gx);
  dstore.stride = (long long)c->found_tasks * kDetectSlots + c->cap_raw;
  dstore.task_count = (int*)c->task_count.p;
  dstore.spill_count = (int*)c->found_count.p;
  dstore.cap_spill = c->cap_raw;
  dstore.hist = c->use_topk ? (unsigned*)c->hist.p : nullptr;
  if (dstore.ntask > c->found_tasks) { set_err(c, "detection store laid out for %d scan tasks, the batch has %d", c->found_tasks, dstore.ntask); return HESS_ERR_ARG; }
  {
    // algorithmic bytes: every det-H level of every octave is read once (4 B R per level-pixel)
    double det_bytes = 0;
    for (int o = 0; o < g.noct; o++) det_bytes += 4.0 * s.level_num * g.o[o].plane;
    ProfScope ps(c, HESS_K_EXTREMA, det_bytes * batch);
    launch_extrema_mark(st, gx, dp, gauss, deth, (uint64_t*)c->rowmask.p, (int*)c->rowcnt.p, dstore, batch,
                        s.detector == HESS_DETECTOR_DOG);
  }
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[2], st));
  {
    ProfScope ps(c, HESS_K_EXTREMA, 0.0);
    launch_extrema_place(st, g, lp, dstore, (const uint64_t*)c->rowmask.p, (const int*)c->rowcnt.p, (int*)c->rowoff.p,
                         (int*)c->level_count.p, (int*)c->raw_total.p, (int*)c->overflow.p, (int*)c->place_ticket.p,
                         (int*)c->place_flag.p, (RawKey*)c->raw.p, c->cap_raw, batch);
  }
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[3], st));
  // ---- top-K (LimitFeatureCount(0) -> SelectTopK) ----
  c->d_list = (const RawKey*)c->raw.p;
  c->d_list_total = (const int*)c->raw_total.p;
  c->cap_list = c->cap_raw;
  if (c->use_topk) {
    ProfScope ps(c, HESS_K_TOPK, 0.0);
    launch_topk(st, g, p.feature_count_threshold, c->d_list, c->d_list_total, c->cap_raw,
                (unsigned*)c->hist.p, (RawKey*)c->sel.p, (int*)c->sel_total.p, c->cap_sel, batch, c->tk.p, (int*)c->overflow.p);
    c->d_list = (const RawKey*)c->sel.p;
    c->d_list_total = (const int*)c->sel_total.p;
    c->cap_list = c->cap_sel;
  }
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[4], st));
  return 0;
}

// ---- orientation (GetFeatureOrientations), multi-orientation expansion (ReshapeFeatureListCPU), descriptors
// (GetFeatureDescriptors) over the list in c->d_list ----
// user: a caller's keypoints (enqueue_user: no expansion, one descriptor launch over the whole lists of all images); orient =
// false: they came with their angle.
static int enqueue_features(hess_ctx* c, const LimitParams& lp, int batch, int pixtype, int desc_format, bool user, bool orient) {
  const Geom& g = c->g;
  hipStream_t st = c->st;
  FeatureBuffers fb;
  fb.list = c->d_list; fb.list_total = c->d_list_total; fb.cap_list = c->cap_list;
  fb.recs = (FRec*)c->recs.p; fb.ocount = (int*)c->ocount.p;
  fb.foffset = (int*)c->foffset.p; fb.fsrc = (int*)c->fsrc.p;
  fb.feat_total = (int*)c->feat_total.p; fb.feat_first = (int*)c->feat_first.p; fb.img_base = (int*)c->img_base.p;
  fb.keys = (HostKeypoint*)c->keys.p; fb.desc = c->dim ? (float*)c->desc.p : nullptr; fb.cap_feat = c->cap_feat;
  const float* got = (const float*)c->got.p;
  if (orient) {
    ProfScope ps(c, HESS_K_ORIENT, 0.0);
    launch_orientation(st, g, orient_params(c, user), fb, got, batch);
  }
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[5], st));
  launch_feature_scan(st, g, lp, (c->multi && !user) ? 1 : 0, fb, (int*)c->overflow.p, (int*)c->h_small.p, batch);
  if (c->stage_events) HIP_TRY(c, hipEventRecord(c->ev[6], st));
  DescParams dsp = desc_params(c, pixtype, desc_format, user);
  if (user) c->parts = Parts{};  // one launch
  else choose_parts(c, batch);
  const Parts& parts = c->parts;
  int first = 0;
  for (int k = 0; k < parts.n; k++) {
    ProfScope ps(c, HESS_K_DESCRIPTOR, 0.0);  // (per launch, so that the counts agree with a kernel trace)
    dsp.first_image = first;
    dsp.part = parts.features ? k : 0;
    dsp.part_den = parts.features ? parts.n : 1;
    launch_descriptor(st, g, dsp, fb, got, user ? batch : parts.end[k] - first, user ? 0 : c->seen_features);
    if (k < parts.n - 1) HIP_TRY(c, hipEventRecord(c->cp.ev_part[k], st));
    if (!parts.features) first = parts.end[k];
  }
  HIP_TRY(c, hipEventRecord(c->ev[7], st));
  return 0;
}

// Enqueue the whole path for the run's `batch` images.
int enqueue(hess_ctx* c, const PendingRun& r) {
  // Stage timers (SiftGPU::_timing[2..10]) only when asked for: hess_params.verbose bit 1 (the reference's _timingS,
  // SiftGPU.cpp:433-464: its stage times, too, are only meaningful when it synchronises at stage ends) or the bench's
  // per-kernel profile.  An event record between two kernels leaves the stream idle for about 6 us.
  c->stage_events = (c->p.verbose & 2) != 0;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->st));
  const bool user_mode = hess::user_mode(c);
  if (!(user_mode && c->user_on_current))  // SIFT_SKIP_FILTERING: the resident pyramid is reused
    if (int rc = enqueue_pyramid(c, r)) return rc;
  if (user_mode) return enqueue_user(c, r.batch, r.desc_format);
  LimitParams lp;
  lp.method = c->p.truncate_method;
  lp.threshold = c->p.feature_count_threshold;
  if (int rc = enqueue_detection(c, r.batch, lp)) return rc;
  return enqueue_features(c, lp, r.batch, r.pixtype, r.desc_format, false, true);
}

// User-supplied keypoints (PyramidCU::GenerateFeatureListTex, PyramidCU.cpp:555-718), one list per image of the batch: the
// keys go up as the caller gave them (they lie in the pinned block since the set call) together with the per-level table
// of the scale rule, key_bin_kernel bins them to levels and packs the fixed-point records, then the strongest orientation
// on the device unless supplied, descriptors.  Nothing here waits for the device.
// Rectangles (HESS_KEYS_RECTANGLES; IsUsingRectDescription, SiftPyramid.cpp:345-354): (x, y) is the corner, s the width
// and o the height; the scale that is binned is min(s, o) / 12 (PyramidCU.cpp:598-599), the record holds the width as the
// scale's 8.8 fixed point and the height o / octave_sigma as it is, a float (:618-622); no orientation pass
// (PyramidCU.cpp:522), and the descriptor launch is descriptor_rect_kernel's.
size_t user_block_bytes(int total, int nimg) {
  return (size_t)total * (sizeof(hess_keypoint) + 4) + (size_t)nimg * 8 + 16 + (size_t)kMaxOct * kMaxDog * sizeof(KeyLevel);
}

int enqueue_user(hess_ctx* c, int batch, int desc_format) {
  const hess_params& p = c->p;
  const Schedule& s = c->sch;
  const Geom& g = c->g;
  hipStream_t st = c->st;
  const int total = c->user_total, cap = user_cap(c);
  static_assert(sizeof(hess_keypoint) == sizeof(HostKeypoint), "keypoint layout");
  if (cap > c->cap_raw || cap > c->cap_sel || cap > c->cap_feat || c->h_user.bytes < user_block_bytes(total, batch) ||
      c->d_user.bytes < c->h_user.bytes) {
    set_err(c, "keypoint lists (%d per image) exceed the reserved feature storage", cap);
    return HESS_ERR_NOMEM;  // plan() sizes storage for 2*num+8 when a list is set
  }
  // the block behind the keys: (first, count) per image, the parity hook's levels (one image), the level table
  char* const hb = (char*)c->h_user.p;
  size_t at = (size_t)total * sizeof(hess_keypoint);
  const size_t o_first = at;
  int* const fc = (int*)(hb + at);
  for (int b = 0, first = 0; b < batch; b++) {
    fc[2 * b] = first;
    fc[2 * b + 1] = c->user_counts[b];
    first += c->user_counts[b];
  }
  at += (size_t)batch * 8;
  const bool given = batch == 1 && (int)c->user_levels.size() == total;
  const size_t o_levels = at;
  if (given) {
    memcpy(hb + at, c->user_levels.data(), (size_t)total * 4);
    at += (size_t)total * 4;
  }
  at = (at + 15) & ~(size_t)15;
  const size_t o_table = at;
  KeyLevel* const table = (KeyLevel*)(hb + at);
  const float sigma_half_step = powf(2.0f, 0.5f / g.dog);
  float octave_sigma = first_octave_sigma(c);
  for (int octave = 0; octave < g.noct; octave++, octave_sigma *= 2.0f) {
    for (int level = 1; level <= g.dog; level++) {
      const float level_sigma = s.level_sigma[level] * octave_sigma;
      table[octave * g.dog + (level - 1)] = KeyLevel{level_sigma / sigma_half_step, level_sigma * sigma_half_step, octave_sigma, level_sigma};
    }
  }
  at += (size_t)g.nlev * sizeof(KeyLevel);
  const char* const db = (const char*)c->d_user.p;
  HIP_TRY(c, hipMemcpyAsync(c->d_user.p, hb, at, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(c->overflow.p, 0, 64, st));  // overflow words + feature_scan_kernel's arrival counter
  HIP_TRY(c, hipMemsetAsync(c->level_count.p, 0, (size_t)batch * g.nlev * 4, st));
  c->d_list = (const RawKey*)c->raw.p;
  c->d_list_total = (const int*)c->raw_total.p;
  c->cap_list = cap;
  KeyBinJob job;
  job.keys = (const HostKeypoint*)db;
  job.first_count = (const int*)(db + o_first);
  job.levels = given ? (const int*)(db + o_levels) : nullptr;
  job.table = (const KeyLevel*)(db + o_table);
  job.total = total; job.max_count = c->user_max; job.nlev = g.nlev;
  job.rect = c->user_rect ? 1 : 0;
  job.origin = p.lowe_origin ? 0.0f : 0.5f;
  job.member = (int*)c->kmember.p;
  job.level_count = (int*)c->level_count.p;
  job.list = (RawKey*)c->raw.p; job.recs = (FRec*)c->recs.p; job.list_total = (int*)c->raw_total.p;
  job.kmap = (int*)c->kmap.p;
  job.host_kmap = c->host_direct ? (int*)c->h_kmap.p : nullptr;
  job.cap_list = cap;
  job.overflow = (int*)c->overflow.p;
  launch_key_bin(st, job, batch);
  if (c->stage_events) for (int e = 1; e <= 4; e++) HIP_TRY(c, hipEventRecord(c->ev[e], st));
  LimitParams lp;
  lp.method = 0;
  lp.threshold = -1;  // LimitFeatureCount returns at once for existing keypoints (SiftPyramid.cpp:203)
  return enqueue_features(c, lp, batch, HESS_PIX_U8, desc_format, true, !c->user_have_orientation);
}

}  // namespace hess
