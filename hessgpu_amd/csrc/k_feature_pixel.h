// k_feature_pixel.h -- the body of descriptor_pixel_kernel, included by k_feature.hip once per output format:
//   HESS_PIXEL_KERNEL  the kernel's name    HESS_PIXEL_U8  false: float descriptors, true: bytes (HESS_DESC_FORMAT_U8)
// Two kernels from one text instead of one kernel with a second template parameter or a shared inlined body: the float
// kernel keeps its name (descriptor_pixel_kernel<host mirror>: profiles and bench.py know it by that) AND its code -- with
// the format as a run-time branch the float form needed 72 registers and 16 - 28 bytes of scratch per lane, through an
// inlined body 70 - 72 registers in another allocation; this way its instructions are the ones it had (71, no scratch).
// What is not the raster -- which features, the feature's record, plane and frame, normalisation and store -- are the helpers
// the three descriptor kernels share (k_feature.hip, "shared by the descriptor kernels").
// (no include guard: meant to be included more than once; everything it uses is defined above the include)
template <bool HOST_MIRROR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PX_WAVES, PX_WAVES))) void HESS_PIXEL_KERNEL(Geom g, DescParams dp, const RawKey* list,
                                                               int cap_list, const FRec* recs,
                                                               const int* fsrc, const int* feat_total,
                                                               const int* feat_first, const int* img_base,
                                                               const float* got, HostKeypoint* keys, float* desc,
                                                               int cap_feat) {
  constexpr bool U8 = HESS_PIXEL_U8;
  __shared__ __attribute__((aligned(16))) float dl[4][128];
  __shared__ __attribute__((aligned(16))) unsigned long long hist[4][PX_WAVE_U64];
  __shared__ __attribute__((aligned(16))) uint4 rowtab[4][64];  // per wavefront: the rows of the current raster band
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const DescImage im = desc_image(dp, feat_total, feat_first, img_base);

  static_assert(sizeof(HostKeypoint) == 24 && sizeof(hist) >= 256 * 24, "record staging fits the sums");
  keypoint_records<HOST_MIRROR>(dp, reinterpret_cast<uint32_t*>(&hist[0][0]), im, list, cap_list, recs, fsrc, cap_feat, keys);
  if (!desc) return;
  unsigned long long* const sums = &hist[wv][0];
  {
    uint4* const z = reinterpret_cast<uint4*>(sums);
    for (int i = lane; i < PX_WAVE_U64 / 2; i += 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  // LDS byte address of the lane's copy, as a float (stage B adds the word's offset in floating point)
  const float mycopy_f = (float)(unsigned)(unsigned long long)(lds_u64*)(sums + (lane % PX_COPIES) * PX_COPY_U64);
  const uint32_t theta_end_bits = theta_end(dp);

  for (int mw = first_feature(dp, wv); mw < im.ftotal; mw += gridDim.x * 4) {
    const Feature f = load_feature(g, im, im.ffirst + im.ftotal - 1 - mw, list, cap_list, recs, fsrc, cap_feat, got);
    const __amdgpu_buffer_rsrc_t grsrc = f.grsrc;
    const int width = f.width, height = f.height;
    const OrientedFrame fr = oriented_frame(dp, f);
    const float kx = fr.kx, ky = fr.ky;
    const float spt = fr.spt, crspt = fr.crspt, srspt = fr.srspt, anglef = fr.anglef;
    const float ext = 2.5f * fr.bsz;  // half extent of the footprint's bounding box
    const float xmin = fmaxf(1.5f, floorf(kx - ext) + 0.5f);
    const float ymin = fmaxf(1.5f, floorf(ky - ext) + 0.5f);
    const float xmax = fminf(width - 1.5f, floorf(kx + ext) + 0.5f);
    const float ymax = fminf(height - 1.5f, floorf(ky + ext) + 0.5f);
    // fixed-point scale 2^sh: 0.75 (spt + 1)^2 < 2^e bounds every sum, sh = 32 - e (the oracle's frexpf)
    const float bound = 0.75f * (spt + 1.0f) * (spt + 1.0f);
    const int sh = min(max(32 - ((int)((__float_as_uint(bound) >> 23) & 0xFFu) - 126), 0), 30);
    const float scale = __uint_as_float((uint32_t)(127 + sh) << 23), rscale = __uint_as_float((uint32_t)(127 - sh) << 23);
    // (the same in every lane: the box is the feature's)
    const int nxs = __builtin_amdgcn_readfirstlane((xmax >= xmin) ? (int)(xmax - xmin) + 1 : 0);
    const int nys = __builtin_amdgcn_readfirstlane((ymax >= ymin) ? (int)(ymax - ymin) + 1 : 0);
    // Row spans.  The window |u| < 2.5, |v| < 2.5 is a rotated square: of the box's pixels 1 / (|c| + |s|)^2 lie inside
    // (0.61 on average over the angles), so the raster runs over the window's own rows instead: row y of the box keeps
    // the pixels x_lo(y) .. x_hi(y), the real-arithmetic solution of the two inequalities for x, slightly widened (a
    // SUPERSET of the pixels that pass the test: every pixel is still tested with the floats the oracle uses, so which
    // pixels count does not depend on the spans; integer sums do not depend on the order either).
    // Bands of <= 64 rows (lane = row) and <= dp.px_band pixels: prefix sums of the span lengths give every row its first
    // place S in the band's sequence; a 64-bit word per step holds the places where rows start (bit S mod 64 of word
    // S / 64, lane w keeps word w), so the lane of place t = 64 step + lane finds its row with two mbcnt and reads the
    // row's entry (first pixel's index - S, x - S, y) from LDS.
    // (a coefficient below 1e-3 per pixel: that inequality is left out -- it cuts the corners of the box only -- so that the
    // rounding of u, v, 1e-6 at most, stays below 1e-3 pixel in x; the spans are widened by PX_SPAN_EPS = 0.02)
    const float rA = (fabsf(crspt) > 1.0e-3f) ? 1.0f / crspt : 0.0f, rB = (fabsf(srspt) > 1.0e-3f) ? 1.0f / srspt : 0.0f;
    const int px_band = __builtin_amdgcn_readfirstlane(dp.px_band);
    for (int ib = 0; ib < nxs; ib += px_band) {  // (column bands: a box wider than a band -- no detected feature's is)
    const int ncol = min(nxs - ib, px_band);
    const int band_rows = min(64, px_band / ncol);
    for (int jb = 0; jb < nys; jb += band_rows) {
    const int nrow = min(band_rows, nys - jb);
    int T;
    uint32_t mword_lo, mword_hi;
    {
      const float yrow = ymin + (float)(jb + lane), dyr = yrow - ky;
      float lo = -3.0e38f, hi = 3.0e38f;
      if (rA != 0.0f) {  // |crspt dx + srspt dy| < 2.5
        const float t1 = (-2.5f - srspt * dyr) * rA, t2 = (2.5f - srspt * dyr) * rA;
        lo = fminf(t1, t2); hi = fmaxf(t1, t2);
      }
      if (rB != 0.0f) {  // |crspt dy - srspt dx| < 2.5
        const float t1 = (crspt * dyr - 2.5f) * rB, t2 = (crspt * dyr + 2.5f) * rB;
        lo = fmaxf(lo, fminf(t1, t2)); hi = fminf(hi, fmaxf(t1, t2));
      }
      const float off = kx - xmin;  // pixel i of the row: x = xmin + i, dx = i - off
      const float flo = fmaxf(ceilf(lo + off - PX_SPAN_EPS), (float)ib), fhi = fminf(floorf(hi + off + PX_SPAN_EPS), (float)(ib + ncol - 1));
      const int len = (lane < nrow && fhi >= flo) ? (int)(fhi - flo) + 1 : 0;
      const int ilo = (int)flo;
      const int incl = wave_inclusive_scan(len);
      const int S = incl - len;
      T = __builtin_amdgcn_readlane(incl, 63);
      const uint64_t ne = __builtin_amdgcn_ballot_w64(len > 0);
      const int r = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ne >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ne, 0u));
      // (dl[wv] is also the float staging area of the feature's end: wavefront fences keep the compiler from moving the
      // 64-bit accesses across the float ones, which type-based alias analysis would allow; they emit no instruction)
      unsigned long long* const starts = reinterpret_cast<unsigned long long*>(&dl[wv][0]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      starts[lane] = 0ull;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (len > 0) {
        (void)__hip_atomic_fetch_or(starts + (S >> 6), 1ull << (S & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        rowtab[wv][r] = make_uint4((uint32_t)(((int)ymin + jb + lane) * width + (int)xmin + ilo - S),
                                   __float_as_uint(xmin + (float)(ilo - S)), __float_as_uint(yrow), 0u);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const unsigned long long mw = starts[lane];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      mword_lo = (uint32_t)mw; mword_hi = (uint32_t)(mw >> 32);
    }
    const int nit = (T + 63) >> 6;
    int step = 0, rows_before = -1;  // (rows that started before this step's 64 places) - 1
    int tl = lane;
    float tf = (float)lane;

    // stage A: the lane's pixel of N steps (row by the start bits, place in the row), keypoint-frame coordinates, window
    // test and gather, issued back to back
    auto stage_a = [&](auto& ck) {
      constexpr int N = std::remove_reference_t<decltype(ck)>::N;
#pragma unroll
      for (int q = 0; q < N; q++) {
        const uint32_t mlo = (uint32_t)__builtin_amdgcn_readlane((int)mword_lo, step), mhi = (uint32_t)__builtin_amdgcn_readlane((int)mword_hi, step);
        const uint64_t m64 = ((uint64_t)mhi << 32) | mlo;
        int rr = rows_before + (int)__builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u)) + (__builtin_amdgcn_inverse_ballot_w64(m64) ? 1 : 0);
        rows_before += __builtin_popcountll(m64);
        rr = (int)min((unsigned)rr, 63u);  // (steps past the band's end: any entry, the lane is switched off below)
        const uint4 e = rowtab[wv][rr];
        const float xf = __uint_as_float(e.y) + tf, yf = __uint_as_float(e.z);
        const unsigned goff = (e.x + (unsigned)tl) * 8u;
        const float dx = xf - kx, dy = yf - ky;
        const float u = fmaf(crspt, dx, srspt * dy);
        ck.v[q] = fmaf(crspt, dy, -(srspt * dx));
        const bool in = (tl < T) & (fabsf(u) < 2.5f) & (fabsf(ck.v[q]) < 2.5f);
        ck.u[q] = in ? u : 3.0f;  // (outside the window)
        const dfloat2 gv = __builtin_amdgcn_raw_buffer_load_b64(grsrc, (int)(in ? goff : 0u), 0, 0);
        ck.cc[q] = make_float2(gv.x, gv.y);
        tl += 64; tf += 64.0f; step++;
      }
    };
    // stage B: the pixel's weight, bin and cell split; four 64-bit additions of two fixed-point values each.
    // (The word's LDS address is formed in floating point from the three floors -- small integers, exact -- and
    // converted once; the four cells' validity masks are combined as wave masks on the scalar unit.)
    auto stage_b = [&](const auto& ck) {
      constexpr int N = std::remove_reference_t<decltype(ck)>::N;
#pragma unroll
      for (int q = 0; q < N; q++) {
        const float u = ck.u[q], v = ck.v[q];
        if (!__any(u < 2.5f)) continue;  // (wave-uniform) a step wholly outside the window: the box's corners
        const float ww = dm_expf_inrange(-0.125f * fmaf(u, u, v * v));
        float theta = (anglef - ck.cc[q].y) * rpi;
        theta = (theta < 0) ? theta + 8.0f : theta;
        // 0 <= theta < theta_end as ONE unsigned compare of the bit patterns (see descriptor_kernel)
        const uint64_t m_hit = __builtin_amdgcn_ballot_w64((u < 2.5f) & (__float_as_uint(theta) < theta_end_bits));
        // b0 = floor(theta), 0..7; theta == 8 (-di only) counts as b0 = 7 with weights (0, 1): the same sums, since word
        // 7 = [bin 7 | bin 0] (the oracle says bin 0 += weight, bin 1 += 0)
        const float fo = fminf(floorf(theta), 7.0f);
        const float wb1 = theta - fo, wb0 = 1.0f - wb1;
        const float au = u + 1.5f, av = v + 1.5f;
        const float fu = floorf(au), fv = floorf(av);  // -1 .. 3: cells fu, fu + 1 / fv, fv + 1 where they exist
        const float wx1 = au - fu, wx0 = 1.0f - wx1;
        const float wy1 = av - fv, wy0 = 1.0f - wy1;
        const float wt = (ww * ck.cc[q].x) * scale;
        const float a0 = wt * wy0, a1 = wt * wy1;
        const float b00 = a0 * wx0, b01 = a0 * wx1, b10 = a1 * wx0, b11 = a1 * wx1;
        const unsigned addr = (unsigned)(int)fmaf(fv, 256.0f, fmaf(fu, 64.0f, fmaf(fo, 8.0f, mycopy_f)));  // byte address in LDS
        lds_u64* const p = (lds_u64*)(unsigned long long)addr;
        const uint64_t mx0 = __builtin_amdgcn_ballot_w64(fu >= 0.0f), mx1 = __builtin_amdgcn_ballot_w64(fu <= 2.0f);
        const uint64_t my0 = m_hit & __builtin_amdgcn_ballot_w64(fv >= 0.0f), my1 = m_hit & __builtin_amdgcn_ballot_w64(fv <= 2.0f);
#define HESS_PX_ADD(P, B)                                                                                          \
  (void)__hip_atomic_fetch_add((P), (unsigned long long)__float2uint_rz(fmaf((B), wb0, 0.5f)) |                    \
                                       ((unsigned long long)__float2uint_rz(fmaf((B), wb1, 0.5f)) << 32),           \
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
        if (__builtin_amdgcn_inverse_ballot_w64(my0 & mx0)) HESS_PX_ADD(p, b00);
        if (__builtin_amdgcn_inverse_ballot_w64(my0 & mx1)) HESS_PX_ADD(p + 8, b01);
        if (__builtin_amdgcn_inverse_ballot_w64(my1 & mx0)) HESS_PX_ADD(p + 32, b10);
        if (__builtin_amdgcn_inverse_ballot_w64(my1 & mx1)) HESS_PX_ADD(p + 40, b11);
#undef HESS_PX_ADD
      }
    };
    {
      constexpr int UN = HESS_PX_UNROLL;
      // software pipeline: the gathers of the next chunk are in flight while the current chunk is accumulated
      PixChunk<UN> ca, cb;
      stage_a(ca);
      for (int it0 = 0; it0 < nit; it0 += 2 * UN) {
        stage_a(cb);
        stage_b(ca);
        if (it0 + UN >= nit) break;
        stage_a(ca);
        stage_b(cb);
      }
    }
    }  // row bands
    }  // column bands
    // The copies' sums: lane (cell, q) reads words 2q, 2q+1 of its cell in every copy (one 16-byte read each), adds the
    // four 32-bit halves apart and clears the words for the next feature.  It owns bins 2q, 2q+1:
    //   bin 2q   = low half of word 2q   + high half of word 2q-1 (lane q-1 of the quad, q = 0: word 7, lane q = 3)
    //   bin 2q+1 = low half of word 2q+1 + high half of word 2q
    __builtin_amdgcn_wave_barrier();
    uint4 t = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int cpy = 0; cpy < PX_COPIES; cpy++) {
      uint4* const w = reinterpret_cast<uint4*>(sums + cpy * PX_COPY_U64 + 2 * lane);
      const uint4 x = *w;
      t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w;
      *w = make_uint4(0u, 0u, 0u, 0u);
    }
    {
      const uint32_t prev_hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)t.w, 0x93 /* quad_perm:[3,0,1,2] */, 0xF, 0xF, true);
      const float f0 = (float)(t.x + prev_hi) * rscale, f1 = (float)(t.z + t.y) * rscale;
      *reinterpret_cast<float2*>(&dl[wv][2 * lane]) = make_float2(f0, f1);
    }
    __builtin_amdgcn_wave_barrier();
    // The end is this kernel's own text on top of finish_values, not finish_descriptor: -half folds des[k] + des[k+4] out of
    // the unfolded staging layout, and with the folded values handed over through LDS once more (or folded in registers
    // ahead of the staging) the raster's loops came out with other waits and scalar instructions, the float form with a 72nd
    // register and scratch (profiles/r14_desc_helpers.txt).
    const int dim = dp.half_sift ? 64 : 128;
    float* const dout = desc_at(desc, im.obase + f.oidx, dim, U8);
    float* const hout = (HOST_MIRROR && dp.hdesc) ? desc_at(dp.hdesc, im.obase + f.oidx, dim, U8) : nullptr;
    if (dp.half_sift) {  // des[k] += des[k+4], ProgramCU.cu:1782-1785: lane < 32 -> cell lane/2, k = 2 (lane & 1) + {0, 1}
      DescValues<2> v = 0.0f;
      if (lane < 32) {
        const float* cellp = &dl[wv][(lane >> 1) * 8 + (lane & 1) * 2];
        const float2 lo = *reinterpret_cast<const float2*>(cellp), hi = *reinterpret_cast<const float2*>(cellp + 4);
        v.x = lo.x + hi.x; v.y = lo.y + hi.y;
      }
      finish_values<HOST_MIRROR, 2>(dp, U8, lane, v, dout, hout);
    } else {
      finish_values<HOST_MIRROR, 4>(dp, U8, lane, staged_values<4>(dl[wv], lane), dout, hout);
    }
    __builtin_amdgcn_wave_barrier();  // (dl and the sums are rewritten by the next feature)
  }
}
