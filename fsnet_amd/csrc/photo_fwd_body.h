// Body of the fused photometric forward, shared by photo_fused.hip (two source frames, pinhole and fisheye) and
// photo_multi.hip / photo_mei_multi.hip (one to four source frames, pinhole / fisheye), as photo_bwd_body.h is for the
// backward: the kernels differ in
// how many frame pairs a wave walks, where the running minimum waits between two walks and in the argument struct, which
// the policy `FR` (photo_common.h) answers — everything else is this one text.  Included after photo_common.h and
// photo_bwd_body.h (F2u, ldg2) by files that allow fused multiply-adds (FS_PHOTO_CONTRACT_FAST).
//
// Structure: a wave owns a strip of 62 columns x 16 rows of one (batch element, scale): lane l holds column
// x0 - 1 + l, so the 3-tap horizontal window sums are two DPP adds (wave_shr / wave_shl, no LDS), and the rows are
// walked top to bottom with the last two rows' horizontal sums kept in registers (the vertical 3-tap sum is two
// adds).  Reflection padding = the halo lane / halo row evaluates the reflected pixel.  Source texels are gathered
// straight from global memory: consecutive lanes sample neighbouring texels (coalesced up to the warp's local
// stretch), the four scales of a strip run back to back on the same XCD, so the source rows stay cache resident.
// The strip is walked once per frame PAIR: the two frames of a pair ride in the two components of the f2 lanes.  Between
// two walks the running minimum and its index of the strip's pixels wait in a per-lane LDS slot (5 bytes per pixel,
// written and read by the same lane: no barrier, no bank conflict); a launch of one pair never touches it, and with
// TwoFrames the pair loop, `first` / `last`, `have2` and the slot fold away at compile time (that kernel passes no slot).
// A half-filled pair (N = 1, 3) points its second component at the pair's first frame, so nothing that is not there is
// read, and leaves it out of the minimum and of pred / ov.
#pragma once
#pragma clang fp contract(fast)

namespace {

constexpr int FW = 62;    // output columns per wave (lanes 1..62; lanes 0 and 63 are halo)
constexpr int FRH = 16;   // output rows per wave

// (hsum3, the per-lane frame pair f2 and the row load ldg live at the end of photo_common.h: the identity kernel of
// photometric.hip walks rows the same way)

struct Row {       // one image row of a strip: horizontal 3-tap sums + the raw values (needed when it is the centre)
  float t[3], tt[3];
  f2 x[3], xx[3], xt[3];        // component = frame of the pair
  float rt[3];
  f2 rx[3];
  bool ov[2];
};

// FISH = false: pinhole geometry inlined with per-lane / per-row invariants hoisted and reciprocals by v_rcp_f32
// (1 ulp; the staged kernels divide) — a sample coordinate moves by < 1e-4 px.  FISH = true (FsPhotoArgs,
// FsPhotoMeiMultiArgs): the shared ray-table geometry (photo_common.h).
// s_best / s_bi: the wave's slot [row][lane] of the running minimum (nullptr where FR walks one pair).
template <bool WRITE_PRED, bool FISH, class FR, class Args>
__device__ __forceinline__ void photo_fwd_body(const Args& p, int SX, int SY, int nwaves, float (*s_best)[64],
                                               uint8_t (*s_bi)[64]) {
  // XCD-contiguous logical block order: consecutive logical blocks (= the scales of one strip row) share an L2
  const int nblk = gridDim.x;
  const int lb = ((int)blockIdx.x & 7) * (nblk >> 3) + ((int)blockIdx.x >> 3);
  const int wv = __builtin_amdgcn_readfirstlane(lb * 4 + ((int)threadIdx.x >> 6));
  if (wv >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int sx = wv % SX;
  int rest = wv / SX;
  const int s = rest % p.S; rest /= p.S;
  const int sy = rest % SY;
  const int b = rest / SY;
  const int N = FR::count(p), npair = FR::pairs(N);
  const int H = p.H, W = p.W;
  const unsigned HW = (unsigned)(H * W);
  const int h = p.dh[s], w = p.dw[s];
  const float* ge = p.geo + (long)b * FR::geo_stride(N);
  const float* timg = p.img0 + (long)b * 3 * HW;
  const float* dmap = p.depth[s] + (long)b * h * w;
  const float* identb = p.ident + (long)b * N * HW;
  uint8_t* selb = p.sel + ((long)s * p.B + b) * HW;
  const int x = sx * FW - 1 + lane;
  const int xr = min(max(refl(x, W), 0), W - 1);
  const bool col_out = lane >= 1 && lane <= FW && x < W;
  const int ys = sy * FRH;
  const int seed = p.noise_seed_ptr ? (*p.noise_seed_ptr & 0x3fffffff) : p.noise_seed;
  const float k9 = 1.f / 9.f, k81 = 1.f / 81.f, k3 = 1.f / 3.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const float iwm1 = 1.f / wm1, ihm1 = 1.f / hm1;
  const bool have_mask = FR::has_ov_mask(p);
  const bool no_ovm = p.no_overlap_mask != 0;

  // per-lane invariants of the depth upsample (ATen upsample_bilinear2d, align_corners=True) and of the ray
  const float sh = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
  const float sw = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
  // (the tap pair starts at dx0 <= w - 2 so that it is one 8-byte load; at the right border the weight moves over)
  const float fxu = sw * (float)xr;
  const int dx0 = w > 1 ? min((int)fxu, w - 2) : 0;
  const float dlx = w > 1 ? fxu - (float)dx0 : 0.f;
  const float pxf = (float)xr;
  float ra[3] = {0.f, 0.f, 0.f};
  if (!FISH) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ra[i] = ge[3 * i] * pxf;
  }
  double acc = 0.0;

  for (int pr = 0; pr < npair; ++pr) {
    const int fa = 2 * pr;
    const bool have2 = FR::full(pr, N);
    const int fb = have2 ? fa + 1 : fa;            // a half-filled pair computes its first frame twice and drops the copy
    const bool first = pr == 0, last = pr == npair - 1;
    const float* srcs[2] = {p.img_src[fa] + (long)b * 3 * HW, p.img_src[fb] + (long)b * 3 * HW};
    f2 Pm[12];                    // (first, second frame of the pair) entries of the two projection matrices
#pragma unroll
    for (int k = 0; k < 12; ++k) Pm[k] = f2{ge[18 + fa * 12 + k], ge[18 + fb * 12 + k]};

    // one row: fill `r0` (row y = ys - 1 + it) and, from the third row on, finish the window centred on row y - 1 = `r1`
    auto step = [&](const Row& r2, const Row& r1, Row& r0, const int it) {
      const int y = ys - 1 + it;
      const int yr = min(max(refl(y, H), 0), H - 1);
      const unsigned ob = (unsigned)(yr * W + xr) * 4u;
#pragma unroll
      for (int c = 0; c < 3; ++c) r0.rt[c] = ldg(timg + c * HW, ob);
      Geo g;
      if constexpr (FISH) {
        pixel_ray(p, p.depth[s], b, yr, xr, H, W, h, w, ge, g);
      } else {
        // depth upsample: the row taps are wave-uniform
        const float fyu = sh * (float)yr;
        const int dy0 = (int)fyu, dy1 = dy0 + (dy0 < h - 1 ? 1 : 0);
        const float dly = fyu - (float)dy0;
        float d00, d01, d10, d11;
        if (w > 1) {
          const F2u a = ldg2(dmap, (unsigned)(dy0 * w + dx0) * 4u), c2 = ldg2(dmap, (unsigned)(dy1 * w + dx0) * 4u);
          d00 = a.a; d01 = a.b; d10 = c2.a; d11 = c2.b;
        } else {
          d00 = d01 = ldg(dmap, (unsigned)(dy0 * w) * 4u); d10 = d11 = ldg(dmap, (unsigned)(dy1 * w) * 4u);
        }
        g.D = (1.f - dly) * ((1.f - dlx) * d00 + dlx * d01) + dly * ((1.f - dlx) * d10 + dlx * d11);
        const float pyf = (float)yr;
#pragma unroll
        for (int i = 0; i < 3; ++i) g.r[i] = (ra[i] + ge[3 * i + 1] * pyf) + ge[3 * i + 2];
      }
      unsigned og[2][2];
      f2 w01[2], w23[2];           // per frame: the sampler weights of the upper / lower tap pair
      unsigned om[2];
      bool inb[2];
      f2 ixu2, iyu2;
      if constexpr (FISH) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          project_ray(p, b, H, W, ge, f ? fb : fa, g);     // the pair's geo entries (TwoFrames: 0, 1)
          ixu2[f] = g.ixu; iyu2[f] = g.iyu;
        }
      } else {
        const float cx_ = g.D * g.r[0], cy_ = g.D * g.r[1], cz_ = g.D * g.r[2];
        const f2 X = Pm[0] * cx_ + Pm[1] * cy_ + Pm[2] * cz_ + Pm[3];
        const f2 Y = Pm[4] * cx_ + Pm[5] * cy_ + Pm[6] * cz_ + Pm[7];
        const f2 Zp = (Pm[8] * cx_ + Pm[9] * cy_ + Pm[10] * cz_ + Pm[11]) + 1e-7f;
        const f2 iz = f2{__builtin_amdgcn_rcpf(Zp.x), __builtin_amdgcn_rcpf(Zp.y)};
        const f2 u = X * iz, v = Y * iz;
        // Project3D normalisation followed by grid_sample's align_corners=True un-normalisation
        const f2 un = (u * iwm1 - 0.5f) * 2.f, vn = (v * ihm1 - 0.5f) * 2.f;
        ixu2 = (un + 1.f) * 0.5f * wm1;
        iyu2 = (vn + 1.f) * 0.5f * hm1;
      }
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        // bilinear taps with border clamping; the tap pair always starts at x0 <= W - 2 / y0 <= H - 2 (at the right /
        // bottom border the weight moves to the second tap: same value) so that (x0, x0 + 1) is one 8-byte load
        const float ixu = ixu2[f], iyu = iyu2[f];
        const float ix = fminf(fmaxf(ixu, 0.f), wm1), iy = fminf(fmaxf(iyu, 0.f), hm1);
        const float fx0 = fminf(floorf(ix), wm1 - 1.f), fy0 = fminf(floorf(iy), hm1 - 1.f);
        const float wx = ix - fx0, wy = iy - fy0;
        const int tx0 = (int)fx0, ty0 = (int)fy0;
        og[f][0] = (unsigned)(ty0 * W + tx0) * 4u;
        og[f][1] = og[f][0] + (unsigned)W * 4u;
        const f2 wxs = f2{1.f - wx, wx};
        w01[f] = wxs * (1.f - wy); w23[f] = wxs * wy;
        // nearest sample of patched_mask (fisheye: x ray-table mask) with zeros padding, round half to even
        const float xn = nearbyintf(ixu), yn = nearbyintf(iyu);
        inb[f] = xn >= 0.f && xn <= wm1 && yn >= 0.f && yn <= hm1;
        om[f] = inb[f] ? (unsigned)((int)yn * W + (int)xn) : 0u;
      }
      // all gathers of the row in flight together: (x0, x0 + 1) of a tap row arrive as one register pair
      f2 tap[2][3][2];
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const F2u v2 = ldg2(srcs[f] + c * HW, og[f][k]);
            tap[f][c][k] = f2{v2.a, v2.b};
          }
      float mv[2] = {1.f, 1.f};
      if (have_mask) {
#pragma unroll
        for (int f = 0; f < 2; ++f) mv[f] = FR::ov_mask(p, (long)b * HW + om[f]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        r0.t[c] = hsum3(r0.rt[c]);
        r0.tt[c] = hsum3(r0.rt[c] * r0.rt[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f2 v;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const f2 q = w01[f] * tap[f][c][0] + w23[f] * tap[f][c][1];      // (x0 column, x0 + 1 column) partial sums
          v[f] = q.x + q.y;
        }
        r0.rx[c] = v;
        r0.x[c] = hsum3(v);
        r0.xx[c] = hsum3(v * v);
        r0.xt[c] = hsum3(v * r0.rt[c]);
      }
#pragma unroll
      for (int f = 0; f < 2; ++f)
        r0.ov[f] = no_ovm || (inb[f] && mv[f] == 1.f);   // overlapped_mask=False: every sample counts (border-clamped)
      if (WRITE_PRED) {
        if (col_out && y >= ys && y < ys + FRH && y < H) {
#pragma unroll
          for (int f = 0; f < 2; ++f) {
            if (f == 1 && !have2) continue;
            const long pl = ((long)s * N + (fa + f)) * p.B + b;
            float* prd = p.pred + pl * 3 * HW + (unsigned)(y * W + x);
            prd[0] = r0.rx[0][f]; prd[HW] = r0.rx[1][f]; prd[2 * HW] = r0.rx[2][f];
            p.ov[pl * HW + (unsigned)(y * W + x)] = r0.ov[f] ? 1 : 0;
          }
        }
      }
      if (it < 2) return;
      const int yc = y - 1;          // window centre row; rows y-2 (r2), y-1 (r1), y (r0)
      f2 ssim_sum = splat(0.f), l1 = splat(0.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float sy_ = (r2.t[c] + r1.t[c]) + r0.t[c], syy = (r2.tt[c] + r1.tt[c]) + r0.tt[c];
        const float muy = sy_ * k9;
        // (co)variances as (9 sum(ab) - sum(a) sum(b)) / 81: with the rounded 1 / 9 in both terms of E[ab] - E[a] E[b] its
        // rounding error, times mu^2, survives the cancellation and shifts every SSIM term the same way (+1.5e-7 on average)
        const float sgy = (9.f * syy - sy_ * sy_) * k81;
        const f2 sxs = (r2.x[c] + r1.x[c]) + r0.x[c], sxx = (r2.xx[c] + r1.xx[c]) + r0.xx[c],
                 sxy = (r2.xt[c] + r1.xt[c]) + r0.xt[c];
        const f2 mux = sxs * k9;
        const f2 sgx = (9.f * sxx - sxs * sxs) * k81, sgxy = (9.f * sxy - sxs * sy_) * k81;
        const f2 n = (2.f * mux * muy + C1) * (2.f * sgxy + C2);
        const f2 d = (mux * mux + muy * muy + C1) * (sgx + sgy + C2);
        const f2 q = FISH ? n / d : n * f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        const f2 sv = (1.f - q) * 0.5f;
        ssim_sum += f2{fminf(fmaxf(sv.x, 0.f), 1.f), fminf(fmaxf(sv.y, 0.f), 1.f)};
        const f2 df = r1.rt[c] - r1.rx[c];
        l1 += f2{fabsf(df.x), fabsf(df.y)};
      }
      if (col_out && yc < H) {       // (yc >= ys always: it >= 2)
        const unsigned i = (unsigned)(yc * W + x);
        const int j = it - 2;        // row of the strip
        float best; int bi;
        if (first) {
          best = INFINITY; bi = N;
          if (!p.motion_mask) {        // identity candidates (the auto-mask); a motion mask replaces them (:243-246)
#pragma unroll
            for (int f = 0; f < MAXF; ++f) {
              if (f < N) {
                uint32_t key = (uint32_t)((((long)s * N + f) * p.B + b) * HW + i);
                float v = ldg(identb + f * HW, i * 4u) + tie_noise(seed, key);
                if (f == 0 || v < best) { best = v; bi = f; }
              }
            }
          }
        } else {
          best = s_best[j][lane]; bi = s_bi[j][lane];
        }
        // reprojection candidates in the reference's cat order; strict <: the first of equal candidates wins.  A winning
        // term whose sample missed the source frame is the constant 100 (:231-235): index 2 N, value only, no gradient
        // (cannot happen next to the identity candidates, which are always below 100)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const float rv = 0.85f * (ssim_sum[f] * k3) + 0.15f * (l1[f] * k3);
          const float v = r1.ov[f] ? rv : 100.f;
          if ((f == 0 || have2) && v < best) { best = v; bi = r1.ov[f] ? N + fa + f : 2 * N; }
        }
        if (last) {
          selb[i] = (uint8_t)bi;
          double pm = p.patched_mask ? p.patched_mask[(long)b * HW + i] : 1.0;
          acc += (double)best * pm;
        } else {
          s_best[j][lane] = best; s_bi[j][lane] = (uint8_t)bi;
        }
      }
    };

    static_assert((FRH + 2) % 3 == 0, "the row ring is rotated by unrolling three steps");
    Row A, B, C;
    for (int it = 0; it < FRH + 2; it += 3) {
      step(B, C, A, it);
      step(C, A, B, it + 1);
      step(A, B, C, it + 2);
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) atomicAdd(p.loss_sums + s * p.B + b, acc);
}

}  // namespace
