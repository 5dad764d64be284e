// Fused photometric forward: warp (backproject -> project -> bilinear grid_sample, border padding) + SSIM/L1
// reprojection loss for both source frames + per-pixel minimum against the identity terms + masked sum, for ALL
// scales, in one launch — the warped images never reach HBM (fs_photo_warp + fs_photo_loss_fwd wrote and re-read
// 8 x [B,3,H,W] floats, and staged the target tile once per scale).
// Replaces (reference): MonoDepth2Decoder._generate_images_pred (monodepth2_decoder.py:61-116; FishEyeDecoder
// :355-411), compute_reprojection_loss (:118-128; SSIM monodepth_utils.py:184-215) and the per-pixel min / masking
// of compute_total_reprojection_loss (:226-272, 292).
//
// Structure: a wave owns a strip of 62 columns x 16 rows of one (batch element, scale): lane l holds column
// x0 - 1 + l, so the 3-tap horizontal window sums are two DPP adds (wave_shr / wave_shl, no LDS), and the rows are
// walked top to bottom with the last two rows' horizontal sums kept in registers (the vertical 3-tap sum is two
// adds).  Reflection padding = the halo lane / halo row evaluates the reflected pixel.  Source texels are gathered
// straight from global memory: consecutive lanes sample neighbouring texels (coalesced up to the warp's local
// stretch), the four scales of a strip run back to back on the same XCD, so the source rows stay cache resident.
// FS_HIPCC_FLAGS: -fno-slp-vectorize
// (SLP packing into v_pk_add/mul_f32 costs register shuffles here and keeps the DPP shifts from folding into the adds)
#include <algorithm>
// photo_common.h's row helpers (hsum3, f2, ldg) under this file's contraction mode: the header switches it on in front of
// them and it stays on from there — last include, so that it reaches nothing but this file's own code
#define FS_PHOTO_CONTRACT_FAST
#include "photo_common.h"

// fused multiply-adds allowed in this file (the library builds with -ffp-contract=off to mirror the unfused ATen
// arithmetic of the staged kernels; here an FMA only removes a rounding and a third of the VALU instructions)
#pragma clang fp contract(fast)
// the channel triple C3, the 8-byte tap pair load ldg2 and the whole backward body: shared with photo_multi.hip
#include "photo_bwd_body.h"

namespace {

constexpr int FW = 62;    // output columns per wave (lanes 1..62; lanes 0 and 63 are halo)
constexpr int FRH = 16;   // output rows per wave

// (hsum3, the per-lane frame pair f2 and the row load ldg live at the end of photo_common.h: the identity kernel of
// photometric.hip walks rows the same way)

struct Row {       // one image row of a strip: horizontal 3-tap sums + the raw values (needed when it is the centre)
  float t[3], tt[3];
  f2 x[3], xx[3], xt[3];        // component = source frame
  float rt[3];
  f2 rx[3];
  bool ov[2];
};


// FISH = false: pinhole geometry inlined with per-lane / per-row invariants hoisted and reciprocals by v_rcp_f32
// (1 ulp; the staged kernels divide) — a sample coordinate moves by < 1e-4 px.  FISH = true: the shared ray-table
// geometry (photo_common.h).
template <bool WRITE_PRED, bool FISH>
__global__ __launch_bounds__(256) void photo_fused_fwd_kernel(const FsPhotoArgs p, int SX, int SY, int nwaves) {
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
  const int H = p.H, W = p.W;
  const unsigned HW = (unsigned)(H * W);
  const int h = p.dh[s], w = p.dw[s];
  const float* ge = p.geo + (long)b * GEO_STRIDE;
  const float* timg = p.img0 + (long)b * 3 * HW;
  const float* srcs[2] = {p.img_src[0] + (long)b * 3 * HW, p.img_src[1] + (long)b * 3 * HW};
  const float* dmap = p.depth[s] + (long)b * h * w;
  const float* identb = p.ident + (long)b * 2 * HW;
  uint8_t* selb = p.sel + ((long)s * p.B + b) * HW;
  const int x = sx * FW - 1 + lane;
  const int xr = min(max(refl(x, W), 0), W - 1);
  const bool col_out = lane >= 1 && lane <= FW && x < W;
  const int ys = sy * FRH;
  const int seed = p.noise_seed_ptr ? (*p.noise_seed_ptr & 0x3fffffff) : p.noise_seed;
  const float k9 = 1.f / 9.f, k81 = 1.f / 81.f, k3 = 1.f / 3.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const float iwm1 = 1.f / wm1, ihm1 = 1.f / hm1;
  const bool have_mask = p.warp_mask || p.patched_mask;
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
  f2 Pm[12];                    // (frame 0, frame 1) entries of the two projection matrices
  if (!FISH) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ra[i] = ge[3 * i] * pxf;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) Pm[k] = f2{ge[18 + k], ge[30 + k]};
  double acc = 0.0;

  // one row: fill `r0` (row y = ys - 1 + it) and, from the third row on, finish the window centred on row y - 1 = `r1`
  auto step = [&](const Row& r2, const Row& r1, Row& r0, const int it) {
    const int y = ys - 1 + it;
    const int yr = min(max(refl(y, H), 0), H - 1);
    const unsigned ob = (unsigned)(yr * W + xr) * 4u;
#pragma unroll
    for (int c = 0; c < 3; ++c) r0.rt[c] = ldg(timg + c * HW, ob);
    Geo g;
    if (FISH) {
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
    if (FISH) {
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        project_ray(p, b, H, W, ge, f, g);
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
      for (int f = 0; f < 2; ++f)
        mv[f] = p.warp_mask ? p.warp_mask[(long)b * HW + om[f]] : (float)p.patched_mask[(long)b * HW + om[f]];
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
          float* pr = p.pred + (((long)s * 2 + f) * p.B + b) * 3 * HW + (unsigned)(y * W + x);
          pr[0] = r0.rx[0][f]; pr[HW] = r0.rx[1][f]; pr[2 * HW] = r0.rx[2][f];
          p.ov[(((long)s * 2 + f) * p.B + b) * HW + (unsigned)(y * W + x)] = r0.ov[f] ? 1 : 0;
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
      float best = INFINITY; int bi = 2;
      if (!p.motion_mask) {          // identity candidates (the auto-mask); a motion mask replaces them (:243-246)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          uint32_t key = (uint32_t)((((long)s * 2 + f) * p.B + b) * HW + i);
          float v = ldg(identb + f * HW, i * 4u) + tie_noise(seed, key);
          if (f == 0 || v < best) { best = v; bi = f; }
        }
      }
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const float rv = 0.85f * (ssim_sum[f] * k3) + 0.15f * (l1[f] * k3);
        float v = r1.ov[f] ? rv : 100.f;
        if (v < best) { best = v; bi = 2 + f; }
      }
      // a selected reprojection term whose sample missed the source frame is the constant 100 (:231-235): value only,
      // no gradient (cannot happen next to the identity candidates, which are always below 100)
      if ((bi == 2 && !r1.ov[0]) || (bi == 3 && !r1.ov[1])) bi = 4;   // (static indices: a runtime index spills the row)
      selb[i] = (uint8_t)bi;
      double pm = p.patched_mask ? p.patched_mask[(long)b * HW + i] : 1.0;
      acc += (double)best * pm;
    }
  };

  static_assert((FRH + 2) % 3 == 0, "the row ring is rotated by unrolling three steps");
  Row A, B, C;
  for (int it = 0; it < FRH + 2; it += 3) {
    step(B, C, A, it);
    step(C, A, B, it + 1);
    step(A, B, C, it + 2);
  }
  acc = wave_sum_d(acc);
  if (lane == 0) atomicAdd(p.loss_sums + s * p.B + b, acc);
}


// =============================================================================================================
// Fused backward: d loss / d depth_s and the per-strip partials of d loss / d P_f, recomputing the warp instead
// of reading the eight warped images back (fs_photo_loss_bwd staged pred + target tiles per scale through LDS).
// A wave owns (batch element, scale, source frame, strip of 60 columns x 32 rows) and walks the rows once with two
// register rings, three stages per step at row y:
//   A  warp row y (both the values and the sampler Jacobian d pred / d (ix, iy)), horizontal window sums
//   B  window centre y-1: SSIM-derivative coefficients A + B x(q) + C t(q) for this frame where the per-pixel minimum
//      selected it (sel == 2 + f), horizontally box-summed (the transpose of the window gather)
//   C  output row y-2: vertical box sum of the coefficient rows -> d loss / d pred, + the L1 term, through the sampler
//      Jacobian, the projection and the depth upsample.
// Reflection padding: halo lanes / rows hold the reflected pixel; the virtual positions x = -1, W and y = -1, H
// (which receive window contributions of the border centres) push their gradient through the reflected pixel's
// chain — the chain is linear in d pred, so that equals folding them onto the reflected pixel.
// =============================================================================================================
// (BW, BRH, the low-res LDS tile, the row structs and the kernel's body: photo_bwd_body.h, shared with photo_multi.hip)

template <bool FISH>
__global__ __launch_bounds__(256) void photo_fused_bwd_kernel(const FsPhotoArgs p, int SX, int SY, int nwaves) {
  __shared__ float s_dd[4][LDS_R * LDS_C];
  photo_bwd_body<FISH, TwoFrames>(p, SX, SY, nwaves, s_dd);
}

}  // namespace

extern "C" int fs_photo_fused_fwd(const FsPhotoArgs* a, void* stream) {
  if (!a || !a->img0 || !a->img_src[0] || !a->img_src[1] || !a->geo || (!a->ident && !a->motion_mask) || !a->sel ||
      !a->loss_sums)
    return FS_EINVAL;
  if (a->S < 1 || a->S > 4 || a->B < 1 || a->H < 2 || a->W < 2) return FS_EINVAL;
  if ((a->lut_ptrs != nullptr) != (a->mei != nullptr)) return FS_EINVAL;
  if ((a->pred != nullptr) != (a->ov != nullptr)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s]) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + FW - 1) / FW, SY = (a->H + FRH - 1) / FRH;
  const long nwaves = (long)a->B * a->S * SY * SX;
  long nblk = (nwaves + 3) / 4;
  nblk = (nblk + 7) / 8 * 8;
  if (nblk > 0x7fffffffL) return FS_EINVAL;
  if ((long)a->H * a->W * 3 >= 0x40000000L) return FS_EINVAL;          // 32-bit plane offsets
  const dim3 grid((unsigned)nblk), blk(256);
  const bool fish = a->lut_ptrs != nullptr;
  if (a->pred) {
    if (fish) hipLaunchKernelGGL((photo_fused_fwd_kernel<true, true>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
    else hipLaunchKernelGGL((photo_fused_fwd_kernel<true, false>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  } else {
    if (fish) hipLaunchKernelGGL((photo_fused_fwd_kernel<false, true>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
    else hipLaunchKernelGGL((photo_fused_fwd_kernel<false, false>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  }
  return fs_launch_status();
}

extern "C" int64_t fs_photo_fused_bwd_tiles(int H, int W) {
  if (H < 2 || W < 2) return -1;
  return (int64_t)((W + BW - 1) / BW) * ((H + BRH - 1) / BRH);
}

extern "C" int fs_photo_fused_bwd(const FsPhotoArgs* a, void* stream) {
  if (!a || !a->img0 || !a->img_src[0] || !a->img_src[1] || !a->geo || !a->sel || !a->dP || !a->mask_sum)
    return FS_EINVAL;
  if (a->S < 1 || a->S > 4 || a->B < 1 || a->H < 2 || a->W < 2) return FS_EINVAL;
  if ((a->lut_ptrs != nullptr) != (a->mei != nullptr)) return FS_EINVAL;
  if ((long)a->H * a->W * 3 >= 0x40000000L) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || !a->d_depth[s]) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + BW - 1) / BW, SY = (a->H + BRH - 1) / BRH;
  const long nwaves = (long)a->B * a->S * 2 * SY * SX;
  long nblk = (nwaves + 3) / 4;
  nblk = (nblk + 7) / 8 * 8;
  if (nblk > 0x7fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  if (a->lut_ptrs) hipLaunchKernelGGL(photo_fused_bwd_kernel<true>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  else hipLaunchKernelGGL(photo_fused_bwd_kernel<false>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}
