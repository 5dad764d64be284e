// Photometric loss chain, forward + backward, as HBM-bound gather / stencil kernels.
// Replaces (reference, all eager ATen):
//   MonoDepth2Decoder._generate_images_pred          monodepth2_decoder.py:61-116
//     F.interpolate(bilinear, align_corners=True)     :68-69
//     K / pinv(K) on host                             :82-85
//     BackprojectDepth / Project3D                    monodepth_utils.py:101-165
//     F.grid_sample(bilinear, border) / (nearest)     monodepth2_decoder.py:98-101,110-116
//   compute_reprojection_loss (SSIM + L1)             monodepth2_decoder.py:118-128, monodepth_utils.py:184-215
//   compute_total_reprojection_loss (min / masks)     monodepth2_decoder.py:205-292
// All four scales run in ONE launch per stage (every stage works at full resolution; only the
// low-res depth map differs).  Images stay planar NCHW fp32 exactly as the data layer hands them over.
// This file holds what runs unfused: setup, identity planes and pose gradient, one kernel each for the two-source entry
// points (fs_photo_*) and the N-frame ones (fs_photo_multi_setup / _identity / _pose_grad); the fused forward and
// backward are photo_fused.hip / photo_multi.hip.
// FS_HIPCC_FLAGS: -fno-slp-vectorize
// (as in photo_fused.hip: SLP packing of the row-walking identity kernel's window sums turns each DPP add into a DPP move
// plus a packed add, costs 12 VGPRs — one wave per SIMD of occupancy — and parks a row's raw values in LDS)
#include "photo_common.h"
#include <algorithm>

namespace {

// ---------------------------------------------------------------------------------------------
// setup: K, K^-1 (f64 adjugate == pinv for a regular K), P_f = (K T_f)[:3] for the nsrc frames of a geo record of
// `stride` floats (fs_photo_setup: 2 frames in 48; fs_photo_multi_setup: 18 + 12 nsrc); bump the noise seed
// ---------------------------------------------------------------------------------------------
__global__ void photo_setup_kernel(const float* __restrict__ P2, const PtrTable<const float> tp, int nsrc, int stride,
                                   float* __restrict__ geo, int B, int* __restrict__ seed_counter, int fisheye) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (seed_counter && b == 0) *seed_counter += 1;      // tie-break noise seed of this step (read by the loss forward)
  if (b >= B) return;
  double k[3][3];
  // fisheye: the transform acts on the ray-table point directly (monodepth2_decoder.py:379-381), the camera model
  // follows it (cam2image) -> "K" is the identity here, P_f = T_f[:3], and fs_photo_pose_grad's K^T dP is dT itself
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i][j] = fisheye ? (i == j ? 1.0 : 0.0) : (double)P2[b * 12 + i * 4 + j];
  double c00 = k[1][1] * k[2][2] - k[1][2] * k[2][1];
  double c01 = k[1][2] * k[2][0] - k[1][0] * k[2][2];
  double c02 = k[1][0] * k[2][1] - k[1][1] * k[2][0];
  double det = k[0][0] * c00 + k[0][1] * c01 + k[0][2] * c02;
  double inv[3][3];
  inv[0][0] = c00 / det; inv[1][0] = c01 / det; inv[2][0] = c02 / det;
  inv[0][1] = (k[0][2] * k[2][1] - k[0][1] * k[2][2]) / det;
  inv[1][1] = (k[0][0] * k[2][2] - k[0][2] * k[2][0]) / det;
  inv[2][1] = (k[0][1] * k[2][0] - k[0][0] * k[2][1]) / det;
  inv[0][2] = (k[0][1] * k[1][2] - k[0][2] * k[1][1]) / det;
  inv[1][2] = (k[0][2] * k[1][0] - k[0][0] * k[1][2]) / det;
  inv[2][2] = (k[0][0] * k[1][1] - k[0][1] * k[1][0]) / det;
  float* g = geo + (long)b * stride;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { g[i * 3 + j] = (float)inv[i][j]; g[9 + i * 3 + j] = (float)k[i][j]; }
#pragma unroll
  for (int f = 0; f < MAXF; ++f) {                     // (unrolled: static indices into the pointer table)
    if (f >= nsrc) break;
    // the three rows of T_f and K from registers: the table's pointers carry no __restrict__, so reading either between
    // the stores to g would be a fresh load per product
    float T[12];
    for (int e = 0; e < 12; ++e) T[e] = tp.p[f][(long)b * 16 + e];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {
        float a = 0.f;
        for (int m = 0; m < 3; ++m) a += (float)k[i][m] * T[m * 4 + j];
        g[18 + f * 12 + i * 4 + j] = a;
      }
  }
}

// ---------------------------------------------------------------------------------------------
// identity reprojection losses (scale independent) + patched-mask sum
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float reproj_at(const float* __restrict__ xp, const float* __restrict__ tp, int y, int x,
                                           int H, int W) {
  // xp, tp: planar [3][H][W] of one batch element; returns 0.85*mean_c SSIM + 0.15*mean_c |t - x|
  int ys[3] = {refl(y - 1, H), y, refl(y + 1, H)}, xs[3] = {refl(x - 1, W), x, refl(x + 1, W)};
  float ssim_sum = 0.f, l1 = 0.f;
  const long HW = (long)H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        float xv = xp[c * HW + (long)ys[a] * W + xs[b]], tv = tp[c * HW + (long)ys[a] * W + xs[b]];
        sx += xv; sy += tv; sxx += xv * xv; syy += tv * tv; sxy += xv * tv;
      }
    const float k = 1.f / 9.f;
    float mux = sx * k, muy = sy * k;
    float sgx = sxx * k - mux * mux, sgy = syy * k - muy * muy, sgxy = sxy * k - mux * muy;
    float n = (2.f * mux * muy + C1) * (2.f * sgxy + C2);
    float d = (mux * mux + muy * muy + C1) * (sgx + sgy + C2);
    ssim_sum += fminf(fmaxf((1.f - n / d) * 0.5f, 0.f), 1.f);
    l1 += fabsf(tp[c * HW + (long)y * W + x] - xp[c * HW + (long)y * W + x]);
  }
  return 0.85f * (ssim_sum / 3.f) + 0.15f * (l1 / 3.f);
}

// One block = a 64 x 4 pixel tile of one sample: the nine planes (target + two source frames, three channels each)
// are staged ONCE with their reflected one-pixel halo into LDS and both identity terms read their 3x3 windows from
// there, in the same order and with the same arithmetic as reproj_at() above (bit-identical results).  History: the
// first version gathered 108 values per pixel from global memory (the target window twice), 154 us per step for 65 MB
// of input; this tile form took 91 us (1.55x the pixels fetched for the halo, 4-byte staging loads behind two integer
// divisions, 108 LDS reads per pixel, the target's window sums once per frame).  The training step now calls the
// row-walking kernel below (fs_photo_identity_rows); fs_photo_identity stays exported as the reference-order form the
// tests measure the new one against.
constexpr int ID_TW = 64, ID_TH = 4, ID_HW = ID_TW + 2, ID_HH = ID_TH + 2;

__global__ __launch_bounds__(256) void photo_ident_kernel(const FsPhotoArgs p) {
  __shared__ float tile[9][ID_HH][ID_HW];
  const int b = blockIdx.y;
  const int tiles_x = (p.W + ID_TW - 1) / ID_TW;
  const int ty_i = blockIdx.x / tiles_x, tx_i = blockIdx.x - ty_i * tiles_x;
  const int y0 = ty_i * ID_TH, x0 = tx_i * ID_TW;
  const long HW = (long)p.H * p.W;
  const int t = threadIdx.x;
  for (int e = t; e < 9 * ID_HH * ID_HW; e += 256) {
    const int pl = e / (ID_HH * ID_HW), r = e - pl * (ID_HH * ID_HW);
    const int hy = r / ID_HW, hx = r - hy * ID_HW;
    // (rows / columns past the image only feed pixels that are not written; clamp keeps the address valid)
    const int yy = refl(min(y0 + hy - 1, p.H), p.H), xx = refl(min(x0 + hx - 1, p.W), p.W);
    const float* src = pl < 3 ? p.img0 : p.img_src[(pl - 3) / 3];
    tile[pl][hy][hx] = src[((long)b * 3 + pl % 3) * HW + (long)yy * p.W + xx];
  }
  __syncthreads();
  const int tx = t & (ID_TW - 1), ty = t / ID_TW;
  const int y = y0 + ty, x = x0 + tx;
  double msum = 0.0;
  if (y < p.H && x < p.W) {
    const long i = (long)y * p.W + x;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      float ssim_sum = 0.f, l1 = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float xv = tile[3 + 3 * f + c][ty + a][tx + q], tv = tile[c][ty + a][tx + q];
            sx += xv; sy += tv; sxx += xv * xv; syy += tv * tv; sxy += xv * tv;
          }
        const float k = 1.f / 9.f;
        float mux = sx * k, muy = sy * k;
        float sgx = sxx * k - mux * mux, sgy = syy * k - muy * muy, sgxy = sxy * k - mux * muy;
        float n = (2.f * mux * muy + C1) * (2.f * sgxy + C2);
        float d = (mux * mux + muy * muy + C1) * (sgx + sgy + C2);
        ssim_sum += fminf(fmaxf((1.f - n / d) * 0.5f, 0.f), 1.f);
        l1 += fabsf(tile[c][ty + 1][tx + 1] - tile[3 + 3 * f + c][ty + 1][tx + 1]);
      }
      p.ident[((long)b * 2 + f) * HW + i] = 0.85f * (ssim_sum / 3.f) + 0.15f * (l1 / 3.f);
    }
    msum = p.patched_mask ? p.patched_mask[(long)b * HW + i] : 1.0;
  }
  __shared__ double sh[4];
  msum = block_sum_d(msum, sh);
  if (threadIdx.x == 0) atomicAdd(p.mask_sum + b, msum);
}

// ---------------------------------------------------------------------------------------------
// The same two planes by walking rows (the decomposition of photo_fused_fwd_kernel): a wave owns a strip of 62 columns x
// ID_RS rows of one sample, lane l holds column x0 - 1 + l (lanes 0 and 63 are halo), the horizontal 3-tap sums are two
// DPP adds, the last two rows' sums stay in registers and the vertical sum is two adds: no LDS, every plane is read once
// apart from the halo, and the target's window sums are formed once for both frames.  Reflection padding = the halo
// lane / halo row loads the reflected pixel.  The nine taps are added as (row sums of three) of three instead of one
// after the other, so a value may differ from reproj_at()'s in the last bits; after the sums it is the same unfused
// arithmetic except for the quotient (div_nr) and the two means over the channels (x 1/3), with sigma_x, sigma_t and
// sigma_xt in one expression shape: a frame equal to the target still gives exactly 0.
// The window sums are taken of (value - 0.5) and the (co)variances formed as (9 sum(ab) - sum(a) sum(b)) / 81.  Variances do
// not move with a shift and images live in [0, 1], so the two terms that cancel are ~ 10 x smaller than with the raw
// values and the result's fp32 noise with them (largest error against f64 over the shapes of the test: 2.5e-7, the tile
// kernel's 1.6e-6).  And no rounded constant stands inside the cancellation: reproj_at()'s sum k - mu mu with k = fl(1 / 9)
// keeps that constant's rounding error times mu^2, which raises every SSIM term by 1.5e-7 on average: a tenth of the
// noise, but one-sided, so it shows in the loss sums (tests/test_photo_fused_seams_gpu.py).  The next row's loads are
// issued into the ring slot whose raw values are no longer needed before the current row is worked on.
// Strip height: a strip re-reads (and re-sums) 2 halo rows, so ID_RS = 16 costs 12.5 % more rows than the image has
// (8: 25 %, 32: 6 %).  Measured alone at 192x640 / batch 12 and 384x384 / batch 16, inputs from HBM: 8 rows 43.8 /
// 68.6 us, 12: 38.6 / 53.4, 16: 35.1 / 45.9, 24: 40.7 / 47.0, 32: 37.4 / 51.0 (the tile kernel: 90.9 / 134.7) — the
// 1.5 waves per SIMD of 16 rows hide a row's loads well enough behind the row before it.  (Taken with IEEE quotients;
// div_nr below then brought 16 rows to 32.7 / 42.6 us.  docs/LAB_r07.md.)
// ---------------------------------------------------------------------------------------------
// (ID_W = 62 columns, ID_RS = 16 rows: photo_common.h)
// n / d without the scaling steps of the IEEE sequence (ten instructions, a third of the kernel's arithmetic with the
// six quotients of a pixel): v_rcp_f32 (1 ulp) and one Newton step on the quotient with the exact fma remainder.  Within
// 1 ulp of n / d, and exactly 1 for n == d (q = 1 + e, the remainder -d e is exact, q - d e r rounds to 1), which the
// exact zero of equal frames rests on.  d = (mu_x^2 + mu_t^2 + C1)(sigma_x + sigma_t + C2) is neither denormal nor huge.
__device__ __forceinline__ float div_nr(float n, float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  const float q = n * r;
  return __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
}

struct IdRow {
  float rt[3];                        // raw target values, per channel
  f2 rx[3];                           // raw source values (component = frame of the pair)
  float t[3], tt[3];                  // horizontal 3-tap sums
  f2 x[3], xx[3], xt[3];
};

// FR (photo_common.h): TwoFrames = a wave per (sample, strip), both planes; NFrames = a wave per (sample, strip, frame
// pair), a half-filled pair (N = 1, 3) points its second component at the pair's first frame and drops the copy.  The
// file is unfused, so the two instantiations give the same bits per plane.
template <class FR, class Args>
__global__ __launch_bounds__(256) void photo_ident_rows_kernel(const Args p, int SX, int SY, int nwaves) {
  const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
  if (wv >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int N = FR::count(p), npair = FR::pairs(N);
  const int pr = wv % npair;
  int rest = wv / npair;
  const int sx = rest % SX; rest /= SX;
  const int sy = rest % SY, b = rest / SY;
  const int fa = 2 * pr;
  const bool have2 = FR::full(pr, N);
  const int H = p.H, W = p.W;
  const unsigned HW = (unsigned)(H * W);
  const float* timg = p.img0 + (long)b * 3 * HW;
  const float* src0 = p.img_src[fa] + (long)b * 3 * HW;
  const float* src1 = p.img_src[have2 ? fa + 1 : fa] + (long)b * 3 * HW;
  float* out = p.ident + ((long)b * N + fa) * HW;
  const double* pm = p.patched_mask ? p.patched_mask + (long)b * HW : nullptr;
  const int x = sx * ID_W - 1 + lane;
  const int xr = min(max(refl(x, W), 0), W - 1);     // (columns past the halo only feed lanes that are not written)
  const bool col_out = lane >= 1 && lane <= ID_W && x < W;
  const int ys = sy * ID_RS;
  const int nsteps = min(ID_RS, H - ys) + 2;         // rows ys - 1 .. ys + rows of the strip
  double msum = 0.0;

  auto load = [&](IdRow& r, const int it) {
    const int yr = min(max(refl(ys - 1 + it, H), 0), H - 1);
    const unsigned ob = (unsigned)(yr * W + xr) * 4u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      r.rt[c] = ldg(timg + c * HW, ob);
      r.rx[c] = f2{ldg(src0 + c * HW, ob), ldg(src1 + c * HW, ob)};
    }
  };

  // one row: `r0` holds the raw values of row y = ys - 1 + it; from the third row on, finish the window centred on `r1`
  auto step = [&](IdRow& r2, const IdRow& r1, IdRow& r0, const int it) {
    load(r2, min(it + 1, nsteps - 1));               // next row (this step reads r2's sums only); last step: a re-load, unused
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tc = r0.rt[c] - 0.5f;              // (exact from 0.25 up, half an ulp of 0.5 below)
      const f2 xc = r0.rx[c] - 0.5f;
      r0.t[c] = hsum3(tc);
      r0.tt[c] = hsum3(tc * tc);
      r0.x[c] = hsum3(xc);
      r0.xx[c] = hsum3(xc * xc);
      r0.xt[c] = hsum3(xc * tc);
    }
    if (it < 2) return;
    const int yc = ys + it - 2;                      // < H by nsteps
    const float k = 1.f / 9.f, k81 = 1.f / 81.f;
    f2 ssim_sum = splat(0.f), l1 = splat(0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sy_ = (r2.t[c] + r1.t[c]) + r0.t[c], syy = (r2.tt[c] + r1.tt[c]) + r0.tt[c];
      const f2 sxs = (r2.x[c] + r1.x[c]) + r0.x[c], sxx = (r2.xx[c] + r1.xx[c]) + r0.xx[c],
               sxy = (r2.xt[c] + r1.xt[c]) + r0.xt[c];
      const float muy = sy_ * k + 0.5f;
      const f2 mux = sxs * k + 0.5f;
      const float sgy = (9.f * syy - sy_ * sy_) * k81;
      const f2 sgx = (9.f * sxx - sxs * sxs) * k81, sgxy = (9.f * sxy - sxs * sy_) * k81;
      const f2 n = (2.f * mux * muy + C1) * (2.f * sgxy + C2);
      const f2 d = (mux * mux + muy * muy + C1) * (sgx + sgy + C2);
      const f2 sv = (1.f - f2{div_nr(n.x, d.x), div_nr(n.y, d.y)}) * 0.5f;
      ssim_sum += f2{fminf(fmaxf(sv.x, 0.f), 1.f), fminf(fmaxf(sv.y, 0.f), 1.f)};
      const f2 df = r1.rt[c] - r1.rx[c];
      l1 += f2{fabsf(df.x), fabsf(df.y)};
    }
    if (col_out) {
      const float k3 = 1.f / 3.f;                    // (the tile kernel divides by 3: at most one more ulp here)
      const f2 v = 0.85f * (ssim_sum * k3) + 0.15f * (l1 * k3);
      const unsigned i = (unsigned)(yc * W + x);
      out[i] = v.x;
      if (have2) out[HW + i] = v.y;
      if (pr == 0) msum += pm ? pm[i] : 1.0;         // the mask sum is added once, by the first pair's wave
    }
  };

  IdRow A, B, C;
  load(A, 0);
  for (int it = 0; it < nsteps; it += 3) {           // (nsteps >= 3; the row ring is rotated by unrolling three steps)
    step(B, C, A, it);
    if (it + 1 < nsteps) step(C, A, B, it + 1);
    if (it + 2 < nsteps) step(A, B, C, it + 2);
  }
  if (pr == 0) {
    msum = wave_sum_d(msum);                         // mask values are 0 / 1: the f64 sum is exact in any order
    if (lane == 0) atomicAdd(p.mask_sum + b, msum);
  }
}

// (Rounds 1-2 ran the chain as three staged kernels here — warp to HBM, loss forward, loss backward; the fused kernels of
// photo_fused.hip replaced them in round 3 and the staged path, kept behind a switch until round 5, is gone.)

// dT[f][b] (4x4, row 3 = 0) = K^T-contracted dP:  P = K3 * T[:3]  =>  dT[k][j] = sum_i K3[i][k] dP[i][j].
// One block per (b, f) = (blockIdx.x, blockIdx.y): sums the per-tile partials dP[s][b][tile][f of N][12] of the fused
// backward in a fixed order.  A partial is three 16-byte lanes; thread (row lane r of 85, quarter q of 3) strides over
// the S * tiles rows, the 85 lanes are then added in f64 (first version: 4-byte loads, 366 dependent-latency iterations
// per thread — 33 us on the critical path between the loss backward and the pose chain's backward).
// dT: one [B][4][4] output per frame (fs_photo_pose_grad: two tensors; fs_photo_multi_pose_grad: slices of one).
__global__ __launch_bounds__(256) void photo_pose_grad_kernel(const float* __restrict__ geo, int stride,
                                                              const float* __restrict__ dP, const PtrTable<float> dT,
                                                              int N, int B, int S, int tiles) {
  constexpr int RL = 85;
  __shared__ double s_part[RL][12];
  __shared__ float s_g[12];
  const int b = blockIdx.x, f = blockIdx.y;
  const int t = threadIdx.x, q = t % 3, r = t / 3;
  if (r < RL) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int rows = S * tiles;
#pragma unroll 4
    for (int j = r; j < rows; j += RL) {
      const int s = j / tiles, tl = j - s * tiles;
      const float4 v = *reinterpret_cast<const float4*>(dP + ((((long)s * B + b) * tiles + tl) * N + f) * 12 + q * 4);
      a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
    }
    s_part[r][q * 4 + 0] = a0; s_part[r][q * 4 + 1] = a1; s_part[r][q * 4 + 2] = a2; s_part[r][q * 4 + 3] = a3;
  }
  __syncthreads();
  if (t < 12) {
    double v = 0.0;
    for (int g = 0; g < RL; ++g) v += s_part[g][t];
    s_g[t] = (float)v;
  }
  __syncthreads();
  if (t < 16) {
    const float* K = geo + (long)b * stride + 9;
    float* o = (f == 0 ? dT.p[0] : f == 1 ? dT.p[1] : f == 2 ? dT.p[2] : dT.p[3]) + (long)b * 16;
    const int rr = t >> 2, j = t & 3;
    o[t] = rr < 3 ? K[0 * 3 + rr] * s_g[0 * 4 + j] + K[1 * 3 + rr] * s_g[1 * 4 + j] + K[2 * 3 + rr] * s_g[2 * 4 + j] : 0.f;
  }
}

// the identity launch of either argument struct: a wave per (sample, strip, frame pair), four waves a block
template <class FR, class Args> int launch_ident_rows(const Args* a, int npair, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + ID_W - 1) / ID_W, SY = (a->H + ID_RS - 1) / ID_RS;
  const long nwaves = (long)a->B * SY * SX * npair;
  if (nwaves > 0x7ffffff0L) return FS_EINVAL;
  hipLaunchKernelGGL((photo_ident_rows_kernel<FR, Args>), dim3((unsigned)photo_blocks(nwaves, 1)), dim3(256), 0, st, *a,
                     SX, SY, (int)nwaves);
  return fs_launch_status();
}

bool valid(const FsPhotoArgs* a) { return photo_args_ok(a, 2) && photo_fisheye_ok(a); }
bool valid(const FsPhotoMultiArgs* a) {
  return a && a->nsrc >= 1 && a->nsrc <= MAXF && photo_args_ok(a, a->nsrc) && photo_planes_32bit(a);
}

}  // namespace

extern "C" int fs_photo_setup(const float* P2, const float* T0, const float* T1, float* geo, int B, int* seed_counter,
                              int fisheye, void* stream) {
  if (!P2 || !T0 || !T1 || !geo) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const PtrTable<const float> tp = {{T0, T1}};
  hipLaunchKernelGGL(photo_setup_kernel, dim3((B + 63) / 64), dim3(64), 0, st, P2, tp, 2, GEO_STRIDE, geo, B,
                     seed_counter, fisheye);
  return fs_launch_status();
}

// the N-frame setup launch; fisheye: P2 is not read (K = identity)
static int launch_multi_setup(const float* P2, const float* const* T, int nsrc, float* geo, int B, int* seed_counter,
                              int fisheye, void* stream) {
  if (!T || !geo || nsrc < 1 || nsrc > MAXF || B < 1) return FS_EINVAL;
  PtrTable<const float> tp = {};
  for (int f = 0; f < nsrc; ++f) {
    if (!T[f]) return FS_EINVAL;
    tp.p[f] = T[f];
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(photo_setup_kernel, dim3((B + 63) / 64), dim3(64), 0, st, P2, tp, nsrc, geo_stride_n(nsrc), geo, B,
                     seed_counter, fisheye);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_setup(const float* P2, const float* const* T, int nsrc, float* geo, int B,
                                    int* seed_counter, void* stream) {
  if (!P2) return FS_EINVAL;
  return launch_multi_setup(P2, T, nsrc, geo, B, seed_counter, 0, stream);
}

extern "C" int fs_photo_mei_multi_setup(const float* const* T, int nsrc, float* geo, int B, int* seed_counter,
                                        void* stream) {
  return launch_multi_setup(nullptr, T, nsrc, geo, B, seed_counter, 1, stream);
}

extern "C" int fs_photo_identity(const FsPhotoArgs* a, void* stream) {
  if (!valid(a) || !a->ident || !a->mask_sum) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)(((a->W + ID_TW - 1) / ID_TW) * ((a->H + ID_TH - 1) / ID_TH)), a->B);
  hipLaunchKernelGGL(photo_ident_kernel, grid, dim3(256), 0, st, *a);
  return fs_launch_status();
}

extern "C" int fs_photo_identity_rows(const FsPhotoArgs* a, void* stream) {
  if (!valid(a) || !a->ident || !a->mask_sum || !photo_planes_32bit(a)) return FS_EINVAL;
  return launch_ident_rows<TwoFrames>(a, 1, stream);
}

extern "C" int fs_photo_multi_identity(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || !a->ident || !a->mask_sum) return FS_EINVAL;
  return launch_ident_rows<NFrames>(a, (a->nsrc + 1) / 2, stream);
}

extern "C" int fs_photo_identity_strip_rows(void) { return ID_RS; }

extern "C" int fs_photo_pose_grad(const float* geo, const float* dP, float* dT0, float* dT1, int B, int S, int tiles,
                                  void* stream) {
  if (!geo || !dP || !dT0 || !dT1 || B < 1 || S < 1 || tiles < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const PtrTable<float> dT = {{dT0, dT1}};
  hipLaunchKernelGGL(photo_pose_grad_kernel, dim3(B, 2), dim3(256), 0, st, geo, GEO_STRIDE, dP, dT, 2, B, S, tiles);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_pose_grad(const float* geo, const float* dP, float* dT, int nsrc, int B, int S, int tiles,
                                        void* stream) {
  if (!geo || !dP || !dT || nsrc < 1 || nsrc > MAXF || B < 1 || S < 1 || S > 4 || tiles < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  PtrTable<float> t = {};
  for (int f = 0; f < nsrc; ++f) t.p[f] = dT + (long)f * B * 16;
  hipLaunchKernelGGL(photo_pose_grad_kernel, dim3(B, nsrc), dim3(256), 0, st, geo, geo_stride_n(nsrc), dP, t, nsrc, B, S,
                     tiles);
  return fs_launch_status();
}
