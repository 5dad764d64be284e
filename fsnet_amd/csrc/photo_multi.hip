// Photometric loss chain over N = 1..4 temporal source frames (train_cfg.frame_ids = [0, a, ...], pinhole camera): the
// kernels of photo_fused.hip / photometric.hip with a frame count.  frame_ids = [0, a, b] keeps running on those; this
// file is the path of every other count (and takes N = 2 as well, which its tests hold against the two-source path).
// Replaces (reference): MonoDepth2Decoder._generate_images_pred, compute_reprojection_loss and the per-pixel minimum of
// compute_total_reprojection_loss (monodepth2_decoder.py:61-128, 205-292) for any length of frame_ids.
//
// Forward: a wave owns a strip of 62 columns x 16 rows of one (sample, scale) as in photo_fused_fwd_kernel and walks it
// once per frame PAIR — the two frames of a pair ride in the two components of the f2 lanes, so the per-frame arithmetic
// is that kernel's to the instruction.  Between the walks the running minimum and its index of the strip's pixels wait
// in a per-lane LDS slot (5 bytes per pixel, written and read by the same lane: no barrier, no bank conflict); N <= 2
// never touches it.  A half-filled pair (N = 1, 3) points its second component at the pair's first frame, so nothing
// that is not there is read, and leaves it out of the minimum and of pred / ov.
// Backward: photo_bwd_body.h, the body photo_fused_bwd_kernel runs, with the frame index taken modulo N.
// Identity planes: the walk of photo_ident_rows_kernel (photometric.hip), a wave per (sample, strip, frame pair), under
// that file's unfused arithmetic: a frame equal to the target gives exactly 0.
// FS_HIPCC_FLAGS: -fno-slp-vectorize
// (as in photo_fused.hip)
#include <algorithm>
#define FS_PHOTO_CONTRACT_FAST
#include "photo_common.h"
#pragma clang fp contract(fast)
#include "photo_bwd_body.h"

// ---------------------------------------------------------------------------------------------
// setup, identity planes, pose gradient: unfused, as photometric.hip builds them
// ---------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

namespace {

constexpr int MAXF = 4;
struct TPtrs { const float* T[MAXF]; };

__device__ __host__ __forceinline__ int geo_stride_n(int n) { return 18 + 12 * n; }

__global__ void photo_multi_setup_kernel(const float* __restrict__ P2, const TPtrs tp, int nsrc, float* __restrict__ geo,
                                         int B, int* __restrict__ seed_counter) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (seed_counter && b == 0) *seed_counter += 1;      // tie-break noise seed of this step (read by the loss forward)
  if (b >= B) return;
  double k[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i][j] = (double)P2[b * 12 + i * 4 + j];
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
  float* g = geo + (long)b * geo_stride_n(nsrc);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { g[i * 3 + j] = (float)inv[i][j]; g[9 + i * 3 + j] = (float)k[i][j]; }
#pragma unroll
  for (int f = 0; f < MAXF; ++f) {
    if (f >= nsrc) break;
    const float* T = tp.T[f] + (long)b * 16;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {
        float a = 0.f;
        for (int m = 0; m < 3; ++m) a += g[9 + i * 3 + m] * T[m * 4 + j];
        g[18 + f * 12 + i * 4 + j] = a;
      }
  }
}

constexpr int ID_W = 62;              // output columns per wave (lanes 1..62)
constexpr int ID_RS = 16;             // output rows per wave

// (photometric.hip: v_rcp_f32 and one Newton step with the exact fma remainder; exactly 1 for n == d)
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

// photo_ident_rows_kernel with a frame pair per wave: wave = (sample, strip row, strip column, pair)
__global__ __launch_bounds__(256) void photo_multi_ident_kernel(const FsPhotoMultiArgs p, int SX, int SY, int nwaves) {
  const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
  if (wv >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int N = p.nsrc, npair = (N + 1) >> 1;
  const int pr = wv % npair;
  int rest = wv / npair;
  const int sx = rest % SX; rest /= SX;
  const int sy = rest % SY, b = rest / SY;
  const int fa = 2 * pr;
  const bool have2 = fa + 1 < N;
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

  auto step = [&](IdRow& r2, const IdRow& r1, IdRow& r0, const int it) {
    load(r2, min(it + 1, nsteps - 1));               // next row (this step reads r2's sums only); last step: a re-load, unused
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tc = r0.rt[c] - 0.5f;
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
      const float k3 = 1.f / 3.f;
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

// photo_pose_grad_kernel with the frame count: one block per (b, f), dT [N][B][4][4]
__global__ __launch_bounds__(256) void photo_multi_pose_grad_kernel(const float* __restrict__ geo,
                                                                    const float* __restrict__ dP, float* __restrict__ dT,
                                                                    int N, int B, int S, int tiles) {
  constexpr int RL = 85;
  __shared__ double s_part[RL][12];
  __shared__ float s_g[12];
  const int b = (int)blockIdx.x / N, f = (int)blockIdx.x % N;
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
    const float* K = geo + (long)b * geo_stride_n(N) + 9;
    float* o = dT + ((long)f * B + b) * 16;
    const int rr = t >> 2, j = t & 3;
    o[t] = rr < 3 ? K[0 * 3 + rr] * s_g[0 * 4 + j] + K[1 * 3 + rr] * s_g[1 * 4 + j] + K[2 * 3 + rr] * s_g[2 * 4 + j] : 0.f;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// forward and backward: fused multiply-adds allowed, as in photo_fused.hip
// ---------------------------------------------------------------------------------------------
#pragma clang fp contract(fast)

namespace {

constexpr int FW = 62;    // output columns per wave (lanes 1..62; lanes 0 and 63 are halo)
constexpr int FRH = 16;   // output rows per wave

struct Row {       // one image row of a strip: horizontal 3-tap sums + the raw values (needed when it is the centre)
  float t[3], tt[3];
  f2 x[3], xx[3], xt[3];        // component = frame of the pair
  float rt[3];
  f2 rx[3];
  bool ov[2];
};

template <bool WRITE_PRED>
__global__ __launch_bounds__(256) void photo_multi_fwd_kernel(const FsPhotoMultiArgs p, int SX, int SY, int nwaves) {
  // the running minimum of the strip's pixels between two pair walks: slot [row][lane], owned by the lane
  __shared__ float s_best[4][FRH][64];
  __shared__ uint8_t s_bi[4][FRH][64];
  // XCD-contiguous logical block order: consecutive logical blocks (= the scales of one strip row) share an L2
  const int nblk = gridDim.x;
  const int lb = ((int)blockIdx.x & 7) * (nblk >> 3) + ((int)blockIdx.x >> 3);
  const int wid = (int)threadIdx.x >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(lb * 4 + wid);
  if (wv >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int sx = wv % SX;
  int rest = wv / SX;
  const int s = rest % p.S; rest /= p.S;
  const int sy = rest % SY;
  const int b = rest / SY;
  const int N = p.nsrc, npair = (N + 1) >> 1;
  const int H = p.H, W = p.W;
  const unsigned HW = (unsigned)(H * W);
  const int h = p.dh[s], w = p.dw[s];
  const float* ge = p.geo + (long)b * geo_stride_n(N);
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
  const bool no_ovm = p.no_overlap_mask != 0;

  // per-lane invariants of the depth upsample (ATen upsample_bilinear2d, align_corners=True) and of the ray
  const float sh = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
  const float sw = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
  const float fxu = sw * (float)xr;
  const int dx0 = w > 1 ? min((int)fxu, w - 2) : 0;
  const float dlx = w > 1 ? fxu - (float)dx0 : 0.f;
  const float pxf = (float)xr;
  float ra[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ra[i] = ge[3 * i] * pxf;
  double acc = 0.0;

  for (int pr = 0; pr < npair; ++pr) {
    const int fa = 2 * pr;
    const bool have2 = fa + 1 < N;
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
      float D, ray[3];
      {
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
        D = (1.f - dly) * ((1.f - dlx) * d00 + dlx * d01) + dly * ((1.f - dlx) * d10 + dlx * d11);
        const float pyf = (float)yr;
#pragma unroll
        for (int i = 0; i < 3; ++i) ray[i] = (ra[i] + ge[3 * i + 1] * pyf) + ge[3 * i + 2];
      }
      unsigned og[2][2];
      f2 w01[2], w23[2];           // per frame: the sampler weights of the upper / lower tap pair
      unsigned om[2];
      bool inb[2];
      f2 ixu2, iyu2;
      {
        const float cx_ = D * ray[0], cy_ = D * ray[1], cz_ = D * ray[2];
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
        // nearest sample of patched_mask with zeros padding, round half to even
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
      if (p.patched_mask) {
#pragma unroll
        for (int f = 0; f < 2; ++f) mv[f] = (float)p.patched_mask[(long)b * HW + om[f]];
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
        // (co)variances as (9 sum(ab) - sum(a) sum(b)) / 81 (photo_fused_fwd_kernel)
        const float sgy = (9.f * syy - sy_ * sy_) * k81;
        const f2 sxs = (r2.x[c] + r1.x[c]) + r0.x[c], sxx = (r2.xx[c] + r1.xx[c]) + r0.xx[c],
                 sxy = (r2.xt[c] + r1.xt[c]) + r0.xt[c];
        const f2 mux = sxs * k9;
        const f2 sgx = (9.f * sxx - sxs * sxs) * k81, sgxy = (9.f * sxy - sxs * sy_) * k81;
        const f2 n = (2.f * mux * muy + C1) * (2.f * sgxy + C2);
        const f2 d = (mux * mux + muy * muy + C1) * (sgx + sgy + C2);
        const f2 q = n * f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
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
          best = s_best[wid][j][lane]; bi = s_bi[wid][j][lane];
        }
        // reprojection candidates in the reference's cat order; strict <: the first of equal candidates wins.  A winning
        // term whose sample missed the source frame is the constant 100 (:231-235): index 2 N, value only, no gradient
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
          s_best[wid][j][lane] = best; s_bi[wid][j][lane] = (uint8_t)bi;
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

// the frame index of a backward wave, modulo the launch's frame count
struct NFrames {
  static __device__ __forceinline__ int count(const FsPhotoMultiArgs& p) { return p.nsrc; }
  static __device__ __forceinline__ void split(int& rest, int n, int& f) { f = rest % n; rest /= n; }
  static __device__ __forceinline__ int geo_stride(int n) { return geo_stride_n(n); }
};

__global__ __launch_bounds__(256) void photo_multi_bwd_kernel(const FsPhotoMultiArgs p, int SX, int SY, int nwaves) {
  __shared__ float s_dd[4][LDS_R * LDS_C];
  photo_bwd_body<false, NFrames>(p, SX, SY, nwaves, s_dd);
}

bool valid(const FsPhotoMultiArgs* a) {
  if (!a || !a->img0 || !a->geo) return false;
  if (a->nsrc < 1 || a->nsrc > MAXF) return false;
  for (int f = 0; f < a->nsrc; ++f) if (!a->img_src[f]) return false;
  if (a->S < 1 || a->S > 4 || a->B < 1 || a->H < 2 || a->W < 2) return false;
  if ((long)a->H * a->W * 3 >= 0x40000000L) return false;             // 32-bit plane offsets
  return true;
}

}  // namespace

extern "C" int fs_photo_multi_setup(const float* P2, const float* const* T, int nsrc, float* geo, int B,
                                    int* seed_counter, void* stream) {
  if (!P2 || !T || !geo || nsrc < 1 || nsrc > MAXF || B < 1) return FS_EINVAL;
  TPtrs tp = {};
  for (int f = 0; f < nsrc; ++f) {
    if (!T[f]) return FS_EINVAL;
    tp.T[f] = T[f];
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(photo_multi_setup_kernel, dim3((B + 63) / 64), dim3(64), 0, st, P2, tp, nsrc, geo, B, seed_counter);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_identity(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || !a->ident || !a->mask_sum) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + ID_W - 1) / ID_W, SY = (a->H + ID_RS - 1) / ID_RS;
  const long nwaves = (long)a->B * SY * SX * ((a->nsrc + 1) / 2);
  const long nblk = (nwaves + 3) / 4;
  if (nwaves > 0x7ffffff0L) return FS_EINVAL;
  hipLaunchKernelGGL(photo_multi_ident_kernel, dim3((unsigned)nblk), dim3(256), 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_fwd(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || (!a->ident && !a->motion_mask) || !a->sel || !a->loss_sums) return FS_EINVAL;
  if ((a->pred != nullptr) != (a->ov != nullptr)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + FW - 1) / FW, SY = (a->H + FRH - 1) / FRH;
  const long nwaves = (long)a->B * a->S * SY * SX;
  long nblk = (nwaves + 3) / 4;
  nblk = (nblk + 7) / 8 * 8;
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  if (a->pred) hipLaunchKernelGGL(photo_multi_fwd_kernel<true>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  else hipLaunchKernelGGL(photo_multi_fwd_kernel<false>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int64_t fs_photo_multi_bwd_tiles(int H, int W) {
  if (H < 2 || W < 2) return -1;
  return (int64_t)((W + BW - 1) / BW) * ((H + BRH - 1) / BRH);
}

extern "C" int fs_photo_multi_bwd(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || !a->sel || !a->dP || !a->mask_sum) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || !a->d_depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + BW - 1) / BW, SY = (a->H + BRH - 1) / BRH;
  const long nwaves = (long)a->B * a->S * a->nsrc * SY * SX;
  long nblk = (nwaves + 3) / 4;
  nblk = (nblk + 7) / 8 * 8;
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  hipLaunchKernelGGL(photo_multi_bwd_kernel, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_pose_grad(const float* geo, const float* dP, float* dT, int nsrc, int B, int S, int tiles,
                                        void* stream) {
  if (!geo || !dP || !dT || nsrc < 1 || nsrc > MAXF || B < 1 || S < 1 || S > 4 || tiles < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(photo_multi_pose_grad_kernel, dim3(nsrc * B), dim3(256), 0, st, geo, dP, dT, nsrc, B, S, tiles);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_strip(int which, int32_t* cols, int32_t* rows) {
  if (!cols || !rows || which < 0 || which > 2) return FS_EINVAL;
  *cols = which == 0 ? ID_W : (which == 1 ? FW : BW);
  *rows = which == 0 ? ID_RS : (which == 1 ? FRH : BRH);
  return 0;
}
