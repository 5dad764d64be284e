// Edge-aware smoothness loss (fwd + bwd, all scales per launch), the final loss assembly, and the
// fused gradient-norm / clip / Adam, AdamW or SGD update over a flat parameter arena.
// Replaces:
//   get_smooth_loss + mean-normalised disparity        monodepth_utils.py:168-181, monodepth2_decoder.py:294-299
//   F.adaptive_avg_pool2d(original_image_0, (h, w))     monodepth2_decoder.py:214-219
//   loss bookkeeping (loss/s, smooth_loss/s, total)     monodepth2_decoder.py:292-304, 343
//   clip_grad_norm_ + torch.optim.{Adam,AdamW,SGD}.step base_training_hooks.py:46-49, optimizers.py:4-11
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>
#include <vector>

namespace {

// colour pyramid: out_s[b][c][y][x] = mean of the (H/h)x(W/w) block (adaptive_avg_pool2d with integer ratio)
__global__ __launch_bounds__(256) void color_pyramid_kernel(const float* __restrict__ img, float* __restrict__ out,
                                                            int B, int H, int W, int h, int w) {
  const int ry = H / h, rx = W / w;
  const long total = (long)B * 3 * h * w;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int x = (int)(i % w); long q = i / w; int y = (int)(q % h); long bc = q / h;
    const float* src = img + bc * H * W;
    float s = 0.f;
    for (int a = 0; a < ry; ++a)
      for (int c = 0; c < rx; ++c) s += src[(long)(y * ry + a) * W + x * rx + c];
    out[i] = s / (float)(ry * rx);
  }
}

// The three standard levels (ratios 2, 4 and 8) from ONE read of the image: a thread owns one 8x8 cell of one plane, loads
// its eight rows as 16-byte units (neighbouring lanes are 32 bytes apart: the two loads of a row use every fetched
// line in full) and keeps each level's block sums in the order of color_pyramid_kernel — row-major within the level's
// own block, one division at the end — so the outputs are bit-identical to three launches of that kernel, which read
// the image three times with 4-byte loads up to 32 bytes apart.
__global__ __launch_bounds__(64) void color_pyramid3_kernel(const float* __restrict__ img, float* __restrict__ o2,
                                                            float* __restrict__ o4, float* __restrict__ o8,
                                                            long cells, int H, int W) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= cells) return;
  const int cw = W >> 3, ch = H >> 3;
  const int cx = (int)(i % cw);
  const long q = i / cw;
  const int cy = (int)(q % ch);
  const long bc = q / ch;
  const float* src = img + bc * H * W + (long)(cy * 8) * W + cx * 8;
  float4 v[8][2];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    v[a][0] = *reinterpret_cast<const float4*>(src + (long)a * W);
    v[a][1] = *reinterpret_cast<const float4*>(src + (long)a * W + 4);
  }
  float* d2 = o2 + bc * (H >> 1) * (W >> 1) + (long)(cy * 4) * (W >> 1) + cx * 4;
  float* d4 = o4 + bc * (H >> 2) * (W >> 2) + (long)(cy * 2) * (W >> 2) + cx * 2;
  float s2[4], s4[2], s8 = 0.f;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const float e[8] = {v[a][0].x, v[a][0].y, v[a][0].z, v[a][0].w, v[a][1].x, v[a][1].y, v[a][1].z, v[a][1].w};
    if (a % 2 == 0) s2[0] = s2[1] = s2[2] = s2[3] = 0.f;
    if (a % 4 == 0) s4[0] = s4[1] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) { s2[c >> 1] += e[c]; s4[c >> 2] += e[c]; s8 += e[c]; }
    if (a % 2 == 1)
      *reinterpret_cast<float4*>(d2 + (long)(a >> 1) * (W >> 1)) =
          make_float4(s2[0] / 4.f, s2[1] / 4.f, s2[2] / 4.f, s2[3] / 4.f);
    if (a % 4 == 3) *reinterpret_cast<float2*>(d4 + (long)(a >> 2) * (W >> 2)) = make_float2(s4[0] / 16.f, s4[1] / 16.f);
  }
  o8[i] = s8 / 64.f;
}

// per (scale, batch) sum of disp -> sums[s][b]  (mean = sums / (h*w))
__global__ __launch_bounds__(256) void smooth_mean_kernel(const FsSmoothArgs p) {
  const int s = blockIdx.z, b = blockIdx.y;
  const long hw = (long)p.h[s] * p.w[s];
  const float* d = p.disp[s] + (long)b * hw;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) acc += d[i];
  __shared__ double sh[4];
  double tot = block_sum_d((double)acc, sh);
  if (threadIdx.x == 0) atomicAdd(p.disp_sum + s * p.B + b, tot);
}

__device__ __forceinline__ float edge_w(const float* __restrict__ col, long hw, long i0, long i1) {
  float g = fabsf(col[i0] - col[i1]) + fabsf(col[hw + i0] - col[hw + i1]) + fabsf(col[2 * hw + i0] - col[2 * hw + i1]);
  return expf(-g * (1.f / 3.f));
}

// forward: sx[s] = sum |nd(x)-nd(x+1)| e^{-gx},  sy[s] likewise (nd = disp / (mean + 1e-7))
__global__ __launch_bounds__(256) void smooth_fwd_kernel(const FsSmoothArgs p) {
  const int s = blockIdx.z, b = blockIdx.y;
  const int h = p.h[s], w = p.w[s];
  const long hw = (long)h * w;
  const float* d = p.disp[s] + (long)b * hw;
  const float* col = p.color[s] + (long)b * 3 * hw;
  const float inv = 1.f / ((float)(p.disp_sum[s * p.B + b] / (double)hw) + 1e-7f);
  float ax = 0.f, ay = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    int x = (int)(i % w), y = (int)(i / w);
    float v = d[i] * inv;
    if (x + 1 < w) ax += fabsf(v - d[i + 1] * inv) * edge_w(col, hw, i, i + 1);
    if (y + 1 < h) ay += fabsf(v - d[i + w] * inv) * edge_w(col, hw, i, i + w);
  }
  __shared__ double sh[4];
  double tx = block_sum_d((double)ax, sh);
  double ty = block_sum_d((double)ay, sh);
  if (threadIdx.x == 0) {
    atomicAdd(p.sm_sums + (s * p.B + b) * 2, tx);
    atomicAdd(p.sm_sums + (s * p.B + b) * 2 + 1, ty);
  }
}

// d loss / d nd at pixel i (both neighbours on each axis), scaled by the loss weights
__device__ __forceinline__ float smooth_dnd(const float* __restrict__ d, const float* __restrict__ col, long hw, int h,
                                            int w, int y, int x, float inv, float kx, float ky) {
  long i = (long)y * w + x;
  float v = d[i] * inv, g = 0.f;
  auto sgn = [](float a) { return a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f); };
  if (x + 1 < w) g += kx * sgn(v - d[i + 1] * inv) * edge_w(col, hw, i, i + 1);
  if (x > 0) g -= kx * sgn(d[i - 1] * inv - v) * edge_w(col, hw, i - 1, i);
  if (y + 1 < h) g += ky * sgn(v - d[i + w] * inv) * edge_w(col, hw, i, i + w);
  if (y > 0) g -= ky * sgn(d[i - w] * inv - v) * edge_w(col, hw, i - w, i);
  return g;
}

// backward pass 1: dot[s][b] = sum_i dnd(i) * disp(i)   (coupling through the mean normalisation)
__global__ __launch_bounds__(256) void smooth_bwd_dot_kernel(const FsSmoothArgs p) {
  const int s = blockIdx.z, b = blockIdx.y;
  const int h = p.h[s], w = p.w[s];
  const long hw = (long)h * w;
  const float* d = p.disp[s] + (long)b * hw;
  const float* col = p.color[s] + (long)b * 3 * hw;
  const float inv = 1.f / ((float)(p.disp_sum[s * p.B + b] / (double)hw) + 1e-7f);
  const float gout = p.gout ? (float)*p.gout : 1.f;
  const float wgt = gout * 1e-5f / (float)(1 << p.scale_id[s]) / (float)p.S;
  const float kx = wgt / (float)((long)p.B * h * (w - 1)), ky = wgt / (float)((long)p.B * (h - 1) * w);
  float* dd = p.d_disp[s] + (long)b * hw;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
    int x = (int)(i % w), y = (int)(i / w);
    float g = smooth_dnd(d, col, hw, h, w, y, x, inv, kx, ky);
    dd[i] = g;                 // pass 2 only rescales and shifts it (no second walk over the colour edges)
    acc += g * d[i];
  }
  __shared__ double sh[4];
  double tot = block_sum_d((double)acc, sh);
  if (threadIdx.x == 0) atomicAdd(p.dot + s * p.B + b, tot);
}

// backward pass 2: d_disp(i) = dnd(i)*inv - dot * inv^2 / (h*w)
__global__ __launch_bounds__(256) void smooth_bwd_apply_kernel(const FsSmoothArgs p) {
  const int s = blockIdx.z, b = blockIdx.y;
  const int h = p.h[s], w = p.w[s];
  const long hw = (long)h * w;
  float* dd = p.d_disp[s] + (long)b * hw;
  const float inv = 1.f / ((float)(p.disp_sum[s * p.B + b] / (double)hw) + 1e-7f);
  const float corr = (float)p.dot[s * p.B + b] * inv * inv / (float)hw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256)
    dd[i] = dd[i] * inv - corr;        // dd holds dnd from pass 1
}

// loss assembly: out[0..S) = loss/s (f64), out[S..2S) = smooth_loss/s, out[2S] = total.  One wave: lane b sums batch
// element b (b, b + 64, ...), wave sums combine them — the single-thread version walked ~100 dependent loads (9 us on
// the serial path between the loss forward and backward).
__global__ __launch_bounds__(64) void loss_finalize_kernel(const double* __restrict__ loss_sums,
                                                           const double* __restrict__ mask_sum,
                                                           const double* __restrict__ sm_sums, const FsSmoothArgs p,
                                                           double* __restrict__ out, double* __restrict__ total_out) {
  const int lane = threadIdx.x;
  double msum = 0.0;
  for (int b = lane; b < p.B; b += 64) msum += mask_sum[b];
  msum = wave_sum_d(msum);
  double total = 0.0;
  for (int s = 0; s < p.S; ++s) {
    const int h = p.h[s], w = p.w[s];
    double ax = 0.0, ay = 0.0, ls = 0.0;
    for (int b = lane; b < p.B; b += 64) {
      ax += sm_sums[(s * p.B + b) * 2]; ay += sm_sums[(s * p.B + b) * 2 + 1]; ls += loss_sums[s * p.B + b];
    }
    ax = wave_sum_d(ax); ay = wave_sum_d(ay); ls = wave_sum_d(ls);
    float sx = (float)(ax / (double)((long)p.B * h * (w - 1)));
    float sy = (float)(ay / (double)((long)p.B * (h - 1) * w));
    float sm = (sx + sy) * 1e-5f / (float)(1 << p.scale_id[s]);   // fp32 like the reference's smooth_loss
    double l = ls / (msum + 1e-6) + (double)sm;
    if (lane == 0) { out[s] = l; out[p.S + s] = (double)sm; }
    total += l;
  }
  if (lane == 0) {
    out[2 * p.S] = total / (double)p.S;
    if (total_out) *total_out = total / (double)p.S;     // the scalar the caller differentiates: no device copy needed
  }
}

// ---------------------------------------------------------------------------------------------
// optimizer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ out,
                                                     int* __restrict__ step_counter) {
  // the optimizer's device-resident step count is bumped here (nothing in this kernel reads it; the Adam launch that
  // follows does): one serial 5-us node less at the tail of every step
  if (step_counter && blockIdx.x == 0 && threadIdx.x == 0) *step_counter += 1;
  double acc = 0.0;
  long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * 256 * 4;
  for (; i + 3 + stride < n; i += 2 * stride) {          // two 16-byte loads in flight per thread
    float4 v = *reinterpret_cast<const float4*>(g + i), u = *reinterpret_cast<const float4*>(g + i + stride);
    acc += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
    acc += (double)(u.x * u.x + u.y * u.y) + (double)(u.z * u.z + u.w * u.w);
  }
  for (; i + 3 < n; i += stride) {
    float4 v = *reinterpret_cast<const float4*>(g + i);
    acc += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
  }
  if (i < n) for (long k = i; k < n && k < i + 4; ++k) acc += (double)g[k] * g[k];
  // one f64 atomic per BLOCK: they all hit the same address (~12 ns each, serialised) — 8192 per-wave atomics
  // were 98 of this kernel's 114 us
  __shared__ double sh[4];
  acc = block_sum_d(acc, sh);
  if (threadIdx.x == 0) atomicAdd(out, acc);
}

__global__ void counter_incr_kernel(int* p) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += 1; }

// ---- the update kernels: one launch over the arena, or over the runs of it that hold trainable parameters ----
// What the three updates share sits in optim_kernel: the device-resident step count and learning rate (the launch is
// hipGraph-replayable), the fused clip, the walk over the run table in 16-byte units.  An update is a struct with
//   NS                  how many state arrays it streams beside the parameter and the gradient (0, 1 or 2)
//   begin(lr, t)        per-thread scalars; t > 0: the step count read from device memory
//   apply(p, g, a, b)   one element: gradient already scaled and clipped, a / b its state
struct AdamUpdate {          // torch.optim.Adam (decoupled = 0: L2 decay folded into the gradient) / AdamW (= 1)
  static constexpr int NS = 2;
  float b1, b2, eps, wd, bc1, bc2_sqrt;
  int decoupled;
  float step, keep;
  __device__ void begin(float lr, int t) {
    if (t > 0) {
      const float st = (float)t;
      bc1 = 1.f - powf(b1, st);
      bc2_sqrt = sqrtf(1.f - powf(b2, st));
    }
    step = lr / bc1;
    keep = 1.f - lr * wd;
  }
  __device__ void apply(float& p, float gi, float& m, float& v) const {
    float pi = p;
    if (wd != 0.f) {
      if (decoupled) pi *= keep;
      else gi += wd * pi;
    }
    float mi = b1 * m + (1.f - b1) * gi;
    float vi = b2 * v + (1.f - b2) * gi * gi;
    m = mi; v = vi;
    p = pi - step * mi / (sqrtf(vi) / bc2_sqrt + eps);
  }
};

template <int MOMENTUM> struct SgdUpdate {   // torch.optim.SGD; MOMENTUM = 0 streams no buffer at all
  static constexpr int NS = MOMENTUM;
  float momentum, dampening, wd;
  int nesterov, first;
  float lr;
  __device__ void begin(float lr_, int t) {
    lr = lr_;
    if (t > 0) first = t == 1;      // torch's first step stores the gradient as the buffer, undamped
  }
  __device__ void apply(float& p, float gi, float& buf, float&) const {
    const float pi = p;
    if (wd != 0.f) gi += wd * pi;
    if (MOMENTUM) {
      const float bi = first ? gi : momentum * buf + (1.f - dampening) * gi;
      buf = bi;
      gi = nesterov ? gi + momentum * bi : bi;
    }
    p = pi - lr * gi;
  }
};

template <class U> __device__ __forceinline__ void update4(const U& u, float* __restrict__ p,
                                                           const float* __restrict__ g, float* __restrict__ s0,
                                                           float* __restrict__ s1, long i, float coef) {
  float4 pv = *reinterpret_cast<const float4*>(p + i);
  const float4 gv = *reinterpret_cast<const float4*>(g + i);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (U::NS > 0) a = *reinterpret_cast<const float4*>(s0 + i);
  if (U::NS > 1) b = *reinterpret_cast<const float4*>(s1 + i);
  u.apply(pv.x, gv.x * coef, a.x, b.x);
  u.apply(pv.y, gv.y * coef, a.y, b.y);
  u.apply(pv.z, gv.z * coef, a.z, b.z);
  u.apply(pv.w, gv.w * coef, a.w, b.w);
  if (U::NS > 0) *reinterpret_cast<float4*>(s0 + i) = a;
  if (U::NS > 1) *reinterpret_cast<float4*>(s1 + i) = b;
  *reinterpret_cast<float4*>(p + i) = pv;
}

template <class U> __device__ __forceinline__ void update1(const U& u, float* __restrict__ p,
                                                           const float* __restrict__ g, float* __restrict__ s0,
                                                           float* __restrict__ s1, long i, float coef) {
  float pi = p[i], a = 0.f, b = 0.f;
  if (U::NS > 0) a = s0[i];
  if (U::NS > 1) b = s1[i];
  u.apply(pi, g[i] * coef, a, b);
  if (U::NS > 0) s0[i] = a;
  if (U::NS > 1) s1[i] = b;
  p[i] = pi;
}

// runs: n_runs [lo, hi) element ranges (NULL: the one range [0, n)).  Nothing outside a run is read or written.  A run
// is walked in 16-byte units between its first and last 16-byte boundary and element-wise outside them (vec = 0, a
// base pointer off that alignment: element-wise throughout).  Run r starts at block r of the grid, so that a table of
// many short runs spreads over the blocks instead of queueing on the first one.  A run that does not lie inside [0, n)
// is skipped: the entry points reject such a table, but inside a stream capture they cannot read it.
template <class U> __global__ __launch_bounds__(256) void optim_kernel(
    U u, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1, long n,
    const int64_t* __restrict__ runs, int n_runs, int vec, float lr, float max_norm, const double* __restrict__ sumsq,
    float grad_scale, const int* __restrict__ step_ptr, const float* __restrict__ lr_ptr) {
  if (lr_ptr) lr = *lr_ptr;
  u.begin(lr, step_ptr ? *step_ptr : 0);
  float coef = grad_scale;
  if (sumsq && max_norm > 0.f) {
    float norm = (float)sqrt(*sumsq) * grad_scale;
    coef *= fminf(max_norm / (norm + 1e-6f), 1.f);
  }
  const long G = gridDim.x;
  const int R = runs ? n_runs : 1;
  for (int r = 0; r < R; ++r) {
    const long lo = runs ? (long)runs[2 * r] : 0, hi = runs ? (long)runs[2 * r + 1] : n;
    if (lo < 0 || hi > n || hi <= lo) continue;
    long a = hi, b = hi;                 // [lo, a) and [b, hi): element-wise; [a, b): 16-byte units
    if (vec) {
      a = (lo + 3) & ~3L;
      if (a > hi) a = hi;
      b = hi & ~3L;
      if (b < a) b = a;
    }
    const long t = ((blockIdx.x + G - r % G) % G) * 256 + threadIdx.x;
    for (long i = a + t * 4; i < b; i += G * 256 * 4) update4(u, p, g, s0, s1, i, coef);
    for (long i = lo + t; i < a; i += G * 256) update1(u, p, g, s0, s1, i, coef);
    for (long i = b + t; i < hi; i += G * 256) update1(u, p, g, s0, s1, i, coef);
  }
}

}  // namespace

static void launch_pyramid_level(const float* img, float* out, int B, int H, int W, int h, int w, hipStream_t st) {
  long total = (long)B * 3 * h * w;
  hipLaunchKernelGGL(color_pyramid_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, img, out, B, H, W, h, w);
}

extern "C" int fs_color_pyramid(const float* img, float* out, int B, int H, int W, int h, int w, void* stream) {
  if (!img || !out || h <= 0 || w <= 0 || H % h != 0 || W % w != 0) return FS_EINVAL;
  launch_pyramid_level(img, out, B, H, W, h, w, reinterpret_cast<hipStream_t>(stream));
  return fs_launch_status();
}

extern "C" int fs_color_pyramid_multi(const float* img, float* const* outs, const int32_t* hs, const int32_t* ws, int n,
                                      int B, int H, int W, void* stream) {
  if (!img || !outs || !hs || !ws || n < 1 || n > 4 || B < 1 || H < 1 || W < 1) return FS_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!outs[i] || hs[i] <= 0 || ws[i] <= 0 || H % hs[i] != 0 || W % ws[i] != 0) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // the one-read kernel: exactly the ratios 2, 4 and 8 (any order) of an image whose sides are multiples of 8
  float* lv[4] = {nullptr, nullptr, nullptr, nullptr};      // by log2(ratio)
  bool fast = n == 3 && H % 8 == 0 && W % 8 == 0 && ((uintptr_t)img & 15) == 0;
  for (int i = 0; fast && i < n; ++i) {
    const int ry = H / hs[i], rx = W / ws[i];
    const int l = ry == 2 ? 1 : (ry == 4 ? 2 : (ry == 8 ? 3 : 0));
    if (ry != rx || l == 0 || lv[l] || ((uintptr_t)outs[i] & 15) != 0) fast = false;
    else lv[l] = outs[i];
  }
  if (fast) {
    const long cells = (long)B * 3 * (H / 8) * (W / 8);
    if ((cells + 63) / 64 > 0x7fffffffL) return FS_EINVAL;
    hipLaunchKernelGGL(color_pyramid3_kernel, dim3((unsigned)((cells + 63) / 64)), dim3(64), 0, st, img, lv[1], lv[2],
                       lv[3], cells, H, W);
  } else {
    for (int i = 0; i < n; ++i) launch_pyramid_level(img, outs[i], B, H, W, hs[i], ws[i], st);
  }
  return fs_launch_status();
}

static bool smooth_valid(const FsSmoothArgs* a) {
  if (!a || a->S < 1 || a->S > 4 || a->B < 1 || !a->disp_sum) return false;
  for (int s = 0; s < a->S; ++s) if (!a->disp[s] || !a->color[s] || a->h[s] < 2 || a->w[s] < 2) return false;
  return true;
}
static dim3 smooth_grid(const FsSmoothArgs* a) {
  long hw = (long)a->h[0] * a->w[0];
  for (int s = 1; s < a->S; ++s) hw = std::max<long>(hw, (long)a->h[s] * a->w[s]);
  return dim3((unsigned)std::min<long>((hw + 255) / 256, 32), a->B, a->S);
}

extern "C" int fs_smooth_mean(const FsSmoothArgs* a, void* stream) {
  if (!smooth_valid(a)) return FS_EINVAL;
  hipLaunchKernelGGL(smooth_mean_kernel, smooth_grid(a), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a);
  return fs_launch_status();
}
extern "C" int fs_smooth_fwd(const FsSmoothArgs* a, void* stream) {
  if (!smooth_valid(a) || !a->sm_sums) return FS_EINVAL;
  hipLaunchKernelGGL(smooth_fwd_kernel, smooth_grid(a), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a);
  return fs_launch_status();
}
extern "C" int fs_smooth_bwd(const FsSmoothArgs* a, void* stream) {
  if (!smooth_valid(a) || !a->dot) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->d_disp[s]) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(smooth_bwd_dot_kernel, smooth_grid(a), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(smooth_bwd_apply_kernel, smooth_grid(a), dim3(256), 0, st, *a);
  return fs_launch_status();
}
extern "C" int fs_loss_finalize(const double* loss_sums, const double* mask_sum, const double* sm_sums,
                                const FsSmoothArgs* a, double* out, double* total_out, void* stream) {
  if (!loss_sums || !mask_sum || !sm_sums || !a || !out) return FS_EINVAL;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), loss_sums, mask_sum, sm_sums, *a, out,
                     total_out);
  return fs_launch_status();
}

extern "C" int fs_sumsq(const float* g, int64_t n, double* out, int* step_counter, void* stream) {
  if (!g || !out || n <= 0) return FS_EINVAL;
  // (one same-address f64 atomic per block at the end: 512 blocks keep that tail at ~6 us)
  long blocks = std::min<long>((n / 4 + 255) / 256 + 1, 512);
  hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, (long)n, out, step_counter);
  return fs_launch_status();
}

extern "C" int fs_counter_incr(int* counter, void* stream) {
  if (!counter) return FS_EINVAL;
  hipLaunchKernelGGL(counter_incr_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), counter);
  return fs_launch_status();
}

// Reads a run table back to check it (blocking: the table is a few dozen bytes and the caller's stream is idle or about
// to be); a stream that is being captured cannot be waited on, there the kernel's own range check stands alone.
static bool runs_valid(const int64_t* runs, int n_runs, int64_t n, hipStream_t st) {
  if (!runs) return n_runs == 0;
  if (n_runs < 1 || n_runs > FS_MAX_RUNS) return false;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) return false;
  if (cap != hipStreamCaptureStatusNone) return true;
  std::vector<int64_t> host(2 * (size_t)n_runs);
  if (hipMemcpyAsync(host.data(), runs, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return false;
  for (int r = 0; r < n_runs; ++r)
    if (host[2 * r] < 0 || host[2 * r + 1] < host[2 * r] || host[2 * r + 1] > n) return false;
  return true;
}

template <class U> static int launch_optim(const U& u, float* p, const float* g, float* s0, float* s1, int64_t n,
                                           float lr, float max_norm, const double* sumsq, float grad_scale,
                                           const int* step_ptr, const float* lr_ptr, const int64_t* runs, int n_runs,
                                           hipStream_t st) {
  if (!runs_valid(runs, n_runs, n, st)) return FS_EINVAL;
  const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0;
  long blocks = std::min<long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(optim_kernel<U>, dim3((unsigned)blocks), dim3(256), 0, st, u, p, g, s0, s1, (long)n, runs, n_runs,
                     vec, lr, max_norm, sumsq, grad_scale, step_ptr, lr_ptr);
  return fs_launch_status();
}

extern "C" int fs_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int decoupled, int step, float max_norm,
                             const double* sumsq, float grad_scale, const int* step_ptr, const float* lr_ptr,
                             const int64_t* runs, int n_runs, void* stream) {
  if (!p || !g || !m || !v || n <= 0 || (step < 1 && !step_ptr)) return FS_EINVAL;
  if (step < 1) step = 1;
  AdamUpdate u;
  u.b1 = beta1; u.b2 = beta2; u.eps = eps; u.wd = weight_decay; u.decoupled = decoupled != 0;
  u.bc1 = 1.f - (float)pow((double)beta1, (double)step);
  u.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  return launch_optim(u, p, g, m, v, n, lr, max_norm, sumsq, grad_scale, step_ptr, lr_ptr, runs, n_runs,
                      reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fs_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int step, float max_norm, const double* sumsq,
                            float grad_scale, const int* step_ptr, const float* lr_ptr, void* stream) {
  return fs_adamw_step(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, 0, step, max_norm, sumsq, grad_scale,
                       step_ptr, lr_ptr, nullptr, 0, stream);
}

extern "C" int fs_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float dampening,
                           int nesterov, float weight_decay, int step, float max_norm, const double* sumsq,
                           float grad_scale, const int* step_ptr, const float* lr_ptr, const int64_t* runs, int n_runs,
                           void* stream) {
  if (!p || !g || n <= 0 || (momentum != 0.f && !buf) || (step < 1 && !step_ptr)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (momentum == 0.f) {
    SgdUpdate<0> u;
    u.momentum = 0.f; u.dampening = dampening; u.wd = weight_decay; u.nesterov = 0; u.first = 0;
    return launch_optim(u, p, g, nullptr, nullptr, n, lr, max_norm, sumsq, grad_scale, step_ptr, lr_ptr, runs, n_runs, st);
  }
  SgdUpdate<1> u;
  u.momentum = momentum; u.dampening = dampening; u.wd = weight_decay; u.nesterov = nesterov != 0; u.first = step <= 1;
  return launch_optim(u, p, g, buf, nullptr, n, lr, max_norm, sumsq, grad_scale, step_ptr, lr_ptr, runs, n_runs, st);
}
