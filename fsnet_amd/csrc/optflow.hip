// Dense optical flow and epipolar motion masks on the device (the masks then travel through the training input
// pipeline as ground-truth images: masks_kernel, augment.hip).  The precompute half of the reference's motion-mask
// option:
//   MotionMaskPrecomputeHook / MotionMaskARFlowPrecomputeHook (monodepth/pipeline_hooks/precomputing_hooks/
//   base_precompute_hooks.py:27-148): cv2.cvtColor(BGR2GRAY) + cv2.calcOpticalFlowFarneback, then the per-pixel
//   distance to the epipolar line of F = K^-T [T]x R K^-1 against a threshold.
//
// Farneback (OpenCV 4.x optflowgf.cpp as restated in tests/helpers_optflow.py; parity with cv2 itself is unpinned,
// DESIGN.md "Motion masks").  One call = a fixed launch sequence, no host round trip, so it can be captured:
//   of_gray                              uint8 RGB pair -> fp32 gray (cv2 BGR2GRAY fixed point, channel 0 as blue)
//   per pyramid level k = L .. 0
//     of_blur_h                          full-resolution gray -> horizontal Gaussian (ksize_k, sigma_k), REFLECT_101
//     of_blur_v_resize                   vertical Gaussian evaluated at the four taps of the INTER_LINEAR resize
//     of_polyexp                         polynomial expansion R (5 planes per frame) through an LDS row tile
//     of_upsample / memset               the coarser level's flow resized and times 1/pyr_scale (zero at the top)
//     per iteration: of_update_matrices  M (5 planes) from R0, R1 and the current flow
//                    of_window_solve     box / Gaussian window sum over an LDS row tile, 2x2 solve -> next flow
// The blur and window weights and the polynomial-expansion constants are computed on the host and passed by value.
// No atomics, every sum in a fixed order: the result is bit-identical from run to run and across batchings.
#include "common.h"
#include "fsnet_hip_internal.h"
#include <cmath>

namespace {

constexpr int MAX_LEVELS = 16;
constexpr int MAX_BLUR_R = 127;        // Gaussian radius of the pyramid blur (ksize <= 255)
constexpr int MAX_POLY_N = 7;
constexpr int MAX_WIN_M = 64;          // winsize <= 129
constexpr int TILE = 128;              // output columns per block in the row-tile kernels (256 threads)
constexpr int MIN_SIZE = 32;           // optflowgf.cpp min_size
constexpr int FLAG_GAUSSIAN = 256;     // OPTFLOW_FARNEBACK_GAUSSIAN
constexpr int BORDER = 5;

struct BlurW { float k[MAX_BLUR_R + 1]; int r; };
struct PolyW { float g[MAX_POLY_N + 1], xg[MAX_POLY_N + 1], xxg[MAX_POLY_N + 1]; double ig11, ig03, ig33, ig55; int n; };
struct WinW { float k[MAX_WIN_M + 1]; double scale; int m; int gaussian; };

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// cv2.cvtColor(COLOR_BGR2GRAY) of uint8: (B*1868 + G*9617 + R*4899 + 2^13) >> 14 with channel 0 taken as B
__global__ __launch_bounds__(256) void of_gray(const uint8_t* img0, const uint8_t* img1, float* gray, long HW) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int b = blockIdx.y >> 1, f = blockIdx.y & 1;
  const uint8_t* p = (f ? img1 : img0) + ((long)b * HW + i) * 3;
  const int v = ((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14;
  gray[(long)blockIdx.y * HW + i] = (float)v;
}

// horizontal pass of the separable blur: k0 * s[x] + sum_i k_i * (s[x-i] + s[x+i]), fp32, i ascending
__global__ __launch_bounds__(256) void of_blur_h(const float* src, float* dst, int H, int W, BlurW w) {
  const long HW = (long)H * W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const float* row = src + (long)blockIdx.y * HW + (long)y * W;
  float s = row[x] * w.k[0];
  for (int t = 1; t <= w.r; ++t) s += w.k[t] * (row[reflect101(x - t, W)] + row[reflect101(x + t, W)]);
  dst[(long)blockIdx.y * HW + i] = s;
}

// cv2.resize INTER_LINEAR source coordinate (the float path of augment.hip resize_coord)
__device__ __forceinline__ void lin_coord(int d, double scale, int n, int& s0, float& f) {
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= n - 1) { fx = 0.f; sx = n - 1; }
  s0 = sx; f = fx;
}

__device__ __forceinline__ float blur_v_at(const float* img, int H, int W, int y, int x, const BlurW& w) {
  float s = img[(long)y * W + x] * w.k[0];
  for (int t = 1; t <= w.r; ++t)
    s += w.k[t] * (img[(long)reflect101(y - t, H) * W + x] + img[(long)reflect101(y + t, H) * W + x]);
  return s;
}

// vertical pass of the blur at the four source taps of each level pixel, then the bilinear resize (horizontal, then
// vertical weights, as cv2.resize)
__global__ __launch_bounds__(256) void of_blur_v_resize(const float* tmp, float* out, int H, int W, int h, int w,
                                                         BlurW bw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * w) return;
  const int y = (int)(i / w), x = (int)(i - (long)y * w);
  const float* img = tmp + (long)blockIdx.y * H * W;
  int x0, y0; float fx, fy;
  lin_coord(x, 1.0 / ((double)w / (double)W), W, x0, fx);
  lin_coord(y, 1.0 / ((double)h / (double)H), H, y0, fy);
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const float v00 = blur_v_at(img, H, W, y0, x0, bw), v01 = blur_v_at(img, H, W, y0, x1, bw);
  const float v10 = blur_v_at(img, H, W, y1, x0, bw), v11 = blur_v_at(img, H, W, y1, x1, bw);
  const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
  out[(long)blockIdx.y * h * w + i] = top * (1.f - fy) + bot * fy;
}

// FarnebackPolyExp: vertical pass (rows clamped) into an LDS row of TILE + 2n columns (columns clamped = replicated),
// horizontal pass in f64.  R planes: 0 r_y, 1 r_x, 2 r_yy, 3 r_xx, 4 r_xy.  grid (tiles, h, 2B)
__global__ __launch_bounds__(256) void of_polyexp(const float* img, float* R, int h, int w, PolyW p) {
  __shared__ float row[3][TILE + 2 * MAX_POLY_N];
  const int n = p.n, y = blockIdx.y, x0 = blockIdx.x * TILE, t = threadIdx.x;
  const long hw = (long)h * w;
  const float* src = img + (long)blockIdx.z * hw;
  if (t < TILE + 2 * n) {
    const int x = min(max(x0 - n + t, 0), w - 1);
    float r0 = src[(long)y * w + x] * p.g[0], r1 = 0.f, r2 = 0.f;
    for (int k = 1; k <= n; ++k) {
      const float s0 = src[(long)max(y - k, 0) * w + x], s1 = src[(long)min(y + k, h - 1) * w + x];
      const float q = s0 + s1;
      r0 = r0 + p.g[k] * q;
      r1 = r1 + p.xg[k] * (s1 - s0);
      r2 = r2 + p.xxg[k] * q;
    }
    row[0][t] = r0; row[1][t] = r1; row[2][t] = r2;
  }
  __syncthreads();
  const int x = x0 + t;
  if (t >= TILE || x >= w) return;
  const int c = t + n;
  double b1 = (double)(row[0][c] * p.g[0]), b2 = 0, b3 = (double)(row[1][c] * p.g[0]), b4 = 0;
  double b5 = (double)(row[2][c] * p.g[0]), b6 = 0;
  for (int k = 1; k <= n; ++k) {
    const double tg = (double)(row[0][c + k] + row[0][c - k]);
    b1 += tg * (double)p.g[k];
    b4 += tg * (double)p.xxg[k];
    b2 += (double)(row[0][c + k] - row[0][c - k]) * (double)p.xg[k];
    b3 += (double)(row[1][c + k] + row[1][c - k]) * (double)p.g[k];
    b6 += (double)(row[1][c + k] - row[1][c - k]) * (double)p.xg[k];
    b5 += (double)(row[2][c + k] + row[2][c - k]) * (double)p.g[k];
  }
  float* o = R + (long)blockIdx.z * 5 * hw + (long)y * w + x;
  o[0] = (float)(b3 * p.ig11);
  o[hw] = (float)(b2 * p.ig11);
  o[2 * hw] = (float)(b1 * p.ig03 + b5 * p.ig33);
  o[3 * hw] = (float)(b1 * p.ig03 + b4 * p.ig33);
  o[4 * hw] = (float)(b6 * p.ig55);
}

// coarser level's flow -> this level: cv2.resize INTER_LINEAR of the 2-channel field, times (float)(1 / pyr_scale)
__global__ __launch_bounds__(256) void of_upsample(const float* src, float* dst, int hs, int ws, int h, int w,
                                                    float mul) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * w) return;
  const int y = (int)(i / w), x = (int)(i - (long)y * w);
  int x0, y0; float fx, fy;
  lin_coord(x, 1.0 / ((double)w / (double)ws), ws, x0, fx);
  lin_coord(y, 1.0 / ((double)h / (double)hs), hs, y0, fy);
  const int x1 = min(x0 + 1, ws - 1), y1 = min(y0 + 1, hs - 1);
  const float* s = src + (long)blockIdx.y * hs * ws * 2;
  float* d = dst + ((long)blockIdx.y * h * w + i) * 2;
  for (int c = 0; c < 2; ++c) {
    const float v00 = s[((long)y0 * ws + x0) * 2 + c], v01 = s[((long)y0 * ws + x1) * 2 + c];
    const float v10 = s[((long)y1 * ws + x0) * 2 + c], v11 = s[((long)y1 * ws + x1) * 2 + c];
    const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
    d[c] = (top * (1.f - fy) + bot * fy) * mul;
  }
}

// FarnebackUpdateMatrices over the whole level.  grid (pixels, B)
__global__ __launch_bounds__(256) void of_update_matrices(const float* R, const float* flow, float* M, int h, int w) {
  const long hw = (long)h * w;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int b = blockIdx.y;
  const int y = (int)(i / w), x = (int)(i - (long)y * w);
  const float* R0 = R + (long)(2 * b) * 5 * hw;
  const float* R1 = R + (long)(2 * b + 1) * 5 * hw;
  const float dx = flow[((long)b * hw + i) * 2], dy = flow[((long)b * hw + i) * 2 + 1];
  float fx = (float)x + dx, fy = (float)y + dy;
  const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
  fx -= (float)x1; fy -= (float)y1;
  float r2, r3, r4, r5, r6;
  if ((unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1)) {
    const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
    const long o = (long)y1 * w + x1;
    float r[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const float* P = R1 + c * hw + o;
      r[c] = a00 * P[0] + a01 * P[1] + a10 * P[w] + a11 * P[w + 1];
    }
    r2 = r[0]; r3 = r[1];
    r4 = (R0[2 * hw + i] + r[2]) * 0.5f;
    r5 = (R0[3 * hw + i] + r[3]) * 0.5f;
    r6 = (R0[4 * hw + i] + r[4]) * 0.25f;
  } else {
    r2 = r3 = 0.f;
    r4 = R0[2 * hw + i];
    r5 = R0[3 * hw + i];
    r6 = R0[4 * hw + i] * 0.5f;
  }
  r2 = (R0[i] - r2) * 0.5f;
  r3 = (R0[hw + i] - r3) * 0.5f;
  r2 += r4 * dy + r6 * dx;
  r3 += r6 * dy + r5 * dx;
  if ((unsigned)(x - BORDER) >= (unsigned)(w - BORDER * 2) || (unsigned)(y - BORDER) >= (unsigned)(h - BORDER * 2)) {
    const float bt[BORDER] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    const float s = (x < BORDER ? bt[x] : 1.f) * (x >= w - BORDER ? bt[w - x - 1] : 1.f) *
                    (y < BORDER ? bt[y] : 1.f) * (y >= h - BORDER ? bt[h - y - 1] : 1.f);
    r2 *= s; r3 *= s; r4 *= s; r5 *= s; r6 *= s;
  }
  float* m = M + (long)b * 5 * hw + i;
  m[0] = r4 * r4 + r6 * r6;
  m[hw] = (r4 + r5) * r6;
  m[2 * hw] = r5 * r5 + r6 * r6;
  m[3 * hw] = r4 * r2 + r6 * r3;
  m[4 * hw] = r6 * r2 + r5 * r3;
}

// FarnebackUpdateFlow_Blur / _GaussianBlur without the matrix update: the window sum of M (rows clamped, columns
// replicated) over an LDS row tile, then the 2x2 solve in f64.  Box: f64 sums (rows -m..m, then columns -m..m) times
// 1 / winsize^2.  Gaussian: fp32 k0 * c + sum_i k_i * (lo_i + hi_i) vertically, then horizontally.  grid (tiles, h, B)
__global__ __launch_bounds__(256) void of_window_solve(const float* M, float* flow, int h, int w, WinW k) {
  __shared__ double vs[5][TILE + 2 * MAX_WIN_M];
  const int m = k.m, y = blockIdx.y, x0 = blockIdx.x * TILE, t = threadIdx.x;
  const long hw = (long)h * w;
  const float* src = M + (long)blockIdx.z * 5 * hw;
  if (t < TILE + 2 * m) {
    const int x = min(max(x0 - m + t, 0), w - 1);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const float* p = src + c * hw + x;
      if (k.gaussian) {
        float s = p[(long)y * w] * k.k[0];
        for (int j = 1; j <= m; ++j) s += (p[(long)min(y + j, h - 1) * w] + p[(long)max(y - j, 0) * w]) * k.k[j];
        vs[c][t] = (double)s;
      } else {
        double s = 0.0;
        for (int j = -m; j <= m; ++j) s += (double)p[(long)min(max(y + j, 0), h - 1) * w];
        vs[c][t] = s;
      }
    }
  }
  __syncthreads();
  const int x = x0 + t;
  if (t >= TILE || x >= w) return;
  const int cc = t + m;
  double g[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    if (k.gaussian) {
      float s = (float)vs[c][cc] * k.k[0];
      for (int j = 1; j <= m; ++j) s += k.k[j] * ((float)vs[c][cc - j] + (float)vs[c][cc + j]);
      g[c] = (double)s;
    } else {
      double s = 0.0;
      for (int j = -m; j <= m; ++j) s += vs[c][cc + j];
      g[c] = s * k.scale;
    }
  }
  const double idet = 1.0 / (g[0] * g[2] - g[1] * g[1] + 1e-3);
  float* f = flow + ((long)blockIdx.z * hw + (long)y * w + x) * 2;
  f[0] = (float)((g[0] * g[4] - g[1] * g[3]) * idet);
  f[1] = (float)((g[2] * g[3] - g[1] * g[4]) * idet);
}

// -- motion mask -------------------------------------------------------------------------------------------------
// F = K^-T [T]x R K^-1 in f64 from P2[:3,:3] and the 4x4 pose (numpy's left-to-right products), rounded to fp32;
// per pixel in fp32 as base_precompute_hooks.py:58-80: l = F [x y 1], d = [x+u, y+v, 1] . (l / |l_0:2|).
// mode 0: |d| > thr; mode 1: |d| / |flow| > thr (0/0 = NaN: not masked, d/0 = inf: masked).  grid (pixels, B)
__global__ __launch_bounds__(256) void of_motion_mask(const FsMotionMaskArgs a) {
  __shared__ float Fs[9];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    const double* P = a.P2 + b * 12;
    const double* T = a.pose + b * 16;
    const double k00 = P[0], k01 = P[1], k02 = P[2], k10 = P[4], k11 = P[5], k12 = P[6], k20 = P[8], k21 = P[9],
                 k22 = P[10];
    const double c00 = k11 * k22 - k12 * k21, c01 = k12 * k20 - k10 * k22, c02 = k10 * k21 - k11 * k20;
    const double det = k00 * c00 + k01 * c01 + k02 * c02;
    double Ki[3][3];
    Ki[0][0] = c00 / det; Ki[0][1] = (k02 * k21 - k01 * k22) / det; Ki[0][2] = (k01 * k12 - k02 * k11) / det;
    Ki[1][0] = c01 / det; Ki[1][1] = (k00 * k22 - k02 * k20) / det; Ki[1][2] = (k02 * k10 - k00 * k12) / det;
    Ki[2][0] = c02 / det; Ki[2][1] = (k01 * k20 - k00 * k21) / det; Ki[2][2] = (k00 * k11 - k01 * k10) / det;
    const double tx = T[3], ty = T[7], tz = T[11];
    const double X[3][3] = {{0.0, -tz, ty}, {tz, 0.0, -tx}, {-ty, tx, 0.0}};
    double A[3][3], Bm[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A[r][c] = Ki[0][r] * X[0][c] + Ki[1][r] * X[1][c] + Ki[2][r] * X[2][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Bm[r][c] = A[r][0] * T[c] + A[r][1] * T[4 + c] + A[r][2] * T[8 + c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Fs[r * 3 + c] = (float)(Bm[r][0] * Ki[0][c] + Bm[r][1] * Ki[1][c] + Bm[r][2] * Ki[2][c]);
  }
  __syncthreads();
  const long HW = (long)a.H * a.W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
  const float xf = (float)x, yf = (float)y;
  const float u = a.flow[((long)b * HW + i) * 2], v = a.flow[((long)b * HW + i) * 2 + 1];
  const float l0 = Fs[0] * xf + Fs[1] * yf + Fs[2];
  const float l1 = Fs[3] * xf + Fs[4] * yf + Fs[5];
  const float l2 = Fs[6] * xf + Fs[7] * yf + Fs[8];
  const float den = sqrtf(l0 * l0 + l1 * l1);
  const float d = (xf + u) * (l0 / den) + (yf + v) * (l1 / den) + 1.f * (l2 / den);
  float q = fabsf(d);
  if (a.mode == 1) q = q / sqrtf(u * u + v * v);
  a.mask[(long)b * HW + i] = q > a.threshold ? 1 : 0;
}

// -- host side ------------------------------------------------------------------------------------------------------
struct Plan {
  int L;                                     // coarsest level index (levels actually used)
  int w[MAX_LEVELS], h[MAX_LEVELS];
  double sigma[MAX_LEVELS];
  int ksize[MAX_LEVELS];
  long off_gray, off_tmp, off_img, off_R, off_M, off_f0, off_f1;
  int64_t bytes;
};

long align256(long v) { return (v + 255) & ~255L; }

int make_plan(const FsFlowArgs* a, Plan& p) {
  if (!a || a->B < 1 || a->H < 2 || a->W < 2) return FS_EINVAL;
  if ((long)a->H * a->W >= (1L << 30)) return FS_EINVAL;
  if (!(a->pyr_scale > 0.0 && a->pyr_scale < 1.0)) return FS_EINVAL;
  if (a->levels < 0 || a->levels >= MAX_LEVELS) return FS_EINVAL;
  if (a->winsize < 1 || a->winsize / 2 > MAX_WIN_M) return FS_EINVAL;
  if (a->iterations < 1) return FS_EINVAL;
  if (a->poly_n != 5 && a->poly_n != 7) return FS_EINVAL;
  if (a->flags != 0 && a->flags != FLAG_GAUSSIAN) return FS_EINVAL;
  if (!(a->poly_sigma >= 0.0) || !std::isfinite(a->poly_sigma)) return FS_EINVAL;
  int k;
  double scale = 1.0;
  for (k = 0; k < a->levels; ++k) {
    scale *= a->pyr_scale;
    if (a->W * scale < MIN_SIZE || a->H * scale < MIN_SIZE) break;
  }
  p.L = k;
  for (k = 0; k <= p.L; ++k) {
    double s = 1.0;
    for (int i = 0; i < k; ++i) s *= a->pyr_scale;
    p.sigma[k] = (1.0 / s - 1.0) * 0.5;
    p.ksize[k] = std::max((int)std::lrint(p.sigma[k] * 5) | 1, 3);
    if (p.ksize[k] / 2 > MAX_BLUR_R) return FS_EINVAL;
    p.w[k] = (int)std::lrint(a->W * s);
    p.h[k] = (int)std::lrint(a->H * s);
    if (p.w[k] < 1 || p.h[k] < 1) return FS_EINVAL;
  }
  const long HW = (long)a->H * a->W, B = a->B;
  long o = 0;
  p.off_gray = o; o = align256(o + 2 * B * HW * 4);
  p.off_tmp = o;  o = align256(o + 2 * B * HW * 4);
  p.off_img = o;  o = align256(o + 2 * B * HW * 4);
  p.off_R = o;    o = align256(o + 10 * B * HW * 4);
  p.off_M = o;    o = align256(o + 5 * B * HW * 4);
  p.off_f0 = o;   o = align256(o + 2 * B * HW * 4);
  p.off_f1 = o;   o = align256(o + 2 * B * HW * 4);
  p.bytes = o;
  return FS_OK;
}

// cv::getGaussianKernel(ksize, sigma, CV_32F): the fixed 3-tap table for sigma <= 0, else exp in f64 rounded to fp32,
// normalised by the f64 sum of those fp32 values
void blur_weights(int ksize, double sigma, BlurW& w) {
  float cf[2 * MAX_BLUR_R + 1];
  const double sx = sigma > 0 ? sigma : ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
  const double s2 = -0.5 / (sx * sx);
  double sum = 0;
  for (int i = 0; i < ksize; ++i) {
    const double x = i - (ksize - 1) * 0.5;
    const double t = (sigma <= 0 && ksize == 3) ? (i == 1 ? 0.5 : 0.25) : std::exp(s2 * x * x);
    cf[i] = (float)t;
    sum += cf[i];
  }
  sum = 1.0 / sum;
  w.r = ksize / 2;
  for (int i = 0; i <= w.r; ++i) w.k[i] = (float)(cf[w.r + i] * sum);
}

// FarnebackPrepareGaussian with the 6x6 moment matrix in f64 and its inverse in closed form (the (0,3,4) block)
void poly_weights(int n, double sigma, PolyW& p) {
  if (sigma < 1.1920928955078125e-07) sigma = n * 0.3;
  float g[2 * MAX_POLY_N + 1];
  double s = 0.0;
  for (int x = -n; x <= n; ++x) {
    g[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma));
    s += g[x + n];
  }
  s = 1.0 / s;
  for (int x = -n; x <= n; ++x) g[x + n] = (float)(g[x + n] * s);
  double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
  for (int y = -n; y <= n; ++y)
    for (int x = -n; x <= n; ++x) {
      const double gg = (double)g[y + n] * (double)g[x + n];
      G00 += gg;
      G11 += gg * x * x;
      G33 += gg * x * x * x * x;
      G55 += gg * x * x * y * y;
    }
  const double a = G00, b = G11, c = G33, d = G55;
  const double D = a * (c + d) - 2 * b * b;
  p.ig11 = 1.0 / b;
  p.ig03 = -b / D;
  p.ig33 = (a * c - b * b) / ((c - d) * D);
  p.ig55 = 1.0 / d;
  p.n = n;
  for (int x = 0; x <= n; ++x) {
    p.g[x] = g[x + n];
    p.xg[x] = (float)x * g[x + n];
    p.xxg[x] = (float)(x * x) * g[x + n];
  }
}

// FarnebackUpdateFlow_Blur's 1 / winsize^2, or FarnebackUpdateFlow_GaussianBlur's kernel (sigma = 0.3 m)
void window_weights(int winsize, int flags, WinW& k) {
  k.m = winsize / 2;
  k.gaussian = flags == FLAG_GAUSSIAN;
  k.scale = 1.0 / ((double)winsize * winsize);
  const double sigma = k.m * 0.3;
  double s = 1.0;
  k.k[0] = 1.f;
  for (int i = 1; i <= k.m; ++i) {
    const float t = (float)std::exp(-i * i / (2 * sigma * sigma));
    k.k[i] = t;
    s += t * 2;
  }
  s = 1.0 / s;
  for (int i = 0; i <= k.m; ++i) k.k[i] = (float)(k.k[i] * s);
}

unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int64_t fs_optflow_workspace_bytes(const FsFlowArgs* a) {
  Plan p;
  if (make_plan(a, p) != FS_OK) return -1;
  return p.bytes;
}

extern "C" int fs_optflow_farneback(const FsFlowArgs* a, void* stream) {
  Plan p;
  if (make_plan(a, p) != FS_OK) return FS_EINVAL;
  if (!a->img0 || !a->img1 || !a->flow || !a->workspace || a->workspace_bytes < p.bytes) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(a->workspace);
  float* gray = reinterpret_cast<float*>(ws + p.off_gray);
  float* tmp = reinterpret_cast<float*>(ws + p.off_tmp);
  float* img = reinterpret_cast<float*>(ws + p.off_img);
  float* R = reinterpret_cast<float*>(ws + p.off_R);
  float* M = reinterpret_cast<float*>(ws + p.off_M);
  float* fbuf[2] = {reinterpret_cast<float*>(ws + p.off_f0), reinterpret_cast<float*>(ws + p.off_f1)};
  const int B = a->B, H = a->H, W = a->W;
  const long HW = (long)H * W;
  PolyW pw;
  poly_weights(a->poly_n, a->poly_sigma, pw);
  WinW ww;
  window_weights(a->winsize, a->flags, ww);
  hipLaunchKernelGGL(of_gray, dim3(nblk(HW), 2 * B), dim3(256), 0, st, a->img0, a->img1, gray, HW);
  int cur = 0;
  const float* prev = nullptr;
  int ph = 0, pwid = 0;
  for (int k = p.L; k >= 0; --k) {
    const int h = p.h[k], w = p.w[k];
    const long hw = (long)h * w;
    BlurW bw;
    blur_weights(p.ksize[k], k == 0 ? 0.0 : p.sigma[k], bw);
    hipLaunchKernelGGL(of_blur_h, dim3(nblk(HW), 2 * B), dim3(256), 0, st, gray, tmp, H, W, bw);
    hipLaunchKernelGGL(of_blur_v_resize, dim3(nblk(hw), 2 * B), dim3(256), 0, st, tmp, img, H, W, h, w, bw);
    hipLaunchKernelGGL(of_polyexp, dim3((w + TILE - 1) / TILE, h, 2 * B), dim3(256), 0, st, img, R, h, w, pw);
    float* f;
    if (prev) {                                      // prev is fbuf[cur]: the resized flow goes to the other buffer
      f = fbuf[cur ^ 1];
      hipLaunchKernelGGL(of_upsample, dim3(nblk(hw), B), dim3(256), 0, st, prev, f, ph, pwid, h, w,
                         (float)(1.0 / a->pyr_scale));
      cur ^= 1;
    } else {
      f = fbuf[cur];
      if (hipMemsetAsync(f, 0, (size_t)B * hw * 2 * sizeof(float), st) != hipSuccess) return FS_ELAUNCH;
    }
    for (int it = 0; it < a->iterations; ++it) {
      hipLaunchKernelGGL(of_update_matrices, dim3(nblk(hw), B), dim3(256), 0, st, R, f, M, h, w);
      float* nf = (k == 0 && it == a->iterations - 1) ? a->flow : fbuf[cur ^ 1];
      hipLaunchKernelGGL(of_window_solve, dim3((w + TILE - 1) / TILE, h, B), dim3(256), 0, st, M, nf, h, w, ww);
      cur ^= 1;
      f = nf;
    }
    prev = f;
    ph = h; pwid = w;
  }
  return fs_launch_status();
}

// one pyramid level's image pair alone (of_gray, of_blur_h, of_blur_v_resize of level `level`) -> out [B][2][h][w]
extern "C" int fs_optflow_level_image(const FsFlowArgs* a, int level, float* out, void* stream) {
  Plan p;
  if (make_plan(a, p) != FS_OK) return FS_EINVAL;
  if (!a->img0 || !a->img1 || !out || !a->workspace || a->workspace_bytes < p.bytes) return FS_EINVAL;
  if (level < 0 || level > p.L) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(a->workspace);
  float* gray = reinterpret_cast<float*>(ws + p.off_gray);
  float* tmp = reinterpret_cast<float*>(ws + p.off_tmp);
  const long HW = (long)a->H * a->W;
  BlurW bw;
  blur_weights(p.ksize[level], level == 0 ? 0.0 : p.sigma[level], bw);
  hipLaunchKernelGGL(of_gray, dim3(nblk(HW), 2 * a->B), dim3(256), 0, st, a->img0, a->img1, gray, HW);
  hipLaunchKernelGGL(of_blur_h, dim3(nblk(HW), 2 * a->B), dim3(256), 0, st, gray, tmp, a->H, a->W, bw);
  hipLaunchKernelGGL(of_blur_v_resize, dim3(nblk((long)p.h[level] * p.w[level]), 2 * a->B), dim3(256), 0, st, tmp,
                     out, a->H, a->W, p.h[level], p.w[level], bw);
  return fs_launch_status();
}

extern "C" int fs_motion_mask(const FsMotionMaskArgs* a, void* stream) {
  if (!a || !a->flow || !a->P2 || !a->pose || !a->mask) return FS_EINVAL;
  if (a->B < 1 || a->H < 1 || a->W < 1 || (a->mode != 0 && a->mode != 1)) return FS_EINVAL;
  if ((long)a->H * a->W >= (1L << 31)) return FS_EINVAL;
  hipLaunchKernelGGL(of_motion_mask, dim3(nblk((long)a->H * a->W), a->B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), *a);
  return fs_launch_status();
}
