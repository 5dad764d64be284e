// The ConvNeXt backbone's operations that the convolution launches do not cover (vision_base/networks/models/backbone/
// convnext.py): depthwise 7x7 convolution, LayerNorm over channels, exact GELU, layer scale + stochastic depth + residual,
// and the space-to-depth of the patch convolutions (kernel == stride).  NHWC, pixel stride Cp >= C channels, 16-byte
// channel units (VN = 8 values in bf16 compute, 4 in fp32 compute); a tensor flagged *_f32 is fp32 in either mode (the
// residual stream).  Every sum is fp32.  No float atomics: parameter gradients are per-slab partial sums in a workspace
// (the slabs a fixed function of the shape), added up in slab order by a second launch.
// Replaces:
//   nn.Conv2d(dim, dim, 7, padding=3, groups=dim)   convnext.py:27, 38     fs_dwconv7_fwd (flip: its data gradient), _bwd_weight
//   LayerNorm, both data formats                    convnext.py:126-150    fs_layernorm_fwd / _bwd
//   nn.GELU()                                       convnext.py:30, 42     fs_gelu_fwd / _bwd
//   gamma * x, input + drop_path(x)                 convnext.py:44-48      fs_scale_residual_fwd / _bwd
//   Conv2d(k, stride=k) as gather + 1x1 GEMM        convnext.py:75, 82     fs_patch_gather / fs_patch_scatter
//   the bias gradients of the Linear / patch layers, in a fixed order           fs_bias_grad
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>
#include <type_traits>

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int grid_for(long total) { return (int)std::max<long>(1, std::min<long>((total + 255) / 256, 4096)); }

template <int VN> using CompT = std::conditional_t<VN == 8, bf16, float>;

// VN consecutive values at element offset `off` as floats: fp32 compute reads floats; bf16 compute reads bf16, or floats
// where the tensor is flagged f32
template <int VN>
__device__ __forceinline__ void ldv(const void* p, long off, int f32, float* v) {
  if constexpr (VN == 4) {
    loadv<float>(reinterpret_cast<const float*>(p) + off, v);
  } else {
    if (f32) {
      loadv<float>(reinterpret_cast<const float*>(p) + off, v);
      loadv<float>(reinterpret_cast<const float*>(p) + off + 4, v + 4);
    } else {
      loadv<bf16>(reinterpret_cast<const bf16*>(p) + off, v);
    }
  }
}
template <int VN>
__device__ __forceinline__ void stv(void* p, long off, int f32, const float* v) {
  if constexpr (VN == 4) {
    storev<float>(reinterpret_cast<float*>(p) + off, v);
  } else {
    if (f32) {
      storev<float>(reinterpret_cast<float*>(p) + off, v);
      storev<float>(reinterpret_cast<float*>(p) + off + 4, v + 4);
    } else {
      storev<bf16>(reinterpret_cast<bf16*>(p) + off, v);
    }
  }
}
__device__ __forceinline__ float round_bf16(float v) { return bf16_bits_to_f(f_to_bf16_bits(v)); }

// ------------------------------------------------------------------------------------------------ depthwise 7x7
constexpr int DW_TH = 8, DW_TW = 8, DW_CU = 4;               // output pixels and channel units of one forward block
constexpr int DW_PH = DW_TH + 6, DW_PW = DW_TW + 6;          // ... with the 3-pixel halo
constexpr int DWW_C = 32;                                    // channels of one weight-gradient block
constexpr int DWW_ROWS = 50;                                 // workspace rows per slab: 49 taps + the bias

// out[n,h,w,c] = bias[c] + sum_{r,s} w[c][r][s] x[n,h+r-3,w+s-3,c] (+ addend); flip: the taps mirrored = the data gradient.
// One thread = one pixel x one 16-byte channel unit; the tile with its halo is staged once, in the compute dtype.
template <int VN>
__global__ __launch_bounds__(256) void dwconv7_fwd_kernel(const FsDwconv7Args a, int tilesW) {
  using T = CompT<VN>;
  __shared__ uint4 tile[DW_PH * DW_PW * DW_CU];
  __shared__ float wl[49 * DW_CU * VN];
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W, Cp = a.Cp, CU = a.Cp / VN;
  const int cu0 = blockIdx.y * DW_CU, n = blockIdx.z;
  const int h0 = (int)(blockIdx.x / tilesW) * DW_TH, w0 = (int)(blockIdx.x % tilesW) * DW_TW;
  for (int i = tid; i < 49 * DW_CU * VN; i += 256) {
    const int t = i / (DW_CU * VN), c = cu0 * VN + i % (DW_CU * VN);
    wl[i] = c < Cp ? a.wtab[(a.flip ? 48 - t : t) * Cp + c] : 0.f;
  }
  for (int i = tid; i < DW_PH * DW_PW * DW_CU; i += 256) {
    const int cu = i % DW_CU, p = i / DW_CU;
    const int h = h0 + p / DW_PW - 3, w = w0 + p % DW_PW - 3;
    float v[VN];
#pragma unroll
    for (int j = 0; j < VN; ++j) v[j] = 0.f;
    if (h >= 0 && h < H && w >= 0 && w < W && cu0 + cu < CU)
      ldv<VN>(a.x, (((long)n * H + h) * W + w) * Cp + (long)(cu0 + cu) * VN, a.x_f32, v);
    tile[i] = Unit<T>::pack(v);
  }
  __syncthreads();
  const int cu = tid & (DW_CU - 1), p = tid / DW_CU;
  const int py = p / DW_TW, px = p % DW_TW;
  float acc[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) acc[j] = 0.f;
#pragma unroll 1
  for (int r = 0; r < 7; ++r) {      // (one tap row in flight: unrolled over all 49 taps the loads pile up in 400 registers)
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      float xv[VN];
      Unit<T>::unpack(tile[((py + r) * DW_PW + px + s) * DW_CU + cu], xv);
      const float* wp = &wl[((r * 7 + s) * DW_CU + cu) * VN];
#pragma unroll
      for (int j = 0; j < VN; ++j) acc[j] = fmaf(xv[j], wp[j], acc[j]);
    }
  }
  const int h = h0 + py, w = w0 + px;
  if (h >= H || w >= W || cu0 + cu >= CU) return;
  const int c0 = (cu0 + cu) * VN;
  const long off = (((long)n * H + h) * W + w) * Cp + c0;
  float ad[VN];
  if (a.addend) ldv<VN>(a.addend, off, a.addend_f32, ad);
#pragma unroll
  for (int j = 0; j < VN; ++j) {
    float v = acc[j] + (a.bias ? a.bias[c0 + j] : 0.f);
    if (a.addend) v += ad[j];
    acc[j] = c0 + j < a.C ? v : 0.f;
  }
  stv<VN>(a.out, off, a.out_f32, acc);
}

// per slab (a run of 8x8 tiles) and channel: the 49 sums dy * x(shifted) and the sum of dy.  Thread = (channel, tap row r)
// with the row's 7 taps in registers; the eighth role sums dy.  x and dy tiles are staged as floats.
template <int VN>
__global__ __launch_bounds__(256) void dwconv7_wgrad_kernel(const FsDwconv7Args a, int tilesH, int tilesW, int tiles_per_slab,
                                                            int ntiles) {
  __shared__ float xl[DW_PH * DW_PW * DWW_C];
  __shared__ float dl[DW_TH * DW_TW * DWW_C];
  constexpr int UPP = DWW_C / VN;
  const int tid = threadIdx.x, c = tid & (DWW_C - 1), role = tid / DWW_C;
  const int H = a.H, W = a.W, Cp = a.Cp, c0 = blockIdx.y * DWW_C;
  float acc[7];
#pragma unroll
  for (int s = 0; s < 7; ++s) acc[s] = 0.f;
  const int t0 = blockIdx.x * tiles_per_slab, t1 = min(ntiles, t0 + tiles_per_slab);
  for (int t = t0; t < t1; ++t) {
    const int n = t / (tilesH * tilesW), rem = t % (tilesH * tilesW);
    const int h0 = (rem / tilesW) * DW_TH, w0 = (rem % tilesW) * DW_TW;
    __syncthreads();
    for (int i = tid; i < DW_PH * DW_PW * UPP; i += 256) {
      const int u = i % UPP, p = i / UPP;
      const int h = h0 + p / DW_PW - 3, w = w0 + p % DW_PW - 3, cc = c0 + u * VN;
      float v[VN];
#pragma unroll
      for (int j = 0; j < VN; ++j) v[j] = 0.f;
      if (h >= 0 && h < H && w >= 0 && w < W && cc < Cp) {
        ldv<VN>(a.x, (((long)n * H + h) * W + w) * Cp + cc, a.x_f32, v);
        if (VN == 8 && a.x_f32) {       // the forward staged this operand in the compute dtype
#pragma unroll
          for (int j = 0; j < VN; ++j) v[j] = round_bf16(v[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < VN; ++j) xl[p * DWW_C + u * VN + j] = v[j];
    }
    for (int i = tid; i < DW_TH * DW_TW * UPP; i += 256) {
      const int u = i % UPP, p = i / UPP;
      const int h = h0 + p / DW_TW, w = w0 + p % DW_TW, cc = c0 + u * VN;
      float v[VN];
#pragma unroll
      for (int j = 0; j < VN; ++j) v[j] = 0.f;
      if (h < H && w < W && cc < Cp) ldv<VN>(a.dy, (((long)n * H + h) * W + w) * Cp + cc, 0, v);
#pragma unroll
      for (int j = 0; j < VN; ++j) dl[p * DWW_C + u * VN + j] = v[j];
    }
    __syncthreads();
    if (role < 7) {
      for (int py = 0; py < DW_TH; ++py) {
        float xr[DW_PW];
#pragma unroll
        for (int q = 0; q < DW_PW; ++q) xr[q] = xl[((py + role) * DW_PW + q) * DWW_C + c];
#pragma unroll
        for (int px = 0; px < DW_TW; ++px) {
          const float d = dl[(py * DW_TW + px) * DWW_C + c];
#pragma unroll
          for (int s = 0; s < 7; ++s) acc[s] = fmaf(d, xr[px + s], acc[s]);
        }
      }
    } else {
      for (int p = 0; p < DW_TH * DW_TW; ++p) acc[0] += dl[p * DWW_C + c];
    }
  }
  if (c0 + c >= Cp) return;
  float* ws = a.workspace + (long)blockIdx.x * DWW_ROWS * Cp + c0 + c;
  if (role < 7) {
#pragma unroll
    for (int s = 0; s < 7; ++s) ws[(long)(role * 7 + s) * Cp] = acc[s];
  } else {
    ws[(long)49 * Cp] = acc[0];
  }
}

// dw[c][t] (+)= the slabs' partials in slab order; t == 49: dbias[c]
__global__ __launch_bounds__(256) void dwconv7_wgrad_reduce_kernel(const float* __restrict__ ws, int nslab, int C, int Cp,
                                                                   float* __restrict__ dw, float* __restrict__ dbias,
                                                                   int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * DWW_ROWS) return;
  const int t = i % DWW_ROWS, c = i / DWW_ROWS;
  float* dst = t < 49 ? (dw ? dw + (long)c * 49 + t : nullptr) : (dbias ? dbias + c : nullptr);
  if (!dst) return;
  float s = 0.f;
  for (int k = 0; k < nslab; ++k) s += ws[((long)k * DWW_ROWS + t) * Cp + c];
  *dst = accumulate ? *dst + s : s;
}

// ------------------------------------------------------------------------------------------------ LayerNorm
__device__ __forceinline__ float group_sum(float v, int G) {      // over the G (power of two) lanes of a row; all lanes call
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// G lanes per row, K units per lane (unit l + k G): the row stays in registers between the mean, the centred second moment
// and the output
template <int VN, int K>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const FsLayerNormArgs a, int G, int U, int Up) {
  const int tid = threadIdx.x, l = tid & (G - 1);
  const long row = (long)blockIdx.x * (256 / G) + tid / G;
  const bool live = row < a.M;
  const int C = a.C;
  const long base = row * a.Cp;
  float v[K][VN];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = l + k * G;
#pragma unroll
    for (int j = 0; j < VN; ++j) v[k][j] = 0.f;
    if (live && u < U) {
      ldv<VN>(a.x, base + (long)u * VN, a.x_f32, v[k]);
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        if (u * VN + j >= C) v[k][j] = 0.f;
        s += v[k][j];
      }
    }
  }
  const float mean = group_sum(s, G) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = l + k * G;
#pragma unroll
    for (int j = 0; j < VN; ++j)
      if (u * VN + j < C) { const float d = v[k][j] - mean; q += d * d; }
  }
  const float rstd = 1.0f / sqrtf(group_sum(q, G) / (float)C + a.eps);
  if (!live) return;
  if (l == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = l + k * G;
    if (u >= Up) continue;
    float y[VN];
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      const int c = u * VN + j;
      y[j] = c < C ? (v[k][j] - mean) * rstd * a.gamma[c] + a.beta[c] : 0.f;
    }
    stv<VN>(a.y, base + (long)u * VN, a.y_f32, y);
  }
  float z[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) z[j] = 0.f;
  for (int u = l + K * G; u < Up; u += G) stv<VN>(a.y, base + (long)u * VN, a.y_f32, z);
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ addend), g = dy gamma, xhat = (x - mean) rstd
template <int VN, int K>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const FsLayerNormArgs a, int G, int U, int Up) {
  const int tid = threadIdx.x, l = tid & (G - 1);
  const long row = (long)blockIdx.x * (256 / G) + tid / G;
  const bool live = row < a.M;
  const int C = a.C;
  const long base = row * a.Cp;
  const float mean = live ? a.mean[row] : 0.f, rstd = live ? a.rstd[row] : 0.f;
  float xh[K][VN], g[K][VN];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = l + k * G;
#pragma unroll
    for (int j = 0; j < VN; ++j) xh[k][j] = g[k][j] = 0.f;
    if (live && u < U) {
      ldv<VN>(a.x, base + (long)u * VN, a.x_f32, xh[k]);
      ldv<VN>(a.dy, base + (long)u * VN, a.y_f32, g[k]);
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const int c = u * VN + j;
        if (c < C) {
          xh[k][j] = (xh[k][j] - mean) * rstd;
          g[k][j] *= a.gamma[c];
          s1 += g[k][j];
          s2 += g[k][j] * xh[k][j];
        } else {
          xh[k][j] = g[k][j] = 0.f;
        }
      }
    }
  }
  const float m1 = group_sum(s1, G) / (float)C, m2 = group_sum(s2, G) / (float)C;
  if (!live) return;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int u = l + k * G;
    if (u >= Up) continue;
    float d[VN], ad[VN];
    if (a.addend) ldv<VN>(a.addend, base + (long)u * VN, a.addend_f32, ad);
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      float t = rstd * (g[k][j] - m1 - xh[k][j] * m2);
      if (a.addend) t += ad[j];
      d[j] = u * VN + j < C ? t : 0.f;
    }
    stv<VN>(a.dx, base + (long)u * VN, a.x_f32, d);
  }
  float z[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) z[j] = 0.f;
  for (int u = l + K * G; u < Up; u += G) stv<VN>(a.dx, base + (long)u * VN, a.x_f32, z);
}

// column sums over a slab of rows: 16 units x 16 row lanes per block; the row lanes are added in lane order
constexpr int COL_U = 16, COL_R = 16;
inline int col_slabs(long M) { return (int)std::max<long>(1, std::min<long>(256, (M + 63) / 64)); }

template <int VN>
__device__ __forceinline__ void col_reduce_store(float (*red)[COL_U * VN], const float* v, int r, int ul, float* dst) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < VN; ++j) red[r][ul * VN + j] = v[j];
  __syncthreads();
  if (r == 0 && dst) {
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      float s = 0.f;
      for (int rr = 0; rr < COL_R; ++rr) s += red[rr][ul * VN + j];
      dst[j] = s;
    }
  }
}

// workspace [slab][2][Cp]: sum dy xhat, sum dy
template <int VN>
__global__ __launch_bounds__(256) void ln_bwd_param_kernel(const FsLayerNormArgs a, long rows_per_slab, int Up) {
  __shared__ float red[COL_R][COL_U * VN];
  const int tid = threadIdx.x, ul = tid & (COL_U - 1), r = tid / COL_U;
  const int u = blockIdx.y * COL_U + ul;
  const long row0 = (long)blockIdx.x * rows_per_slab, row1 = std::min<long>(a.M, row0 + rows_per_slab);
  float dg[VN], db[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) dg[j] = db[j] = 0.f;
  if (u < Up)
    for (long row = row0 + r; row < row1; row += COL_R) {
      float x[VN], d[VN];
      ldv<VN>(a.x, row * a.Cp + (long)u * VN, a.x_f32, x);
      ldv<VN>(a.dy, row * a.Cp + (long)u * VN, a.y_f32, d);
      const float mean = a.mean[row], rstd = a.rstd[row];
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        dg[j] += d[j] * ((x[j] - mean) * rstd);
        db[j] += d[j];
      }
    }
  float* ws = a.workspace + (long)blockIdx.x * 2 * a.Cp + (long)u * VN;
  col_reduce_store<VN>(red, dg, r, ul, u < Up ? ws : nullptr);
  col_reduce_store<VN>(red, db, r, ul, u < Up ? ws + a.Cp : nullptr);
}

// workspace [slab][Cp]: the column sums of x over the slab's rows (a bias gradient without fs_channel_sum's float atomics)
template <int VN>
__global__ __launch_bounds__(256) void bias_grad_kernel(const void* __restrict__ x, int x_f32, float* __restrict__ ws, long M,
                                                        int Cp, long rows_per_slab, int Up) {
  __shared__ float red[COL_R][COL_U * VN];
  const int tid = threadIdx.x, ul = tid & (COL_U - 1), r = tid / COL_U;
  const int u = blockIdx.y * COL_U + ul;
  const long row0 = (long)blockIdx.x * rows_per_slab, row1 = std::min<long>(M, row0 + rows_per_slab);
  float acc[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) acc[j] = 0.f;
  if (u < Up)
    for (long row = row0 + r; row < row1; row += COL_R) {
      float v[VN];
      ldv<VN>(x, row * Cp + (long)u * VN, x_f32, v);
#pragma unroll
      for (int j = 0; j < VN; ++j) acc[j] += v[j];
    }
  col_reduce_store<VN>(red, acc, r, ul, u < Up ? ws + (long)blockIdx.x * Cp + (long)u * VN : nullptr);
}

// dst_k[i] (+)= sum over slabs, in slab order, of ws[slab * slab_stride + off_k + i], i < n
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ ws, int nslab, long slab_stride, int n,
                                                          float* __restrict__ dst0, long off0, float* __restrict__ dst1,
                                                          long off1, int accumulate, const float* __restrict__ scale1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dst0) {
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += ws[k * slab_stride + off0 + i];
    dst0[i] = accumulate ? dst0[i] + s : s;
  }
  if (dst1) {
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += ws[k * slab_stride + off1 + i];
    if (scale1) s *= scale1[i];
    dst1[i] = accumulate ? dst1[i] + s : s;
  }
}

// ------------------------------------------------------------------------------------------------ GELU (erf form)
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_df(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out, long n) {
  constexpr int VN = VecN<T>::N;
  const long nv = n / VN;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    float v[VN], d[VN];
    loadv<T>(x + i * VN, v);
    if constexpr (BWD) loadv<T>(dy + i * VN, d);
#pragma unroll
    for (int j = 0; j < VN; ++j) v[j] = BWD ? d[j] * gelu_df(v[j]) : gelu_f(v[j]);
    storev<T>(out + i * VN, v);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - nv * VN)) {      // the tail that is no whole vector
    const long i = nv * VN + threadIdx.x;
    const float v = ElemTraits<T>::to_f(x[i]);
    out[i] = ElemTraits<T>::from_f(BWD ? ElemTraits<T>::to_f(dy[i]) * gelu_df(v) : gelu_f(v));
  }
}

// ------------------------------------------------------------------------------------------------ scale + residual
// out = inp + keep[n] gamma[c] z; out_c: a copy of out in the compute dtype
template <int VN>
__global__ __launch_bounds__(256) void scale_residual_fwd_kernel(const FsScaleResidualArgs a) {
  const int Up = a.Cp / VN;
  const long M = (long)a.N * a.HW, total = M * Up;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int u = (int)(i % Up);
    const long m = i / Up, off = m * a.Cp + (long)u * VN;
    const float keep = a.keep ? a.keep[m / a.HW] : 1.f;
    float x[VN], z[VN];
    ldv<VN>(a.inp, off, a.stream_f32, x);
    ldv<VN>(a.z, off, 0, z);
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      const int c = u * VN + j;
      // a dropped sample keeps its input bit for bit, whatever the branch holds
      x[j] = c < a.C ? (keep != 0.f ? x[j] + keep * (a.gamma ? a.gamma[c] : 1.f) * z[j] : x[j]) : 0.f;
    }
    stv<VN>(a.out, off, a.stream_f32, x);
    if (a.out_c) stv<VN>(a.out_c, off, 0, x);
  }
}

// dz = keep[n] gamma[c] dout; workspace [slab][2][Cp]: sum keep[n] dout z (dgamma) and sum keep[n] dout (times gamma: the
// gradient of the bias behind z, from the unrounded gradient)
template <int VN>
__global__ __launch_bounds__(256) void scale_residual_bwd_kernel(const FsScaleResidualArgs a, long rows_per_slab, int Up) {
  __shared__ float red[COL_R][COL_U * VN];
  const int tid = threadIdx.x, ul = tid & (COL_U - 1), r = tid / COL_U;
  const int u = blockIdx.y * COL_U + ul;
  const long M = (long)a.N * a.HW;
  const long row0 = (long)blockIdx.x * rows_per_slab, row1 = std::min<long>(M, row0 + rows_per_slab);
  const bool want_g = a.dgamma != nullptr, want_b = a.dbias != nullptr;
  float dg[VN], db[VN], gam[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) {
    dg[j] = db[j] = 0.f;
    const int c = u * VN + j;
    gam[j] = c < a.C ? (a.gamma ? a.gamma[c] : 1.f) : 0.f;
  }
  if (u < Up)
    for (long row = row0 + r; row < row1; row += COL_R) {
      const long off = row * a.Cp + (long)u * VN;
      const float keep = a.keep ? a.keep[row / a.HW] : 1.f;
      float d[VN], z[VN];
      ldv<VN>(a.dout, off, a.stream_f32, d);
      if (want_g) ldv<VN>(a.z, off, 0, z);
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        // (padding channels: zero whatever dout and z hold there)
        const float kd = (keep != 0.f && u * VN + j < a.C) ? keep * d[j] : 0.f;
        if (want_g) dg[j] += u * VN + j < a.C ? kd * z[j] : 0.f;
        db[j] += kd;
        d[j] = kd * gam[j];
      }
      stv<VN>(a.dz, off, 0, d);
    }
  float* ws = a.workspace + (long)blockIdx.x * 2 * a.Cp + (long)u * VN;
  if (want_g) col_reduce_store<VN>(red, dg, r, ul, u < Up ? ws : nullptr);
  if (want_b) col_reduce_store<VN>(red, db, r, ul, u < Up ? ws + a.Cp : nullptr);
}

// ------------------------------------------------------------------------------------------------ patch gather / scatter
// 16-byte units only.  GATHER: out[n,ho,wo,(r k + s) CU + u] = x[n, ho k + r, wo k + s, u].  Scatter: its inverse over
// every unit of dx, zero in the rows and columns the floor drops.
template <bool GATHER>
__global__ __launch_bounds__(256) void patch_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long N, int H, int W,
                                                    int CU, int k) {
  const int Ho = H / k, Wo = W / k;
  const long total = GATHER ? N * Ho * Wo * k * k * CU : N * H * W * CU;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    if constexpr (GATHER) {
      const int u = (int)(i % CU); long q = i / CU;
      const int s = (int)(q % k); q /= k;
      const int r = (int)(q % k); q /= k;
      const int wo = (int)(q % Wo); q /= Wo;
      const int ho = (int)(q % Ho); const long n = q / Ho;
      dst[i] = src[((n * H + ho * k + r) * W + wo * k + s) * CU + u];
    } else {
      const int u = (int)(i % CU); long q = i / CU;
      const int w = (int)(q % W); q /= W;
      const int h = (int)(q % H); const long n = q / H;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (h < Ho * k && w < Wo * k)
        v = src[((((n * Ho + h / k) * Wo + w / k) * k + h % k) * k + w % k) * CU + u];
      dst[i] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool dtype_ok(int dtype) { return dtype == FS_DTYPE_BF16 || dtype == FS_DTYPE_F32; }
inline int vec_of(int dtype) { return dtype == FS_DTYPE_BF16 ? 8 : 4; }

bool dwconv_geometry_ok(const FsDwconv7Args* a, int vn) {
  return a && a->N > 0 && a->N <= 65535 && a->H > 0 && a->W > 0 && a->C > 0 && a->Cp >= a->C && a->Cp % vn == 0 &&
         (long)a->N * a->H * a->W * a->Cp < (1L << 40);
}
inline int dw_tiles(int v, int t) { return (v + t - 1) / t; }

// slabs of the weight gradient: runs of whole tiles, at most 128 and about 1024 blocks over all channel groups
void dww_plan(int N, int H, int W, int Cp, int* tilesH, int* tilesW, int* ntiles, int* tps, int* nslab, int* cgroups) {
  *tilesH = dw_tiles(H, DW_TH); *tilesW = dw_tiles(W, DW_TW);
  const long nt = (long)N * *tilesH * *tilesW;
  *ntiles = (int)nt;
  *cgroups = (Cp + DWW_C - 1) / DWW_C;
  const long want = std::max<long>(1, std::min<long>(128, 1024 / *cgroups));
  const long slabs = std::min<long>(nt, want);
  *tps = (int)((nt + slabs - 1) / slabs);
  *nslab = (int)((nt + *tps - 1) / *tps);
}

template <int VN, int K>
void ln_launch(bool bwd, const FsLayerNormArgs& a, int G, int U, int Up, hipStream_t st) {
  const long rows = 256 / G;
  dim3 grid((unsigned)((a.M + rows - 1) / rows));
  if (bwd) hipLaunchKernelGGL((ln_bwd_kernel<VN, K>), grid, dim3(256), 0, st, a, G, U, Up);
  else hipLaunchKernelGGL((ln_fwd_kernel<VN, K>), grid, dim3(256), 0, st, a, G, U, Up);
}

template <int VN>
int ln_dispatch(bool bwd, const FsLayerNormArgs& a, hipStream_t st) {
  const int U = (a.C + VN - 1) / VN, Up = a.Cp / VN;
  int G = 4;
  while (G < 64 && G < U) G <<= 1;
  const int per = (U + G - 1) / G;
  if (per <= 1) ln_launch<VN, 1>(bwd, a, G, U, Up, st);
  else if (per <= 2) ln_launch<VN, 2>(bwd, a, G, U, Up, st);
  else if (per <= 4) ln_launch<VN, 4>(bwd, a, G, U, Up, st);
  else if (per <= 8) ln_launch<VN, 8>(bwd, a, G, U, Up, st);
  else return FS_EINVAL;
  return FS_OK;
}

bool ln_geometry_ok(const FsLayerNormArgs* a, int vn) {
  return a && a->M > 0 && a->M < (1L << 31) && a->C > 0 && a->Cp >= a->C && a->Cp % vn == 0 &&
         (a->C + vn - 1) / vn <= 64 * 8 && a->eps >= 0.f && a->M * a->Cp < (1L << 40);
}

bool sr_geometry_ok(const FsScaleResidualArgs* a, int vn) {
  return a && a->N > 0 && a->HW > 0 && a->C > 0 && a->Cp >= a->C && a->Cp % vn == 0 && (long)a->N * a->HW < (1L << 31) &&
         (long)a->N * a->HW * a->Cp < (1L << 40);
}

}  // namespace

extern "C" int fs_dwconv7_tile(int dtype, int32_t* rows, int32_t* cols, int32_t* channels) {
  if (!dtype_ok(dtype) || !rows || !cols || !channels) return FS_EINVAL;
  *rows = DW_TH; *cols = DW_TW; *channels = DW_CU * vec_of(dtype);
  return FS_OK;
}

extern "C" int64_t fs_dwconv7_workspace_bytes(int N, int H, int W, int Cp) {
  if (N <= 0 || H <= 0 || W <= 0 || Cp <= 0 || (long)N * dw_tiles(H, DW_TH) * dw_tiles(W, DW_TW) >= (1L << 31)) return -1;
  int tH, tW, nt, tps, nslab, cg;
  dww_plan(N, H, W, Cp, &tH, &tW, &nt, &tps, &nslab, &cg);
  return (int64_t)nslab * DWW_ROWS * Cp * 4;
}

extern "C" int fs_dwconv7_fwd(const FsDwconv7Args* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!dwconv_geometry_ok(a, vn) || !a->x || !a->wtab || !a->out || !aligned16(a->x) || !aligned16(a->out) ||
      (a->addend && !aligned16(a->addend)))
    return FS_EINVAL;
  const int tH = dw_tiles(a->H, DW_TH), tW = dw_tiles(a->W, DW_TW);
  const int gy = (a->Cp / vn + DW_CU - 1) / DW_CU;
  if ((long)tH * tW >= (1L << 31) || gy > 65535) return FS_EINVAL;
  dim3 grid((unsigned)(tH * tW), (unsigned)gy, (unsigned)a->N);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vn == 8) hipLaunchKernelGGL(dwconv7_fwd_kernel<8>, grid, dim3(256), 0, st, *a, tW);
  else hipLaunchKernelGGL(dwconv7_fwd_kernel<4>, grid, dim3(256), 0, st, *a, tW);
  return fs_launch_status();
}

extern "C" int fs_dwconv7_bwd_weight(const FsDwconv7Args* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!dwconv_geometry_ok(a, vn) || !a->x || !a->dy || !a->workspace || (!a->dw && !a->dbias) || !aligned16(a->x) ||
      !aligned16(a->dy) || (long)a->N * dw_tiles(a->H, DW_TH) * dw_tiles(a->W, DW_TW) >= (1L << 31))
    return FS_EINVAL;
  int tH, tW, nt, tps, nslab, cg;
  dww_plan(a->N, a->H, a->W, a->Cp, &tH, &tW, &nt, &tps, &nslab, &cg);
  if (a->workspace_bytes < (int64_t)nslab * DWW_ROWS * a->Cp * 4 || cg > 65535) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)nslab, (unsigned)cg);
  if (vn == 8) hipLaunchKernelGGL(dwconv7_wgrad_kernel<8>, grid, dim3(256), 0, st, *a, tH, tW, tps, nt);
  else hipLaunchKernelGGL(dwconv7_wgrad_kernel<4>, grid, dim3(256), 0, st, *a, tH, tW, tps, nt);
  hipLaunchKernelGGL(dwconv7_wgrad_reduce_kernel, dim3((a->C * DWW_ROWS + 255) / 256), dim3(256), 0, st, a->workspace, nslab,
                     a->C, a->Cp, a->dw, a->dbias, a->accumulate);
  return fs_launch_status();
}

extern "C" int64_t fs_layernorm_workspace_bytes(int64_t M, int Cp) {
  if (M <= 0 || Cp <= 0) return -1;
  return (int64_t)col_slabs(M) * 2 * Cp * 4;
}

extern "C" int fs_layernorm_fwd(const FsLayerNormArgs* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!ln_geometry_ok(a, vn) || !a->x || !a->y || !a->gamma || !a->beta || !a->mean || !a->rstd || !aligned16(a->x) ||
      !aligned16(a->y))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = vn == 8 ? ln_dispatch<8>(false, *a, st) : ln_dispatch<4>(false, *a, st);
  return rc != FS_OK ? rc : fs_launch_status();
}

extern "C" int fs_layernorm_bwd(const FsLayerNormArgs* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  const bool params = a && (a->dgamma || a->dbeta);
  if (!ln_geometry_ok(a, vn) || !a->x || !a->dy || !a->gamma || !a->mean || !a->rstd || (!a->dx && !params) ||
      !aligned16(a->x) || !aligned16(a->dy) || (a->dx && !aligned16(a->dx)) || (a->addend && !aligned16(a->addend)))
    return FS_EINVAL;
  const int nslab = col_slabs(a->M);
  if (params && (!a->workspace || a->workspace_bytes < (int64_t)nslab * 2 * a->Cp * 4)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a->dx) {
    const int rc = vn == 8 ? ln_dispatch<8>(true, *a, st) : ln_dispatch<4>(true, *a, st);
    if (rc != FS_OK) return rc;
  }
  if (params) {
    const long rps = (a->M + nslab - 1) / nslab;
    const int Up = a->Cp / vn;
    dim3 grid((unsigned)nslab, (unsigned)((Up + COL_U - 1) / COL_U));
    if (vn == 8) hipLaunchKernelGGL(ln_bwd_param_kernel<8>, grid, dim3(256), 0, st, *a, rps, Up);
    else hipLaunchKernelGGL(ln_bwd_param_kernel<4>, grid, dim3(256), 0, st, *a, rps, Up);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((a->C + 255) / 256), dim3(256), 0, st, a->workspace, nslab, (long)2 * a->Cp, a->C,
                       a->dgamma, 0L, a->dbeta, (long)a->Cp, a->accumulate, (const float*)nullptr);
  }
  return fs_launch_status();
}

extern "C" int fs_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream) {
  if (!dtype_ok(dtype) || !x || !y || n <= 0 || !aligned16(x) || !aligned16(y)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for(n / vec_of(dtype)));
  if (dtype == FS_DTYPE_BF16)
    hipLaunchKernelGGL((gelu_kernel<bf16, false>), grid, dim3(256), 0, st, (const bf16*)x, (const bf16*)nullptr, (bf16*)y, (long)n);
  else
    hipLaunchKernelGGL((gelu_kernel<float, false>), grid, dim3(256), 0, st, (const float*)x, (const float*)nullptr, (float*)y, (long)n);
  return fs_launch_status();
}

extern "C" int fs_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, void* stream) {
  if (!dtype_ok(dtype) || !x || !dy || !dx || n <= 0 || !aligned16(x) || !aligned16(dy) || !aligned16(dx)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for(n / vec_of(dtype)));
  if (dtype == FS_DTYPE_BF16)
    hipLaunchKernelGGL((gelu_kernel<bf16, true>), grid, dim3(256), 0, st, (const bf16*)x, (const bf16*)dy, (bf16*)dx, (long)n);
  else
    hipLaunchKernelGGL((gelu_kernel<float, true>), grid, dim3(256), 0, st, (const float*)x, (const float*)dy, (float*)dx, (long)n);
  return fs_launch_status();
}

extern "C" int fs_bias_grad(const void* x, float* dbias, float* workspace, int64_t workspace_bytes, int64_t M, int C, int Cp,
                            int x_f32, int accumulate, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!x || !dbias || !workspace || M <= 0 || M >= (1L << 31) || C <= 0 || Cp < C || Cp % vn || !aligned16(x) ||
      M * Cp >= (1L << 40))
    return FS_EINVAL;
  const int nslab = col_slabs(M);
  if (workspace_bytes < (int64_t)nslab * Cp * 4) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long rps = (M + nslab - 1) / nslab;
  const int Up = Cp / vn;
  dim3 grid((unsigned)nslab, (unsigned)((Up + COL_U - 1) / COL_U));
  if (vn == 8) hipLaunchKernelGGL(bias_grad_kernel<8>, grid, dim3(256), 0, st, x, x_f32, workspace, (long)M, Cp, rps, Up);
  else hipLaunchKernelGGL(bias_grad_kernel<4>, grid, dim3(256), 0, st, x, x_f32, workspace, (long)M, Cp, rps, Up);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((C + 255) / 256), dim3(256), 0, st, workspace, nslab, (long)Cp, C, dbias, 0L,
                     (float*)nullptr, 0L, accumulate, (const float*)nullptr);
  return fs_launch_status();
}

extern "C" int64_t fs_scale_residual_workspace_bytes(int64_t M, int Cp) {
  if (M <= 0 || Cp <= 0) return -1;
  return (int64_t)col_slabs(M) * 2 * Cp * 4;
}

extern "C" int fs_scale_residual_fwd(const FsScaleResidualArgs* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!sr_geometry_ok(a, vn) || !a->inp || !a->z || !a->out || !aligned16(a->inp) || !aligned16(a->z) || !aligned16(a->out) ||
      (a->out_c && !aligned16(a->out_c)))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for((long)a->N * a->HW * (a->Cp / vn)));
  if (vn == 8) hipLaunchKernelGGL(scale_residual_fwd_kernel<8>, grid, dim3(256), 0, st, *a);
  else hipLaunchKernelGGL(scale_residual_fwd_kernel<4>, grid, dim3(256), 0, st, *a);
  return fs_launch_status();
}

extern "C" int fs_scale_residual_bwd(const FsScaleResidualArgs* a, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!sr_geometry_ok(a, vn) || !a->dout || !a->dz || !aligned16(a->dout) || !aligned16(a->dz) ||
      (a->dgamma && (!a->gamma || !a->z || !a->workspace || !aligned16(a->z))) || (a->dbias && !a->workspace))
    return FS_EINVAL;
  const long M = (long)a->N * a->HW;
  const int nslab = col_slabs(M);
  const bool params = a->dgamma || a->dbias;
  if (params && a->workspace_bytes < (int64_t)nslab * 2 * a->Cp * 4) return FS_EINVAL;
  const FsScaleResidualArgs& b = *a;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long rps = (M + nslab - 1) / nslab;
  const int Up = a->Cp / vn;
  dim3 grid((unsigned)nslab, (unsigned)((Up + COL_U - 1) / COL_U));
  if (vn == 8) hipLaunchKernelGGL(scale_residual_bwd_kernel<8>, grid, dim3(256), 0, st, b, rps, Up);
  else hipLaunchKernelGGL(scale_residual_bwd_kernel<4>, grid, dim3(256), 0, st, b, rps, Up);
  if (params)
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((a->C + 255) / 256), dim3(256), 0, st, a->workspace, nslab, (long)2 * a->Cp, a->C,
                       a->dgamma, 0L, a->dbias, (long)a->Cp, a->accumulate, a->gamma);
  return fs_launch_status();
}

static int patch_launch(bool gather, const void* src, void* dst, int N, int H, int W, int Cp, int k, int dtype, void* stream) {
  if (!dtype_ok(dtype)) return FS_EINVAL;
  const int vn = vec_of(dtype);
  if (!src || !dst || N <= 0 || H <= 0 || W <= 0 || Cp <= 0 || Cp % vn || k < 1 || k > 8 || H < k || W < k ||
      !aligned16(src) || !aligned16(dst) || (long)N * H * W * Cp >= (1L << 40))
    return FS_EINVAL;
  const int CU = Cp / vn;
  const long total = gather ? (long)N * (H / k) * (W / k) * k * k * CU : (long)N * H * W * CU;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for(total));
  if (gather)
    hipLaunchKernelGGL(patch_kernel<true>, grid, dim3(256), 0, st, (const uint4*)src, (uint4*)dst, (long)N, H, W, CU, k);
  else
    hipLaunchKernelGGL(patch_kernel<false>, grid, dim3(256), 0, st, (const uint4*)src, (uint4*)dst, (long)N, H, W, CU, k);
  return fs_launch_status();
}

extern "C" int fs_patch_gather(const void* x, void* out, int N, int H, int W, int Cp, int k, int dtype, void* stream) {
  return patch_launch(true, x, out, N, H, W, Cp, k, dtype, stream);
}

extern "C" int fs_patch_scatter(const void* dg, void* dx, int N, int H, int W, int Cp, int k, int dtype, void* stream) {
  return patch_launch(false, dg, dx, N, H, W, Cp, k, dtype, stream);
}
