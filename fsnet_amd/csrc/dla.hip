// The two memory-bound pieces of the DLA backbone (vision_base/networks/models/backbone/dla.py) that the convolution
// and BatchNorm launches do not cover.  NHWC, one 16-byte lane (8 bf16 / 4 f32 channels) per thread, grid-stride.
// Replaces:
//   nn.MaxPool2d(2, stride=2)      dla.py:207-208, 218   (Tree.downsample)
//   torch.cat(x, 1)                dla.py:167            (Root.forward) and its split in the backward
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

inline int grid_for(long total) { return (int)std::max<long>(1, std::min<long>((total + 255) / 256, 2048)); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// y[n, ho, wo, y_off + c] = max over the 2x2 window; idx = position 2 * r + s of the maximum.  Position 0 is taken as it
// is, a later one only where it is strictly greater (fs_maxpool_fwd's rule: ties go to the first position in row-major
// order as in ATen; a NaN stays where it is at position 0 and is never picked anywhere else).
template <typename T>
__global__ __launch_bounds__(256) void pool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx,
                                                        long N, int H, int W, int C, long y_pix, long y_off) {
  constexpr int VN = VecN<T>::N;
  const int CG = C / VN, Ho = H / 2, Wo = W / 2;
  const long total = N * Ho * Wo * CG;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cg = (int)(i % CG); const long m = i / CG;
    const int wo = (int)(m % Wo); const long q = m / Wo; const int ho = (int)(q % Ho); const long n = q / Ho;
    const T* p = x + ((n * H + 2 * ho) * W + 2 * wo) * C + cg * VN;
    float best[VN], v[VN];
    uint32_t bi[VN];
    loadv<T>(p, best);
#pragma unroll
    for (int j = 0; j < VN; ++j) bi[j] = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      loadv<T>(p + ((long)(k >> 1) * W + (k & 1)) * C, v);
#pragma unroll
      for (int j = 0; j < VN; ++j)
        if (v[j] > best[j]) { best[j] = v[j]; bi[j] = k; }
    }
    storev<T>(y + m * y_pix + y_off + cg * VN, best);
    uint32_t* ip = reinterpret_cast<uint32_t*>(idx + m * C + cg * VN);
#pragma unroll
    for (int k = 0; k < VN / 4; ++k)
      ip[k] = bi[4 * k] | (bi[4 * k + 1] << 8) | (bi[4 * k + 2] << 16) | (bi[4 * k + 3] << 24);
  }
}

// gather form, one thread per dx vector: dx = (idx == own position ? dy : 0) + addend — every element written once
template <typename T>
__global__ __launch_bounds__(256) void pool2_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                        const T* __restrict__ addend, T* __restrict__ dx, long N, int H,
                                                        int W, int C, long dy_pix, long dy_off) {
  constexpr int VN = VecN<T>::N;
  const int CG = C / VN, Ho = H / 2, Wo = W / 2;
  const long total = N * H * W * CG;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cg = (int)(i % CG); const long m = i / CG;
    const int w = (int)(m % W); const long q = m / W; const int h = (int)(q % H); const long n = q / H;
    const long mo = (n * Ho + (h >> 1)) * Wo + (w >> 1);
    const uint32_t code = (uint32_t)((h & 1) * 2 + (w & 1));
    float g[VN], acc[VN];
    loadv<T>(dy + mo * dy_pix + dy_off + cg * VN, g);
    const uint32_t* ip = reinterpret_cast<const uint32_t*>(idx + mo * C + cg * VN);
    uint32_t packed[VN / 4];
#pragma unroll
    for (int k = 0; k < VN / 4; ++k) packed[k] = ip[k];
    if (addend) loadv<T>(addend + m * C + cg * VN, acc);
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      const float t = ((packed[j >> 2] >> (8 * (j & 3))) & 0xffu) == code ? g[j] : 0.f;
      acc[j] = addend ? acc[j] + t : t;
    }
    storev<T>(dx + m * C + cg * VN, acc);
  }
}

// the parts of one concatenation with a vector-group prefix table: part k owns groups [g0[k], g0[k + 1]) of a row
struct CatParts {
  void* part[FS_CAT_MAX];
  int32_t C[FS_CAT_MAX], off[FS_CAT_MAX], accumulate[FS_CAT_MAX], g0[FS_CAT_MAX + 1];
  int32_t n;
};

// BWD = false: wide[m, off_k + c] = part_k[m, c].  BWD = true: part_k[m, c] = wide[m, off_k + c] (+ part_k[m, c]).
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void cat_kernel(const CatParts p, T* __restrict__ wide, long M, int Ctot) {
  constexpr int VN = VecN<T>::N;
  const int G = p.g0[p.n];
  const long total = M * G;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int g = (int)(i % G); const long m = i / G;
    // (selected with compile-time indices: a lane-varying index into the argument struct would copy it to scratch)
    T* part = reinterpret_cast<T*>(p.part[0]);
    int Ck = p.C[0], offk = p.off[0], acck = p.accumulate[0], g0k = 0;
#pragma unroll
    for (int t = 1; t < FS_CAT_MAX; ++t)
      if (t < p.n && g >= p.g0[t]) {
        part = reinterpret_cast<T*>(p.part[t]); Ck = p.C[t]; offk = p.off[t]; acck = p.accumulate[t]; g0k = p.g0[t];
      }
    const int c = (g - g0k) * VN;
    part += m * Ck + c;
    T* w = wide + m * Ctot + offk + c;
    float v[VN];
    if constexpr (!BWD) {
      loadv<T>(part, v);
      storev<T>(w, v);
    } else {
      loadv<T>(w, v);
      if (acck) {
        float a[VN];
        loadv<T>(part, a);
#pragma unroll
        for (int j = 0; j < VN; ++j) v[j] += a[j];
      }
      storev<T>(part, v);
    }
  }
}

// FS_EINVAL, or FS_OK with the prefix table of the parts that are present filled in
int cat_parts(const FsCatArgs* a, int vn, CatParts* cp) {
  if (!a || !a->wide || a->n < 1 || a->n > FS_CAT_MAX || a->M <= 0 || a->Ctot <= 0 || a->Ctot % vn || !aligned16(a->wide))
    return FS_EINVAL;
  cp->n = 0;
  cp->g0[0] = 0;
  for (int i = 0; i < a->n; ++i) {
    if (a->C[i] <= 0 || a->C[i] % vn || a->off[i] < 0 || a->off[i] % vn || (long)a->off[i] + a->C[i] > a->Ctot)
      return FS_EINVAL;
    for (int j = 0; j < i; ++j)       // channel slices of two parts never overlap
      if (a->off[i] < a->off[j] + a->C[j] && a->off[j] < a->off[i] + a->C[i]) return FS_EINVAL;
    if (!a->part[i]) continue;        // a part that lives in its slice already (forward) or is read from it (backward)
    if (!aligned16(a->part[i])) return FS_EINVAL;
    const int k = cp->n++;
    cp->part[k] = a->part[i]; cp->C[k] = a->C[i]; cp->off[k] = a->off[i]; cp->accumulate[k] = a->accumulate[i];
    cp->g0[k + 1] = cp->g0[k] + a->C[i] / vn;
  }
  for (int k = cp->n; k < FS_CAT_MAX; ++k) {
    cp->part[k] = nullptr; cp->C[k] = cp->off[k] = cp->accumulate[k] = 0; cp->g0[k + 1] = cp->g0[cp->n];
  }
  return FS_OK;
}

template <bool BWD>
int cat_launch(const FsCatArgs* a, int dtype, void* stream) {
  if (dtype != FS_DTYPE_BF16 && dtype != FS_DTYPE_F32) return FS_EINVAL;
  CatParts cp;
  if (cat_parts(a, dtype == FS_DTYPE_BF16 ? 8 : 4, &cp) != FS_OK) return FS_EINVAL;
  if (cp.n == 0) return FS_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for(a->M * cp.g0[cp.n]));
  if (dtype == FS_DTYPE_BF16)
    hipLaunchKernelGGL((cat_kernel<bf16, BWD>), grid, dim3(256), 0, st, cp, (bf16*)a->wide, (long)a->M, a->Ctot);
  else
    hipLaunchKernelGGL((cat_kernel<float, BWD>), grid, dim3(256), 0, st, cp, (float*)a->wide, (long)a->M, a->Ctot);
  return fs_launch_status();
}

bool pool2_ok(const void* a, const void* b, const void* c, int N, int H, int W, int C, int64_t pix, int64_t off, int vn) {
  return a && b && c && N > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % vn == 0 && off >= 0 &&
         off % vn == 0 && pix % vn == 0 && off + C <= pix && aligned16(a) && aligned16(b);
}

}  // namespace

extern "C" int fs_pool2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int64_t y_pix,
                            int64_t y_off, int dtype, void* stream) {
  if (dtype != FS_DTYPE_BF16 && dtype != FS_DTYPE_F32) return FS_EINVAL;
  const int vn = dtype == FS_DTYPE_BF16 ? 8 : 4;
  if (!pool2_ok(x, y, idx, N, H, W, C, y_pix, y_off, vn) || (reinterpret_cast<uintptr_t>(idx) & 3u)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for((long)N * (H / 2) * (W / 2) * (C / vn)));
  if (dtype == FS_DTYPE_BF16)
    hipLaunchKernelGGL(pool2_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, (bf16*)y, idx, (long)N, H, W, C, (long)y_pix, (long)y_off);
  else
    hipLaunchKernelGGL(pool2_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (float*)y, idx, (long)N, H, W, C, (long)y_pix, (long)y_off);
  return fs_launch_status();
}

extern "C" int fs_pool2_bwd(const void* dy, const uint8_t* idx, const void* addend, void* dx, int N, int H, int W, int C,
                            int64_t dy_pix, int64_t dy_off, int dtype, void* stream) {
  if (dtype != FS_DTYPE_BF16 && dtype != FS_DTYPE_F32) return FS_EINVAL;
  const int vn = dtype == FS_DTYPE_BF16 ? 8 : 4;
  if (!pool2_ok(dy, dx, idx, N, H, W, C, dy_pix, dy_off, vn) || (reinterpret_cast<uintptr_t>(idx) & 3u) ||
      (addend && !aligned16(addend)))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(grid_for((long)N * H * W * (C / vn)));
  if (dtype == FS_DTYPE_BF16)
    hipLaunchKernelGGL(pool2_bwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)dy, idx, (const bf16*)addend, (bf16*)dx, (long)N, H, W, C, (long)dy_pix, (long)dy_off);
  else
    hipLaunchKernelGGL(pool2_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)dy, idx, (const float*)addend, (float*)dx, (long)N, H, W, C, (long)dy_pix, (long)dy_off);
  return fs_launch_status();
}

extern "C" int fs_cat_fwd(const FsCatArgs* args, int dtype, void* stream) { return cat_launch<false>(args, dtype, stream); }
extern "C" int fs_cat_bwd(const FsCatArgs* args, int dtype, void* stream) { return cat_launch<true>(args, dtype, stream); }
