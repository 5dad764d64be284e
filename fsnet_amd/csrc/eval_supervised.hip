// Supervised KITTI depth-benchmark metrics on the device, and the quantiser that writes predictions for them.
// Replaces:
//   compute_errors (nine metrics, a Python double loop under numba)   monodepth/evaluation/kitti_supervised_eval.py:7-81
//   cv2.imread(path, -1) / scale of both operands                     kitti_supervised_eval.py:102, 138-139
//   uint16(depth * 256) of the KITTI devkit's depth writer            (the inverse of datasets/utils.py:32-40 read_depth)
// Everything is f64 in the reference's operation order; this library is built with -ffp-contract=off and this file uses no
// fast-math, so `a * b + c` stays two roundings as in numpy.
//
// Summation order.  The result must not depend on where an image lies in its batch, and image n of a u16 batch starts at
// byte n*H*W*2, which is 16-byte aligned only when n*H*W is a multiple of 8.  So the work is divided by the pixel index
// inside the image, never by the address: pixels [8j, 8j+8) are "group j", a lane owns groups j0 + lane, + 256, ... of
// its block's contiguous range and adds a group's pixels in index order.  A group is fetched with aligned 16-byte loads
// whatever the image's start: the aligned vectors that cover it are loaded and the group's bytes are funnelled out with
// v_alignbyte_b32 (shift = start address mod 16, uniform per image).  The first and the last full group and the ragged
// tail are read one element at a time by fixed lanes of block 0, so that no vector load ever touches a byte outside
// [image start, image end).  Lanes -> wave (DPP) -> block (LDS) -> plain stores of every block's partials; a second
// launch adds them in block order and finalises.  No floating-point atomics: the same bits for any run and any grouping.
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

constexpr int NACC = 10;          // nine sums and the pixel count
constexpr int PIX = 8;            // pixels per group
constexpr int MAX_BLOCKS = 64;    // per image

// blocks per image: a function of H*W alone (one block per 8192 pixels = four rounds of 256 lanes x 8 pixels)
inline int blocks_per_image(long hw) { return (int)std::max<long>(1, std::min<long>((hw + 8191) / 8192, MAX_BLOCKS)); }

struct Acc {
  double s[NACC - 1];
  int n;
};

// one pixel of compute_errors (:28-59); p, g already divided by the scale
__device__ __forceinline__ void add_pixel(Acc& a, double p, double g) {
  if (!(g > 0.01)) return;
  const double d = fabs(p - g), d2 = d * d;
  const double di = fabs(1.0 / g - 1.0 / p), di2 = di * di;
  const double lp = log(p), lg = log(g);
  const double dl = fabs(lp - lg), dl2 = dl * dl;
  a.s[0] += d;
  a.s[1] += d2;
  a.s[2] += di;
  a.s[3] += di2;
  a.s[4] += dl;
  a.s[5] += dl2;
  a.s[6] += lg - lp;
  a.s[7] += d / g;
  a.s[8] += d2 / (g * g);
  a.n += 1;
}

template <typename T> __device__ __forceinline__ double widen(T v, double scale);
template <> __device__ __forceinline__ double widen<uint16_t>(uint16_t v, double scale) { return (double)v / scale; }
template <> __device__ __forceinline__ double widen<float>(float v, double) { return (double)v; }

// o[i] = dword i of the byte string that starts DS dwords + bs bytes into d[]
template <int DS, int NO> __device__ __forceinline__ void funnel(const uint32_t* d, unsigned bs, uint32_t* o) {
#pragma unroll
  for (int i = 0; i < NO; ++i) o[i] = __builtin_amdgcn_alignbyte(d[DS + i + 1], d[DS + i], bs);
}

// The PIX elements of type T at `p` (aligned to sizeof(T) only) as NO = PIX*sizeof(T)/4 dwords, from NO/4 + 1 aligned
// 16-byte loads.  r = p mod 16, the same for every group of an image.  Reads [p - r, p - r + 4*NO + 16): the caller keeps
// one whole group of the same image on either side of every group it passes.
template <typename T> __device__ __forceinline__ void load_group(const T* p, unsigned r, uint32_t* o) {
  constexpr int NO = PIX * (int)sizeof(T) / 4, NV = NO / 4 + 1;
  const uint4* v = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p) - r);
  uint32_t d[NV * 4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const uint4 t = v[i];
    d[4 * i] = t.x; d[4 * i + 1] = t.y; d[4 * i + 2] = t.z; d[4 * i + 3] = t.w;
  }
  const unsigned bs = r & 3u;
  switch (r >> 2) {          // uniform; constant register indices in every arm
    case 0: funnel<0, NO>(d, bs, o); break;
    case 1: funnel<1, NO>(d, bs, o); break;
    case 2: funnel<2, NO>(d, bs, o); break;
    default: funnel<3, NO>(d, bs, o); break;
  }
}

template <typename T> __device__ __forceinline__ T element(const uint32_t* o, int i);
template <> __device__ __forceinline__ uint16_t element<uint16_t>(const uint32_t* o, int i) {
  return (uint16_t)(o[i >> 1] >> ((i & 1) * 16));
}
template <> __device__ __forceinline__ float element<float>(const uint32_t* o, int i) { return __uint_as_float(o[i]); }

// grid (blocks_per_image(H*W), N), 256 threads.  part[n][block][NACC]
template <typename TP, typename TG>
__global__ __launch_bounds__(256) void errors9_partial_kernel(const TP* __restrict__ pred, const TG* __restrict__ gt,
                                                              double scale, long hw, double* __restrict__ part) {
  __shared__ double sh[4][NACC];
  const int n = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  const TP* p0 = pred + (long)n * hw;
  const TG* g0 = gt + (long)n * hw;
  Acc a;
#pragma unroll
  for (int j = 0; j < NACC - 1; ++j) a.s[j] = 0.0;
  a.n = 0;

  const long ngroups = hw / PIX;                       // full groups; 0 and ngroups-1 are read by element below
  if (b == 0) {
    const long head = hw < PIX ? hw : PIX;
    const long tail0 = ngroups >= 2 ? (ngroups - 1) * PIX : head;      // [tail0, hw): at most 15 pixels
    long i = threadIdx.x;
    if (i >= head) i = tail0 + (i - head);
    if (i < hw) add_pixel(a, widen<TP>(p0[i], scale), widen<TG>(g0[i], scale));
  }
  const long body = ngroups > 2 ? ngroups - 2 : 0;     // groups 1 .. ngroups-2
  const long per = (body + nb - 1) / nb;
  const long j1 = std::min<long>(body, (long)(b + 1) * per) + 1;
  const unsigned rp = (unsigned)(reinterpret_cast<uintptr_t>(p0) & 15u);
  const unsigned rg = (unsigned)(reinterpret_cast<uintptr_t>(g0) & 15u);
  for (long j = (long)b * per + 1 + threadIdx.x; j < j1; j += 256) {
    uint32_t wp[PIX * sizeof(TP) / 4], wg[PIX * sizeof(TG) / 4];
    load_group<TP>(p0 + j * PIX, rp, wp);
    load_group<TG>(g0 + j * PIX, rg, wg);
#pragma unroll
    for (int k = 0; k < PIX; ++k)
      add_pixel(a, widen<TP>(element<TP>(wp, k), scale), widen<TG>(element<TG>(wg, k), scale));
  }

  double tot[NACC];
#pragma unroll
  for (int j = 0; j < NACC - 1; ++j) tot[j] = wave_sum_d(a.s[j]);
  tot[NACC - 1] = wave_sum_d((double)a.n);             // exact: at most 2^31 ones
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NACC; ++j) sh[threadIdx.x >> 6][j] = tot[j];
  }
  __syncthreads();
  if (threadIdx.x < NACC)
    part[((long)n * nb + b) * NACC + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// grid N, 64 threads: the blocks' partials in block order, then :60-80
__global__ __launch_bounds__(64) void errors9_finalize_kernel(const double* __restrict__ part, int nb,
                                                              double* __restrict__ out) {
  __shared__ double acc[NACC];
  const int n = blockIdx.x;
  if (threadIdx.x < NACC) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[((long)n * nb + b) * NACC + threadIdx.x];
    acc[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* o = out + (long)n * NACC;
  const double num = acc[9];
  if (num == 0.0) {          // the reference divides by zero here; the host side raises
    for (int j = 0; j < NACC; ++j) o[j] = 0.0;
    return;
  }
  o[0] = acc[0] / num;
  o[1] = sqrt(acc[1] / num);
  o[2] = acc[2] / num;
  o[3] = sqrt(acc[3] / num);
  o[4] = acc[4] / num;
  const double nsl = acc[5] / num;
  o[5] = sqrt(nsl);
  o[6] = sqrt(nsl - (acc[6] * acc[6]) / (num * num));
  o[7] = acc[7] / num;
  o[8] = acc[8] / num;
  o[9] = num;
}

// trunc(depth * scale) saturated to [0, 65535], NaN -> 0 (the comparisons are false for NaN)
__device__ __forceinline__ uint32_t quantize(float d, float scale) {
  const float v = d * scale;
  return v >= 65535.0f ? 65535u : (v >= 1.0f ? (uint32_t)v : 0u);
}

__global__ __launch_bounds__(256) void quantize_u16_kernel(const float* __restrict__ depth, uint16_t* __restrict__ out,
                                                           float scale, long total, long nvec) {
  const long stride = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  for (long i = t; i < nvec; i += stride) {
    const float4 d = reinterpret_cast<const float4*>(depth)[i];
    uint2 q;
    q.x = quantize(d.x, scale) | (quantize(d.y, scale) << 16);
    q.y = quantize(d.z, scale) | (quantize(d.w, scale) << 16);
    reinterpret_cast<uint2*>(out)[i] = q;
  }
  for (long i = nvec * 4 + t; i < total; i += stride) out[i] = (uint16_t)quantize(depth[i], scale);
}

template <typename TP, typename TG>
void launch_errors9(const void* pred, const void* gt, double scale, int N, long hw, int nb, double* part, hipStream_t st) {
  hipLaunchKernelGGL((errors9_partial_kernel<TP, TG>), dim3(nb, N), dim3(256), 0, st, static_cast<const TP*>(pred),
                     static_cast<const TG*>(gt), scale, hw, part);
}

}  // namespace

extern "C" int64_t fs_depth_errors9_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1 || N > 65535 || (int64_t)H * W >= (int64_t)1 << 31) return -1;
  return (int64_t)N * blocks_per_image((long)H * W) * NACC * (int64_t)sizeof(double);
}

extern "C" int fs_depth_errors9(const void* pred, const void* gt, int pred_is_u16, int gt_is_u16, double scale, int N,
                                int H, int W, void* workspace, int64_t workspace_bytes, double* out, void* stream) {
  const int64_t need = fs_depth_errors9_workspace_bytes(N, H, W);
  if (!pred || !gt || !workspace || !out || need < 0 || !(scale > 0.0) || workspace_bytes < need ||
      (reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(pred) & (pred_is_u16 ? 1 : 3)) ||
      (reinterpret_cast<uintptr_t>(gt) & (gt_is_u16 ? 1 : 3)))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long hw = (long)H * W;
  const int nb = blocks_per_image(hw);
  double* part = static_cast<double*>(workspace);
  if (pred_is_u16 && gt_is_u16) launch_errors9<uint16_t, uint16_t>(pred, gt, scale, N, hw, nb, part, st);
  else if (pred_is_u16) launch_errors9<uint16_t, float>(pred, gt, scale, N, hw, nb, part, st);
  else if (gt_is_u16) launch_errors9<float, uint16_t>(pred, gt, scale, N, hw, nb, part, st);
  else launch_errors9<float, float>(pred, gt, scale, N, hw, nb, part, st);
  hipLaunchKernelGGL(errors9_finalize_kernel, dim3(N), dim3(64), 0, st, part, nb, out);
  return fs_launch_status();
}

extern "C" int fs_depth_quantize_u16(const float* depth, void* out, float scale, int H, int W, void* stream) {
  if (!depth || !out || H < 1 || W < 1 || !(scale > 0.0f) || (reinterpret_cast<uintptr_t>(depth) & 3) ||
      (reinterpret_cast<uintptr_t>(out) & 1))
    return FS_EINVAL;
  const long total = (long)H * W;
  const bool vec = !(reinterpret_cast<uintptr_t>(depth) & 15) && !(reinterpret_cast<uintptr_t>(out) & 7);
  const long nvec = vec ? total / 4 : 0;
  const unsigned blocks = (unsigned)std::max<long>(1, std::min<long>((total / 4 + 255) / 256, 2048));
  hipLaunchKernelGGL(quantize_u16_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth,
                     static_cast<uint16_t*>(out), scale, total, nvec);
  return fs_launch_status();
}
