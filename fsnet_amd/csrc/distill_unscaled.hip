// Scale-aligned self-distillation: compute_distill_loss with is_unscaled_distill = True
//   ratio = (pred / (teacher + 1e-5)).mean(dim=[2, 3]);  error = |ratio * teacher - pred|
//                                                        monodepth/networks/models/heads/monodepth2_decoder.py:185-203
// forward and backward for one to four scales per launch.  Every sample plane (b, c) of n = h*w elements
// is cut into chunks of DU_CHUNK elements, one block each.  Three passes over the data:
//   ratio pass     per-block f64 partial of  sum p / (t + 1e-5)                         -> workspace R[plane][chunk]
//   loss pass      per-block f64 partials of the loss sum and of G = sum w s t          -> workspace L, G
//   backward pass  d_pred = k (-w s + (G / n) / (t + 1e-5)),  d_uncertain as in distill.hip
// and a one-block kernel behind the loss pass that adds each scale's L partials in index order.  A block rebuilds its
// plane's ratio (and G) from the partials in index order, so every block of a plane holds the same bits; no
// floating-point atomics anywhere, and a thread owns the same elements whether or not its addresses allow 16-byte
// accesses: results do not depend on alignment.
#include "common.h"
#include "fsnet_hip_internal.h"

namespace {

constexpr int DU_CHUNK = 2048;                  // elements of a plane per block: 256 threads x 2 groups of 4

// launch geometry derived on the host from (planes, n[], S)
struct DuPlan {
  long n[4];
  long woff[4];        // first double of scale s in the workspace: R, then L, then G, [planes][chunks[s]] each
  int chunks[4];
  int bstart[5];       // first block of scale s
  int planes, S;
};

struct DuBlock {
  int s, plane, chunk;
  long n, base;        // elements of the plane; first element of this block in the tensor
  int count;           // elements of this block, 1..DU_CHUNK
  long cells;          // planes * chunks[s]
  const double* ws;    // scale s of the workspace
};

__device__ inline DuBlock du_block(const DuPlan& pl, const double* ws) {
  DuBlock b;
  int s = 0;
  while (s + 1 < pl.S && (int)blockIdx.x >= pl.bstart[s + 1]) ++s;
  const int r = (int)blockIdx.x - pl.bstart[s];
  b.s = s;
  b.plane = r / pl.chunks[s];
  b.chunk = r - b.plane * pl.chunks[s];
  b.n = pl.n[s];
  const long first = (long)b.chunk * DU_CHUNK;
  b.base = (long)b.plane * b.n + first;
  b.count = (int)(b.n - first < (long)DU_CHUNK ? b.n - first : (long)DU_CHUNK);
  b.cells = (long)pl.planes * pl.chunks[s];
  b.ws = ws + pl.woff[s];
  return b;
}

// sum of one plane's partials in index order (uniform across the block: scalar loads)
__device__ inline double du_plane_sum(const double* part, int plane, int chunks) {
  const double* p = part + (long)plane * chunks;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc += p[c];
  return acc;
}

__device__ inline bool du_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements [i, i + 4) of a block's `count`: one 16-byte load where the address allows and all four exist
__device__ inline void du_load4(const float* p, int i, int count, bool wide, float v[4]) {
  if (wide && i + 4 <= count) {
    load4<float>(p + i, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < count ? p[i + k] : 0.f;
  }
}
__device__ inline void du_store4(float* p, int i, int count, bool wide, const float v[4]) {
  if (wide && i + 4 <= count) {
    store4<float>(p + i, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < count) p[i + k] = v[k];
  }
}

__device__ inline float du_ratio(const DuBlock& b, int chunks) {
  return (float)(du_plane_sum(b.ws, b.plane, chunks) / (double)b.n);     // rounded to fp32 once, here
}

__global__ __launch_bounds__(256) void distill_unscaled_ratio_kernel(FsDistillUnscaledArgs a, DuPlan pl) {
  const DuBlock b = du_block(pl, (const double*)a.workspace);
  const float* p = a.pred[b.s] + b.base;
  const float* t = a.teacher[b.s] + b.base;
  const bool wide = du_aligned16(p) && du_aligned16(t);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < DU_CHUNK / 1024; ++j) {
    const int i = (j * 256 + (int)threadIdx.x) * 4;
    if (i >= b.count) continue;
    float pv[4], tv[4];
    du_load4(p, i, b.count, wide, pv);
    du_load4(t, i, b.count, wide, tv);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < b.count) acc += (double)(pv[k] / (tv[k] + 1e-5f));
  }
  __shared__ double sh[4];
  acc = block_sum_d(acc, sh);
  if (threadIdx.x == 0) ((double*)a.workspace)[pl.woff[b.s] + (long)b.plane * pl.chunks[b.s] + b.chunk] = acc;
}

template <bool UNC>
__global__ __launch_bounds__(256) void distill_unscaled_loss_kernel(FsDistillUnscaledArgs a, DuPlan pl) {
  const DuBlock b = du_block(pl, (const double*)a.workspace);
  const float ratio = du_ratio(b, pl.chunks[b.s]);
  const float* p = a.pred[b.s] + b.base;
  const float* t = a.teacher[b.s] + b.base;
  const float* u = UNC ? a.uncertain[b.s] + b.base : nullptr;
  const bool wide = du_aligned16(p) && du_aligned16(t) && (!UNC || du_aligned16(u));
  double accl = 0.0, accg = 0.0;
#pragma unroll
  for (int j = 0; j < DU_CHUNK / 1024; ++j) {
    const int i = (j * 256 + (int)threadIdx.x) * 4;
    if (i >= b.count) continue;
    float pv[4], tv[4], uv[4];
    du_load4(p, i, b.count, wide, pv);
    du_load4(t, i, b.count, wide, tv);
    if (UNC) du_load4(u, i, b.count, wide, uv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k >= b.count) continue;
      const float x = __fsub_rn(__fmul_rn(ratio, tv[k]), pv[k]);        // never fused: the sign of x is the gradient
      const float e = fabsf(x);
      const float st = x > 0.f ? tv[k] : (x < 0.f ? -tv[k] : 0.f);      // s t
      if (UNC) {
        accl += (double)(e / uv[k] + logf(uv[k] + 1e-5f));
        accg += (double)(st / uv[k]);
      } else {
        accl += (double)e;
        accg += (double)st;
      }
    }
  }
  __shared__ double shl[4], shg[4];
  accl = block_sum_d(accl, shl);
  accg = block_sum_d(accg, shg);
  if (threadIdx.x == 0) {
    double* w = (double*)a.workspace + pl.woff[b.s] + (long)b.plane * pl.chunks[b.s] + b.chunk;
    w[b.cells] = accl;
    w[2 * b.cells] = accg;
  }
}

// loss_out[s] = (sum of scale s's loss partials, thread-strided then block-wide: one fixed order) / (planes n)
__global__ __launch_bounds__(256) void distill_unscaled_finish_kernel(FsDistillUnscaledArgs a, DuPlan pl) {
  __shared__ double sh[4];
  for (int s = 0; s < pl.S; ++s) {
    const long cells = (long)pl.planes * pl.chunks[s];
    const double* part = (const double*)a.workspace + pl.woff[s] + cells;
    double acc = 0.0;
    for (long i = threadIdx.x; i < cells; i += 256) acc += part[i];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) a.loss_out[s] = acc / ((double)pl.planes * (double)pl.n[s]);
  }
}

template <bool UNC>
__global__ __launch_bounds__(256) void distill_unscaled_bwd_kernel(FsDistillUnscaledArgs a, DuPlan pl) {
  const DuBlock b = du_block(pl, (const double*)a.workspace);
  const int chunks = pl.chunks[b.s];
  const float ratio = du_ratio(b, chunks);
  const float gn = (float)(du_plane_sum(b.ws + 2 * b.cells, b.plane, chunks) / (double)b.n);     // G / n
  const float kk = (float)((a.gout ? a.gout[b.s] : 1.0) / ((double)pl.planes * (double)b.n));
  const float* p = a.pred[b.s] + b.base;
  const float* t = a.teacher[b.s] + b.base;
  const float* u = UNC ? a.uncertain[b.s] + b.base : nullptr;
  float* dp = a.d_pred[b.s] + b.base;
  float* du = UNC ? a.d_uncertain[b.s] + b.base : nullptr;
  const bool wide = du_aligned16(p) && du_aligned16(t) && du_aligned16(dp) && (!UNC || (du_aligned16(u) && du_aligned16(du)));
#pragma unroll
  for (int j = 0; j < DU_CHUNK / 1024; ++j) {
    const int i = (j * 256 + (int)threadIdx.x) * 4;
    if (i >= b.count) continue;
    float pv[4], tv[4], uv[4], dpv[4], duv[4];
    du_load4(p, i, b.count, wide, pv);
    du_load4(t, i, b.count, wide, tv);
    if (UNC) du_load4(u, i, b.count, wide, uv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = __fsub_rn(__fmul_rn(ratio, tv[k]), pv[k]);
      const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);          // torch.abs backward: sign, 0 at 0
      const float through = gn / (tv[k] + 1e-5f);                       // the path through the plane's ratio
      if (UNC) {
        const float uu = uv[k];
        dpv[k] = (-sg / uu + through) * kk;
        duv[k] = (-fabsf(x) / (uu * uu) + 1.f / (uu + 1e-5f)) * kk;
      } else {
        dpv[k] = (-sg + through) * kk;
      }
    }
    du_store4(dp, i, b.count, wide, dpv);
    if (UNC) du_store4(du, i, b.count, wide, duv);
  }
}

// FS_OK and the plan, or FS_EINVAL
int du_plan(int planes, const int64_t* n, int S, DuPlan* pl) {
  if (!n || S < 1 || S > 4 || planes < 1) return FS_EINVAL;
  long blocks = 0, cells = 0;
  for (int s = 0; s < 4; ++s) { pl->n[s] = 0; pl->woff[s] = 0; pl->chunks[s] = 0; pl->bstart[s] = 0; }
  for (int s = 0; s < S; ++s) {
    if (n[s] < 1) return FS_EINVAL;
    const long chunks = (long)((n[s] + DU_CHUNK - 1) / DU_CHUNK);
    if (chunks > 0x7fffffffL / planes) return FS_EINVAL;
    pl->n[s] = (long)n[s];
    pl->chunks[s] = (int)chunks;
    pl->bstart[s] = (int)blocks;
    pl->woff[s] = 3 * cells;
    blocks += chunks * planes;
    cells += chunks * planes;
    if (blocks > 0x7fffffffL) return FS_EINVAL;
  }
  pl->bstart[S] = (int)blocks;
  for (int s = S + 1; s < 5; ++s) pl->bstart[s] = (int)blocks;
  pl->planes = planes;
  pl->S = S;
  return FS_OK;
}

// pointers both entry points need; `unc` = the uncertainty variant
int du_check(const FsDistillUnscaledArgs* a, DuPlan* pl, bool* unc) {
  if (!a || !a->workspace) return FS_EINVAL;
  if (du_plan(a->planes, a->n, a->S, pl) != FS_OK) return FS_EINVAL;
  int nu = 0;
  for (int s = 0; s < a->S; ++s) {
    if (!a->pred[s] || !a->teacher[s]) return FS_EINVAL;
    nu += a->uncertain[s] != nullptr;
  }
  if (nu != 0 && nu != a->S) return FS_EINVAL;
  *unc = nu != 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_distill_unscaled_chunk(void) { return DU_CHUNK; }

extern "C" int64_t fs_distill_unscaled_workspace_bytes(int planes, const int64_t* n, int S) {
  DuPlan pl;
  if (du_plan(planes, n, S, &pl) != FS_OK) return -1;
  return (int64_t)3 * (int64_t)pl.bstart[S] * (int64_t)sizeof(double);
}

extern "C" int fs_distill_unscaled_fwd(const FsDistillUnscaledArgs* a, void* stream) {
  DuPlan pl;
  bool unc;
  if (du_check(a, &pl, &unc) != FS_OK || !a->loss_out) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.bstart[pl.S]), block(256);
  hipLaunchKernelGGL(distill_unscaled_ratio_kernel, grid, block, 0, st, *a, pl);
  if (unc) hipLaunchKernelGGL(distill_unscaled_loss_kernel<true>, grid, block, 0, st, *a, pl);
  else hipLaunchKernelGGL(distill_unscaled_loss_kernel<false>, grid, block, 0, st, *a, pl);
  hipLaunchKernelGGL(distill_unscaled_finish_kernel, dim3(1), block, 0, st, *a, pl);
  return fs_launch_status();
}

extern "C" int fs_distill_unscaled_bwd(const FsDistillUnscaledArgs* a, void* stream) {
  DuPlan pl;
  bool unc;
  if (du_check(a, &pl, &unc) != FS_OK) return FS_EINVAL;
  int ndu = 0;
  for (int s = 0; s < a->S; ++s) {
    if (!a->d_pred[s]) return FS_EINVAL;
    ndu += a->d_uncertain[s] != nullptr;
  }
  if (ndu != (unc ? a->S : 0)) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.bstart[pl.S]), block(256);
  if (unc) hipLaunchKernelGGL(distill_unscaled_bwd_kernel<true>, grid, block, 0, st, *a, pl);
  else hipLaunchKernelGGL(distill_unscaled_bwd_kernel<false>, grid, block, 0, st, *a, pl);
  return fs_launch_status();
}
