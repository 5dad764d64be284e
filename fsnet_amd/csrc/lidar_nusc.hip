// LiDAR ground truth of the nuScenes evaluation: one sweep through C cameras, exported as the uint16 PNG plane.
// Replaces (reference):
//   generate_depth_map                         monodepth/evaluation/nuscenes_unsupervised_eval.py:85-126
//   (depth * 256).astype(np.uint16)            nuscenes_unsupervised_eval.py:198
//   sub2ind                                    nuscenes_unsupervised_eval.py:79-83
// Per sample g and camera c, with M = rows 0..2 of homo_intrinsics @ inv(extrinsics) (row 3 of the reference's 4x4
// product never reaches the result): p_k = m_k0 x + m_k1 y + m_k2 z + m_k3 in f64, added in that order (the library is
// compiled with -ffp-contract=off: no FMA); keep the point iff p2 > 0 (a NaN fails); col = rint(p0 / p2) - 1,
// row = rint(p1 / p2) - 1 (np.round: half to even); keep 0 <= col < W, 0 <= row < H.  The value of a point is
// q = min(trunc(p2 * 256.0), 65535) in f64: the uint16 the reference's cast makes of a depth below 256 m.  Beyond that
// the reference's cast wraps; this kernel saturates (the sensor does not reach that range).  Quantising per point is
// exact: trunc(. * 256) and the saturation are monotone, so min-then-quantise equals quantise-then-min, and a last
// writer's value is quantised alone either way.
// A pixel takes the q of its last kept point in scan order; then, for every group of more than one point sharing the
// export index row * (W - 1) + col - 1 (one pixel, or the pair (r, W-1) / (r+1, 0); W >= 2), the pixel of the group's
// FIRST point takes the group's minimum q.  0 where no point lands.
//
// G samples x C cameras per call, three launches, the slot and the integer-atomic argument of lidar_pinhole.hip:
//   init     one 16-byte slot per pixel: { last = 0, first = 0xffffffff, min = 0xffffffff }
//   scatter  grid (blocks, G * C): sample and camera are uniform per block, so the 12 matrix entries and the two offsets
//            are the same for every lane; one thread per point, the point read as one float4 (the C cameras of a
//            sample read the same points).  u64 max of ((scan index + 1) << 32 | q), u32 min of the scan index, u32
//            min of q.  The scan index is the point's index in its sample: the p2 > 0 filter keeps the order.
//   gather   one thread per pixel: its slot and, for an edge pixel, the slot of its partner (flat index +-1).
// Integer max / min do not depend on the order in which points arrive: the same bits on every run, for any grouping of
// samples into calls and under graph replay.  No floating-point atomics, no host sync.
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

struct __attribute__((aligned(16))) Slot {
  unsigned long long last;   // (scan index + 1) << 32 | q of the last point; 0 = no point
  unsigned int first;        // scan index of the first point
  unsigned int vmin;         // smallest q
};
static_assert(sizeof(Slot) == 16, "one 16-byte slot per pixel");

__global__ __launch_bounds__(256) void nusc_slot_init_kernel(uint4* __restrict__ slots, long n) {
  const uint4 empty = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) slots[i] = empty;
}

__global__ __launch_bounds__(256) void nusc_scatter_kernel(const float4* __restrict__ points,
                                                           const int64_t* __restrict__ offsets, long n_points,
                                                           const double* __restrict__ Ms, int C, int H, int W,
                                                           Slot* __restrict__ slots) {
  const int gc = blockIdx.y, g = gc / C;
  const long begin = std::max<long>(offsets[g], 0), end = std::min<long>(offsets[g + 1], n_points);
  if (end - begin > 0x7fffffffL) return;
  const double* __restrict__ M = Ms + (long)gc * 12;
  const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5], m6 = M[6], m7 = M[7], m8 = M[8],
               m9 = M[9], m10 = M[10], m11 = M[11];
  Slot* __restrict__ frame = slots + (long)gc * H * W;
  for (long i = begin + (long)blockIdx.x * 256 + threadIdx.x; i < end; i += (long)gridDim.x * 256) {
    const float4 p = points[i];
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double p0 = m0 * x + m1 * y + m2 * z + m3;
    const double p1 = m4 * x + m5 * y + m6 * z + m7;
    const double p2 = m8 * x + m9 * y + m10 * z + m11;
    if (!(p2 > 0.0)) continue;                                                         // NaN fails
    const double col = rint(p0 / p2) - 1.0, row = rint(p1 / p2) - 1.0;
    if (!(col >= 0.0 && col < (double)W && row >= 0.0 && row < (double)H)) continue;   // NaN and inf fail here
    const unsigned int local = (unsigned int)(i - begin);
    const unsigned int q = (unsigned int)fmin(trunc(p2 * 256.0), 65535.0);             // p2 > 0: q >= 0; inf -> 65535
    Slot* s = frame + (long)(int)row * W + (int)col;
    atomicMax(&s->last, ((unsigned long long)(local + 1u) << 32) | q);
    atomicMin(&s->first, local);
    atomicMin(&s->vmin, q);
  }
}

__global__ __launch_bounds__(256) void nusc_gather_kernel(const uint4* __restrict__ slots, long maps, int H, int W,
                                                          unsigned short* __restrict__ depth) {
  const long HW = (long)H * W, total = maps * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const uint4 a = slots[i];                           // x, y = last (low, high), z = first, w = min
    unsigned int q = 0u;
    if (a.y != 0u) {
      q = a.x;
      const long pix = i % HW;
      const int r = (int)(pix / W), c = (int)(pix - (long)r * W);
      uint4 b = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
      if (c == W - 1 && r + 1 < H) b = slots[i + 1];    // (r + 1, 0)
      else if (c == 0 && r > 0) b = slots[i - 1];       // (r - 1, W - 1)
      const bool many = a.z != a.y - 1u || b.y != 0u;   // two points here, or one here and one on the partner
      if (many && a.z < b.z) q = std::min(a.w, b.w);    // this pixel holds the group's first point
    }
    depth[i] = (unsigned short)q;
  }
}

unsigned grid_for(long n, long cap) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

}  // namespace

extern "C" int64_t fs_lidar_nusc_depth_workspace_bytes(int G, int C, int H, int W) {
  if (G < 1 || C < 1 || H < 1 || W < 2 || (int64_t)G * C > 65535 || (int64_t)G * C * H * W >= (int64_t)1 << 31)
    return -1;
  return (int64_t)G * C * H * W * (int64_t)sizeof(Slot);
}

extern "C" int fs_lidar_nusc_depth_u16(const float* points, const int64_t* offsets, int64_t n_points, const double* M,
                                       int G, int C, int H, int W, void* depth_u16, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  const int64_t need = fs_lidar_nusc_depth_workspace_bytes(G, C, H, W);
  if (!offsets || !M || !depth_u16 || !workspace || need < 0 || n_points < 0 || (n_points > 0 && !points) ||
      workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
      (reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(depth_u16) & 1))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long maps = (long)G * C, total = maps * H * W;
  hipLaunchKernelGGL(nusc_slot_init_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st,
                     static_cast<uint4*>(workspace), total);
  if (n_points > 0)
    hipLaunchKernelGGL(nusc_scatter_kernel, dim3(grid_for((n_points + G - 1) / G, 2048), (unsigned)maps), dim3(256), 0,
                       st, reinterpret_cast<const float4*>(points), offsets, (long)n_points, M, C, H, W,
                       static_cast<Slot*>(workspace));
  hipLaunchKernelGGL(nusc_gather_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st,
                     static_cast<const uint4*>(workspace), maps, H, W, static_cast<unsigned short*>(depth_u16));
  return fs_launch_status();
}
