// LiDAR ground truth through pinhole cameras on the device: the KITTI / KITTI-360 export (float32 metres) and the
// nuScenes export (one sweep through C cameras, the uint16 PNG plane).  One kernel set; a rule per export says which
// points survive and what value a point carries.
// Per map (frame g, or sample g and camera c) with its matrix M [3, 4]: p_k = m_k0 x + m_k1 y + m_k2 z + m_k3 in f64,
// added in that order (the library is compiled with -ffp-contract=off: no FMA); u = p0 / p2, v = p1 / p2;
// col = rint(u) - 1, row = rint(v) - 1 (np.round: half to even); keep 0 <= col < W, 0 <= row < H.  A zero or NaN p2
// only fails these range tests.  A pixel takes the value of its last point in scan order (numpy's fancy assignment);
// then, for every group of more than one point sharing the export index row * (W - 1) + col - 1, the pixel of the
// group's FIRST point takes the group's minimum.  0 where no point lands.
//
// Edge pairs.  That index is not injective: (r, W-1) and (r+1, 0) share one, and no other pair of pixels does (W >= 2;
// W = 1 would put the whole image in one group and is refused).  So a group is one pixel, or such an edge pair; the
// second pixel of a pair keeps its last writer.
//
// Slots.  G * C maps per call, three launches.
//   init     one 16-byte slot per pixel: { last = 0, first = 0xffffffff, min = 0xffffffff }
//   scatter  grid (blocks, G * C): the map is uniform per block, so its 12 matrix entries and its two offsets come
//            through scalar loads; one thread per point, the point read as one float4 (the C cameras of a sample read
//            the same points).  Three no-return integer atomics into the pixel's slot (one 64-byte line): u64 max of
//            ((scan index + 1) << 32 | value bits) = the last point with its value, u32 min of the scan index = the
//            first point, u32 min of the value bits = the smallest value.  The scan index is the point's index in its
//            scan: a rule's filter keeps the order.  A rule's value bits must order like the values.
//   gather   one thread per pixel: its slot and, for an edge pixel, the neighbouring slot of its partner (flat index
//            +-1); more than one point in the group <=> first != last in this pixel, or the partner is hit at all.
//
// Determinism.  Integer max / min do not depend on the order in which points arrive: the maps are the same bit for bit
// on every run, for any grouping of frames into calls and under graph replay.  No floating-point atomics, no host sync.
//
// Replaces (reference):
//   KittiRule   project_depth_map (Kitti360Evaluator._precompute)      monodepth/networks/utils/monodepth_utils.py:422-458
//               generate_depth_map(vel_depth=True), the same arithmetic  monodepth_utils.py:386-420
//               sub2ind                                                  monodepth_utils.py:291-295
//   NuscRule    generate_depth_map                   monodepth/evaluation/nuscenes_unsupervised_eval.py:85-126
//               (depth * 256).astype(np.uint16)      nuscenes_unsupervised_eval.py:198
//               sub2ind                              nuscenes_unsupervised_eval.py:79-83
//               M = rows 0..2 of homo_intrinsics @ inv(extrinsics); row 3 of the reference's 4x4 product never reaches
//               the result.
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

struct __attribute__((aligned(16))) Slot {
  unsigned long long last;   // (scan index + 1) << 32 | value bits of the last point; 0 = no point
  unsigned int first;        // scan index of the first point
  unsigned int vmin;         // smallest value bits
};
static_assert(sizeof(Slot) == 16, "one 16-byte slot per pixel");

// KITTI: keep the points with float32 x >= 0, before the projection; there is no test on p2.  The value is the float32
// x.  The kept values are >= 0, so their bit patterns order like the values — except x = -0.0, which passes x >= 0 with
// the sign bit set and would order above everything.  Its sign bit is cleared: -0.0 is treated as +0.0 throughout.  The
// reference may write either zero there; the two compare equal and the metric's gt > 1e-3 drops both.
struct KittiRule {
  static constexpr bool one_camera = true;             // map g reads scan g: no division by C
  static __device__ __forceinline__ bool keep_point(const float4& p) { return p.x >= 0.f; }
  static __device__ __forceinline__ bool keep_depth(double) { return true; }
  static __device__ __forceinline__ unsigned int value(const float4& p, double) {
    return __float_as_uint(p.x) & 0x7fffffffu;
  }
};

// nuScenes: keep the point iff p2 > 0 (a NaN fails).  The value is q = min(trunc(p2 * 256.0), 65535) in f64: the uint16
// the reference's cast makes of a depth below 256 m (p2 > 0: q >= 0; inf -> 65535).  Beyond that the reference's cast
// wraps; this saturates (the sensor does not reach that range).  Quantising per point is exact: trunc(. * 256) and the
// saturation are monotone, so min-then-quantise equals quantise-then-min, and a last writer's value is quantised alone
// either way.
struct NuscRule {
  static constexpr bool one_camera = false;
  static __device__ __forceinline__ bool keep_point(const float4&) { return true; }
  static __device__ __forceinline__ bool keep_depth(double p2) { return p2 > 0.0; }
  static __device__ __forceinline__ unsigned int value(const float4&, double p2) {
    return (unsigned int)fmin(trunc(p2 * 256.0), 65535.0);
  }
};

__device__ __forceinline__ void store_bits(float* out, unsigned int bits) { *out = __uint_as_float(bits); }
__device__ __forceinline__ void store_bits(unsigned short* out, unsigned int bits) { *out = (unsigned short)bits; }

__global__ __launch_bounds__(256) void slot_init_kernel(uint4* __restrict__ slots, long n) {
  const uint4 empty = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) slots[i] = empty;
}

template <class Rule>
__global__ __launch_bounds__(256) void scatter_kernel(const float4* __restrict__ points,
                                                      const int64_t* __restrict__ offsets, long n_points,
                                                      const double* __restrict__ Ms, int C, int H, int W,
                                                      Slot* __restrict__ slots) {
  const int gc = blockIdx.y, g = Rule::one_camera ? gc : gc / C;
  const long begin = std::max<long>(offsets[g], 0), end = std::min<long>(offsets[g + 1], n_points);
  if (end - begin > 0x7fffffffL) return;
  const double* __restrict__ M = Ms + (long)gc * 12;
  const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5], m6 = M[6], m7 = M[7], m8 = M[8],
               m9 = M[9], m10 = M[10], m11 = M[11];
  Slot* __restrict__ frame = slots + (long)gc * H * W;
  for (long i = begin + (long)blockIdx.x * 256 + threadIdx.x; i < end; i += (long)gridDim.x * 256) {
    const float4 p = points[i];
    if (!Rule::keep_point(p)) continue;
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double p0 = m0 * x + m1 * y + m2 * z + m3;
    const double p1 = m4 * x + m5 * y + m6 * z + m7;
    const double p2 = m8 * x + m9 * y + m10 * z + m11;
    if (!Rule::keep_depth(p2)) continue;
    const double col = rint(p0 / p2) - 1.0, row = rint(p1 / p2) - 1.0;
    if (!(col >= 0.0 && col < (double)W && row >= 0.0 && row < (double)H)) continue;   // NaN and inf fail here
    const unsigned int local = (unsigned int)(i - begin);
    const unsigned int bits = Rule::value(p, p2);
    Slot* s = frame + (long)(int)row * W + (int)col;
    atomicMax(&s->last, ((unsigned long long)(local + 1u) << 32) | bits);
    atomicMin(&s->first, local);
    atomicMin(&s->vmin, bits);
  }
}

template <class Out>
__global__ __launch_bounds__(256) void gather_kernel(const uint4* __restrict__ slots, long maps, int H, int W,
                                                     Out* __restrict__ depth) {
  const long HW = (long)H * W, total = maps * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const uint4 a = slots[i];                           // x, y = last (low, high), z = first, w = min
    unsigned int bits = 0u;
    if (a.y != 0u) {
      bits = a.x;
      const long pix = i % HW;
      const int r = (int)(pix / W), c = (int)(pix - (long)r * W);
      uint4 b = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
      if (c == W - 1 && r + 1 < H) b = slots[i + 1];    // (r + 1, 0)
      else if (c == 0 && r > 0) b = slots[i - 1];       // (r - 1, W - 1)
      const bool many = a.z != a.y - 1u || b.y != 0u;   // two points here, or one here and one on the partner
      if (many && a.z < b.z) bits = std::min(a.w, b.w); // this pixel holds the group's first point
    }
    store_bits(depth + i, bits);
  }
}

unsigned grid_for(long n, long cap) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

int64_t slot_bytes(int G, int C, int H, int W) {
  if (G < 1 || C < 1 || H < 1 || W < 2 || (int64_t)G * C > 65535 || (int64_t)G * C * H * W >= (int64_t)1 << 31)
    return -1;
  return (int64_t)G * C * H * W * (int64_t)sizeof(Slot);
}

template <class Rule, class Out>
int lidar_depth(const float* points, const int64_t* offsets, int64_t n_points, const double* M, int G, int C, int H,
                int W, Out* depth, void* workspace, int64_t have, void* stream) {
  const int64_t need = slot_bytes(G, C, H, W);
  if (!offsets || !M || !depth || !workspace || need < 0 || n_points < 0 || (n_points > 0 && !points) || have < need ||
      (reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(points) & 15) ||
      (sizeof(Out) == 2 && (reinterpret_cast<uintptr_t>(depth) & 1)))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long maps = (long)G * C, total = maps * H * W;
  hipLaunchKernelGGL(slot_init_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st, static_cast<uint4*>(workspace),
                     total);
  if (n_points > 0)
    hipLaunchKernelGGL(scatter_kernel<Rule>, dim3(grid_for((n_points + G - 1) / G, 2048), (unsigned)maps), dim3(256), 0,
                       st, reinterpret_cast<const float4*>(points), offsets, (long)n_points, M, C, H, W,
                       static_cast<Slot*>(workspace));
  hipLaunchKernelGGL(gather_kernel<Out>, dim3(grid_for(total, 8192)), dim3(256), 0, st,
                     static_cast<const uint4*>(workspace), maps, H, W, depth);
  return fs_launch_status();
}

}  // namespace

extern "C" int64_t fs_lidar_pinhole_depth_workspace_bytes(int G, int H, int W) { return slot_bytes(G, 1, H, W); }

extern "C" int64_t fs_lidar_nusc_depth_workspace_bytes(int G, int C, int H, int W) {
  return slot_bytes(G, C, H, W);
}

extern "C" int fs_lidar_pinhole_depth(const float* points, const int64_t* offsets, int64_t n_points, const double* P,
                                      int G, int H, int W, float* depth, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  return lidar_depth<KittiRule>(points, offsets, n_points, P, G, 1, H, W, depth, workspace, workspace_bytes, stream);
}

extern "C" int fs_lidar_nusc_depth_u16(const float* points, const int64_t* offsets, int64_t n_points, const double* M,
                                       int G, int C, int H, int W, void* depth_u16, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return lidar_depth<NuscRule>(points, offsets, n_points, M, G, C, H, W, static_cast<unsigned short*>(depth_u16),
                               workspace, workspace_bytes, stream);
}
