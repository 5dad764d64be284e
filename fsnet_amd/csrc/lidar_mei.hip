// LiDAR ground truth of the KITTI-360 fisheye evaluation: every scan point carried into the left fisheye camera and
// projected through the Mei unified model, the last point (in scan order) per pixel kept.
// Replaces (reference):
//   T_velo2cam02 @ [velo, 1]^T, z > 0                     monodepth/evaluation/kitti360_fisheye_eval.py:122-125
//   MeiCameraProjection.cam2image -> _cam2image            monodepth/networks/utils/mei_fisheye_utils.py:23-51,135-137
//   _projection (numpy fancy assignment, last writer wins) kitti360_fisheye_eval.py:75-95
//   norm, close mask 0 < norm < 8, astype(float32)         kitti360_fisheye_eval.py:135-141
// G frames per call.  Pass 1, one thread per point: transform + project in f64 in _cam2image's operation order (the
// library is compiled with -ffp-contract=off: no FMA anywhere), then atomicMax of the point's scan index into an int32
// winner plane initialised to -1.  Pass 2, one thread per pixel: the winner's z (depth) and norm (close mask) are
// recomputed from its point.  atomicMax does not depend on the order in which points arrive, so the maps are the same
// bit for bit on every run and for any grouping of frames into calls.
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

struct CamPoint {
  double x, y, z;   // camera frame
};

__device__ __forceinline__ CamPoint to_camera(const float* __restrict__ p, const double* __restrict__ T) {
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  CamPoint c;
  c.x = T[0] * px + T[1] * py + T[2] * pz + T[3];
  c.y = T[4] * px + T[5] * py + T[6] * pz + T[7];
  c.z = T[8] * px + T[9] * py + T[10] * pz + T[11];
  return c;
}

// np.linalg.norm(points, axis=-1): sqrt((x^2 + y^2) + z^2)
__device__ __forceinline__ double cam_norm(const CamPoint& c) { return sqrt(c.x * c.x + c.y * c.y + c.z * c.z); }

// mei = gamma1, gamma2, u0, v0, k1, k2, xi
__device__ __forceinline__ void mei_project(const CamPoint& c, double norm, const double* __restrict__ mei, double& u,
                                            double& v) {
  const double eps = 1e-6;
  double x = c.x / (norm + eps);
  double y = c.y / (norm + eps);
  const double z = c.z / (norm + eps);
  x /= z + mei[6] + eps;
  y /= z + mei[6] + eps;
  const double ro2 = x * x + y * y;
  x = x * (1.0 + mei[4] * ro2 + mei[5] * ro2 * ro2);
  y = y * (1.0 + mei[4] * ro2 + mei[5] * ro2 * ro2);
  u = mei[0] * x + mei[2];
  v = mei[1] * y + mei[3];
}

__global__ __launch_bounds__(256) void winner_init_kernel(int* __restrict__ winner, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) winner[i] = -1;
}

// frame of global point i: the last g with offsets[g] <= i
__device__ __forceinline__ int frame_of(const int64_t* __restrict__ offsets, int G, long i) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void lidar_scatter_kernel(const float* __restrict__ points,
                                                            const int64_t* __restrict__ offsets, long n_points,
                                                            const double* __restrict__ T, const double* __restrict__ mei,
                                                            int G, int H, int W, int* __restrict__ winner) {
  const long HW = (long)H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_points; i += (long)gridDim.x * 256) {
    const int g = frame_of(offsets, G, i);
    const long local = i - offsets[g];
    if (local < 0 || local > 0x7fffffffL) continue;
    const CamPoint c = to_camera(points + i * 4, T + g * 16);
    if (!(c.z > 0.0)) continue;
    double u, v;
    mei_project(c, cam_norm(c), mei + g * 7, u, v);
    // astype(np.int32) truncates toward zero: (-1, W) is the range whose index lands inside; NaN fails both tests
    if (!(u > -1.0 && u < (double)W && v > -1.0 && v < (double)H)) continue;
    const int ix = (int)u, iy = (int)v;
    atomicMax(winner + g * HW + (long)iy * W + ix, (int)local);
  }
}

__global__ __launch_bounds__(256) void lidar_gather_kernel(const float* __restrict__ points,
                                                           const int64_t* __restrict__ offsets, long n_points,
                                                           const double* __restrict__ T, const int* __restrict__ winner,
                                                           int G, int H, int W, float* __restrict__ depth,
                                                           uint8_t* __restrict__ close_mask) {
  const long HW = (long)H * W, total = (long)G * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int g = (int)(i / HW);
    const int w = winner[i];
    float d = 0.f;
    uint8_t m = 0;
    const long p = offsets[g] + (long)w;
    if (w >= 0 && p >= 0 && p < n_points) {
      const CamPoint c = to_camera(points + p * 4, T + g * 16);
      const double norm = cam_norm(c);
      d = (float)c.z;
      m = (norm > 0.0 && norm < 8.0) ? 1 : 0;
    }
    depth[i] = d;
    close_mask[i] = m;
  }
}

unsigned grid_for(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }

}  // namespace

extern "C" int64_t fs_lidar_mei_depth_workspace_bytes(int G, int H, int W) {
  if (G < 1 || H < 1 || W < 1) return -1;
  return (((int64_t)G * H * W * 4) + 255) / 256 * 256;
}

extern "C" int fs_lidar_mei_depth(const float* points, const int64_t* offsets, int64_t n_points, const double* T,
                                  const double* mei, int G, int H, int W, float* depth, uint8_t* close_mask,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (!offsets || !T || !mei || !depth || !close_mask || !workspace || G < 1 || H < 1 || W < 1 || n_points < 0 ||
      (n_points > 0 && !points) || (int64_t)G * H * W >= (int64_t)1 << 31 ||
      workspace_bytes < fs_lidar_mei_depth_workspace_bytes(G, H, W))
    return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int* winner = static_cast<int*>(workspace);
  const long total = (long)G * H * W;
  hipLaunchKernelGGL(winner_init_kernel, dim3(grid_for(total)), dim3(256), 0, st, winner, total);
  if (n_points > 0)
    hipLaunchKernelGGL(lidar_scatter_kernel, dim3(grid_for(n_points)), dim3(256), 0, st, points, offsets, (long)n_points,
                       T, mei, G, H, W, winner);
  hipLaunchKernelGGL(lidar_gather_kernel, dim3(grid_for(total)), dim3(256), 0, st, points, offsets, (long)n_points, T,
                     winner, G, H, W, depth, close_mask);
  return fs_launch_status();
}
