// Nearest-neighbour source coordinates of the training input pipeline, in one place: the patched mask that rides in the
// frames' launches and the other ground-truth images (fs_augment_masks), both through augment.hip's Sampler, sample with
// the same arithmetic as cv2.warpAffine / cv2.resize with INTER_NEAREST (oracle/augment_oracle.py warp_affine_nearest,
// resize_nearest; reference augmentations.py:163-164, :484-487).
#pragma once
#include <cstdint>

constexpr int FS_WARP_AB_BITS = 10;      // imgwarp.cpp AB_BITS: fixed-point fraction of a warpAffine coordinate

// cv2.warpAffine's fixed-point source coordinate of output pixel (x, y) under the inverted map m (f64 [6]), before the
// interpolation's rounding term: saturate_cast<int>(double) = round-half-even on each of the two addends.
struct FsWarpFixed { long X, Y; };

__device__ __forceinline__ FsWarpFixed fs_warp_fixed(const double* m, int x, int y) {
  const double s = (double)(1 << FS_WARP_AB_BITS);
  const long adelta = (long)rint(m[0] * (double)x * s);
  const long bdelta = (long)rint(m[3] * (double)x * s);
  const long X00 = (long)rint((m[1] * (double)y + m[2]) * s);
  const long Y00 = (long)rint((m[4] * (double)y + m[5]) * s);
  return {X00 + adelta, Y00 + bdelta};
}

// INTER_NEAREST: round to the nearest source pixel; true when it lies inside the sample's own sh x sw
__device__ __forceinline__ bool fs_warp_nearest(const FsWarpFixed c, int sh, int sw, long& sx, long& sy) {
  const long rd = (1 << FS_WARP_AB_BITS) / 2;
  sx = (c.X + rd) >> FS_WARP_AB_BITS;
  sy = (c.Y + rd) >> FS_WARP_AB_BITS;
  return sx >= 0 && sx < sw && sy >= 0 && sy < sh;
}

// cv2.resize INTER_NEAREST (resize.cpp resizeNN): min(floor(d * (n_src / n_dst)), n_src - 1), the scale in f64
__device__ __forceinline__ int fs_resize_nearest(int d, int n_dst, int n_src) {
  return min((int)floor((double)d * (1.0 / ((double)n_dst / (double)n_src))), n_src - 1);
}
