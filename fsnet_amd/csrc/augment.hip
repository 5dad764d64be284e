// Training input pipeline on the device: one launch turns a batch of raw uint8 frames into the
// network / loss inputs.  Replaces, per sample and per frame, the DataLoader-worker chain of
// configs/kitti_wpose_example:129-155:
//   ConvertToFloat                                          vision_base/data/augmentations/augmentations.py:50-59
//   RandomWarpAffine (cv2.warpAffine, INTER_LINEAR for the frames, INTER_NEAREST for patched_mask)      :436-497
//   RandomMirror (images, mask)                                                                         :377-433
//   Shuffle[RandomBrightness :572-591, RandomContrast :545-569, ConvertColor/RandomSaturation :527-542, :200-226]
//   Normalize (mean/std for ('image', i); 0/1 for ('original_image', i))                                :91-109
//   ConvertToTensor (HWC -> CHW)                                                                        :62-88
// The random draws and the O(B) bookkeeping (P2, relative poses) stay on the host in the mirrored classes
// (fsnet_amd/vision_base/data/augmentations); this kernel receives them as a per-sample plan.
// A patched_mask that is not all ones (NusceneJsonDataset's CAM_BACK) rides in the same launch through the *_masked
// entry points: mask_src, a uint8 0/1 plane in the frames' padded extent, is read at the INTER_NEAREST coordinate
// (nearest.h) and written as f64; without a plane the mask of ones is synthesised from the coordinate alone.
// cv2 is a third-party dependency absent from the reference tree: warpAffine follows OpenCV's imgwarp.cpp (matrix
// inverted in f64 by the host, 10-bit fixed-point coordinates, 1/32-pixel bilinear grid, BORDER_CONSTANT 0) and
// cvtColor its color_hsv RGB2HSV_f / HSV2RGB_f (hrange 360) — see oracle/augment_oracle.py ("parity unpinned").
// All pixel arithmetic is fp32 in the reference's operation order (the build has -ffp-contract=off, divisions are
// IEEE), so the result equals the numpy restatement bit for bit.
#include "common.h"
#include "fsnet_hip_internal.h"
#include "nearest.h"
#include <cstdint>

namespace {

constexpr int AB_BITS = FS_WARP_AB_BITS, INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS;
constexpr float FLT_EPS = 1.1920929e-07f;

__device__ __forceinline__ void rgb2hsv(float r, float g, float b, float& h, float& s, float& v) {
  v = fmaxf(fmaxf(r, g), b);
  const float vmin = fminf(fminf(r, g), b);
  float diff = v - vmin;
  s = diff / (fabsf(v) + FLT_EPS);
  diff = 60.f / (diff + FLT_EPS);
  if (v == r) h = (g - b) * diff;
  else if (v == g) h = (b - r) * diff + 120.f;
  else h = (r - g) * diff + 240.f;
  if (h < 0.f) h += 360.f;
}

__device__ __forceinline__ void hsv2rgb(float h, float s, float v, float& r, float& g, float& b) {
  if (s == 0.f) { r = g = b = v; return; }
  float hh = h * (6.f / 360.f);
  if (hh < 0.f) hh += 6.f;
  if (hh >= 6.f) hh -= 6.f;
  int sector = (int)floorf(hh);
  float f = hh - (float)sector;
  if ((unsigned)sector >= 6u) { sector = 0; f = 0.f; }
  const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * f), t3 = v * (1.f - s * (1.f - f));
  switch (sector) {           // (b, g, r) <- {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
    case 0: b = t1; g = t3; r = t0; break;
    case 1: b = t1; g = t0; r = t2; break;
    case 2: b = t3; g = t0; r = t1; break;
    case 3: b = t0; g = t2; r = t1; break;
    case 4: b = t0; g = t1; r = t3; break;
    default: b = t2; g = t1; r = t0; break;
  }
}

// Shuffle[RandomBrightness, RandomContrast, HSV round trip with RandomSaturation] in the drawn order (plan slots 0-2,
// applied-bits in slot 3) on one pixel, 0..255 scale
__device__ __forceinline__ void colour_chain(float (&c)[3], const int32_t* ip, const float* fp) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int op = ip[q];
    if (op == 0) {
      if (ip[3] & 1) { c[0] = c[0] + fp[0]; c[1] = c[1] + fp[0]; c[2] = c[2] + fp[0]; }
    } else if (op == 1) {
      if (ip[3] & 2) { c[0] = c[0] * fp[1]; c[1] = c[1] * fp[1]; c[2] = c[2] * fp[1]; }
    } else if (op == 2 && (ip[3] & 8)) {      // ConvertColor(HSV) .. ConvertColor(RGB) with or without a draw
      float h, s, v;
      rgb2hsv(c[0], c[1], c[2], h, s, v);
      if (ip[3] & 4) s = s * fp[2];
      hsv2rgb(h, s, v, c[0], c[1], c[2]);
    }
  }
}

__global__ __launch_bounds__(256) void augment_frames_kernel(const FsAugArgs p, const uint8_t* mask_src) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.H * p.W) return;
  const int y = i / p.W, xo = i - y * p.W;
  const int32_t* ip = p.iplan + b * FS_AUG_IPLAN;
  const float* fp = p.fplan + b * FS_AUG_FPLAN;
  const double* m = p.minv + b * 6;
  const int sh = ip[5], sw = ip[6];
  const int x = ip[4] ? p.W - 1 - xo : xo;                 // RandomMirror: out[:, xo] = warped[:, W-1-xo]

  const FsWarpFixed c0 = fs_warp_fixed(m, x, y);           // cv2.warpAffine coordinates

  if (p.mask) {   // patched_mask warped with INTER_NEAREST: the mask's value (1 without a plane) where the nearest
                  // source pixel exists, BORDER_CONSTANT 0 elsewhere
    long nx, ny;
    double v = 0.0;
    if (!mask_src) v = fs_warp_nearest(c0, sh, sw, nx, ny) ? 1.0 : 0.0;
    else if (fs_warp_nearest(c0, min(sh, p.Hs), min(sw, p.Ws), nx, ny))   // a plan past the plane reads nothing
      v = (double)mask_src[((long)b * p.Hs + ny) * p.Ws + nx];
    p.mask[((long)b * p.H + y) * p.W + xo] = v;
  }
  const long rd = (1 << AB_BITS) / INTER_TAB / 2;
  const long X = (c0.X + rd) >> (AB_BITS - INTER_BITS), Y = (c0.Y + rd) >> (AB_BITS - INTER_BITS);
  const long sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
  const float fx = (float)(X & (INTER_TAB - 1)) / (float)INTER_TAB, fy = (float)(Y & (INTER_TAB - 1)) / (float)INTER_TAB;
  const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
  const bool x0ok = sx >= 0 && sx < sw, x1ok = sx + 1 >= 0 && sx + 1 < sw;
  const bool y0ok = sy >= 0 && sy < sh, y1ok = sy + 1 >= 0 && sy + 1 < sh;
  const long HW = (long)p.H * p.W;

  for (int f = 0; f < p.F; ++f) {
    const uint8_t* src = p.src + ((long)b * p.F + f) * p.Hs * p.Ws * 3;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v00 = (y0ok && x0ok) ? (float)src[(sy * p.Ws + sx) * 3 + k] : 0.f;
      const float v01 = (y0ok && x1ok) ? (float)src[(sy * p.Ws + sx + 1) * 3 + k] : 0.f;
      const float v10 = (y1ok && x0ok) ? (float)src[((sy + 1) * p.Ws + sx) * 3 + k] : 0.f;
      const float v11 = (y1ok && x1ok) ? (float)src[((sy + 1) * p.Ws + sx + 1) * 3 + k] : 0.f;
      c[k] = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
    }
    const long o = (((long)f * p.B + b) * 3) * HW + (long)y * p.W + xo;
    if (p.original) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p.original[o + k * HW] = c[k] / 255.0f;        // Normalize(mean 0, std 1)
    }
    if (p.image) {
      colour_chain(c, ip, fp);
#pragma unroll
      for (int k = 0; k < 3; ++k) p.image[o + k * HW] = (c[k] / 255.0f - p.mean[k]) / p.std[k];
    }
  }
}

// Resize-based inputs.  Validation (configs/kitti_wpose_example:156-166) and, with a per-sample plan, the training
// input of the Resize-based configs (configs/multi_dataset_example:178-205: Resize of all frames + INTER_NEAREST
// patched_mask, colour Shuffle, RandomMirror, two Normalizes).  Resize = cv2.resize(float image, INTER_LINEAR) to
// rh x rw, zero-padded / cropped to H x W (augmentations.py:112-198), then Normalize and CHW.  OpenCV's float
// path (resize.cpp resizeGeneric_ / HResizeLinear / VResizeLinear): source coordinate (d + 0.5) * scale - 0.5 in
// f64, rounded to f32, floor + fraction; fraction 0 and index clamped at both borders; horizontal pass, then vertical.
__device__ __forceinline__ void resize_coord(int d, double scale, int n, int& s0, float& f) {
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= n - 1) { fx = 0.f; sx = n - 1; }
  s0 = sx; f = fx;
}

__global__ __launch_bounds__(256) void resize_frames_kernel(const FsResizeArgs p, const uint8_t* mask_src) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.H * p.W) return;
  const int y = i / p.W, xo = i - y * p.W;
  const int32_t* d = p.dims + b * 4;
  const int sh = d[0], sw = d[1], rh = d[2], rw = d[3];
  const int32_t* ip = p.iplan ? p.iplan + b * FS_AUG_IPLAN : nullptr;
  const float* fp = p.fplan ? p.fplan + b * FS_AUG_FPLAN : nullptr;
  const int x = (ip && ip[4]) ? p.W - 1 - xo : xo;         // RandomMirror of the padded / cropped image
  const bool inside = y < rh && x < rw;                    // outside: np.pad zeros (they pass the colour ops too)
  int x0 = 0, y0 = 0; float fx = 0.f, fy = 0.f;
  if (inside) {
    resize_coord(x, 1.0 / ((double)rw / (double)sw), sw, x0, fx);
    resize_coord(y, 1.0 / ((double)rh / (double)sh), sh, y0, fy);
  }
  const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
  const long HW = (long)p.H * p.W;
  // patched_mask through cv2.resize(INTER_NEAREST): the plane's value (ones without a plane); the padding is zero
  if (p.mask) {
    double v = inside ? 1.0 : 0.0;
    if (inside && mask_src) {
      const int ny = min(max(fs_resize_nearest(y, rh, sh), 0), p.Hs - 1);   // inside the plane whatever dims say
      const int nx = min(max(fs_resize_nearest(x, rw, sw), 0), p.Ws - 1);
      v = (double)mask_src[((long)b * p.Hs + ny) * p.Ws + nx];
    }
    p.mask[((long)b * p.H + y) * p.W + xo] = v;
  }
  for (int f = 0; f < p.F; ++f) {
    const uint8_t* src = p.src + ((long)b * p.F + f) * p.Hs * p.Ws * 3;
    const long o = (((long)f * p.B + b) * 3) * HW + (long)y * p.W + xo;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = 0.f;
      if (inside) {
        const float v00 = (float)src[((long)y0 * p.Ws + x0) * 3 + k], v01 = (float)src[((long)y0 * p.Ws + x1) * 3 + k];
        const float v10 = (float)src[((long)y1 * p.Ws + x0) * 3 + k], v11 = (float)src[((long)y1 * p.Ws + x1) * 3 + k];
        const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
        v = top * (1.f - fy) + bot * fy;
      }
      c[k] = v;
    }
    if (p.original) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p.original[o + k * HW] = c[k] / 255.0f;
    }
    if (ip) colour_chain(c, ip, fp);
#pragma unroll
    for (int k = 0; k < 3; ++k) p.image[o + k * HW] = (c[k] / 255.0f - p.mean[k]) / p.std[k];
  }
}

int launch_resize(const FsResizeArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !a->src || !a->dims || !a->image) return FS_EINVAL;
  if ((a->iplan != nullptr) != (a->fplan != nullptr)) return FS_EINVAL;
  if (a->B < 1 || a->F < 1 || a->H < 1 || a->W < 1 || a->Hs < 1 || a->Ws < 1) return FS_EINVAL;
  if ((long)a->Hs * a->Ws * 3 > 0x7fffffffL) return FS_EINVAL;
  for (int k = 0; k < 3; ++k) if (a->std[k] == 0.f) return FS_EINVAL;
  dim3 grid((unsigned)(((long)a->H * a->W + 255) / 256), (unsigned)a->B);
  hipLaunchKernelGGL(resize_frames_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a, mask_src);
  return fs_launch_status();
}

int launch_augment(const FsAugArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !a->src || !a->minv || !a->iplan || !a->fplan || (!a->image && !a->original)) return FS_EINVAL;
  if (a->B < 1 || a->F < 1 || a->H < 1 || a->W < 1 || a->Hs < 1 || a->Ws < 1) return FS_EINVAL;
  if ((long)a->Hs * a->Ws * 3 > 0x7fffffffL) return FS_EINVAL;
  for (int k = 0; k < 3; ++k) if (a->std[k] == 0.f) return FS_EINVAL;
  dim3 grid((unsigned)(((long)a->H * a->W + 255) / 256), (unsigned)a->B);
  hipLaunchKernelGGL(augment_frames_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a, mask_src);
  return fs_launch_status();
}

// ---- extended launches: an output window over the resampled canvas and a colour op list ---------------------------
// The remaining classes of the reference's augmentations.py — CropTop :228-265, CropRight :268-301, Pad2Shape :304-324,
// RandomCropToWidth :343-375 after the resampling stage, RandomHue :500-524, RandomEigenvalueNoise :594-626,
// PhotometricDistort :628-666, Copy :668-680.  The host composes every crop / pad / mirror that follows the warp or
// resize into one window row per sample (FsAugExtArgs::win); output pixel (xo, yo) reads canvas pixel
// (x_off -+ xo, y_off + yo) inside the valid rectangle and is np.pad's zero outside it.  The sampling arithmetic is
// that of the two kernels above, statement for statement.
struct ExtPixel {
  float c[3];
  double d[3];
  bool wide;         // RandomEigenvalueNoise added an f64 array: the image is f64 from there on (numpy promotion)
};

__device__ __forceinline__ float ext_value(const ExtPixel& px, int k) { return px.wide ? (float)px.d[k] : px.c[k]; }

// slots [from, to) of one sample's op list on one pixel, 0..255 scale
__device__ __forceinline__ void ext_ops(ExtPixel& px, const int32_t* code, const double* val, int from, int to) {
  for (int q = from; q < to; ++q) {
    const int kind = code[q] & 15, flags = code[q] >> 4;
    const double* v = val + q * 3;
    if (kind == FS_AUGX_BRIGHTNESS) {
      if (px.wide) { px.d[0] = px.d[0] + v[0]; px.d[1] = px.d[1] + v[0]; px.d[2] = px.d[2] + v[0]; }
      else { const float t = (float)v[0]; px.c[0] = px.c[0] + t; px.c[1] = px.c[1] + t; px.c[2] = px.c[2] + t; }
    } else if (kind == FS_AUGX_CONTRAST) {
      if (px.wide) { px.d[0] = px.d[0] * v[0]; px.d[1] = px.d[1] * v[0]; px.d[2] = px.d[2] * v[0]; }
      else { const float t = (float)v[0]; px.c[0] = px.c[0] * t; px.c[1] = px.c[1] * t; px.c[2] = px.c[2] * t; }
    } else if (kind == FS_AUGX_HSV) {
      if (px.wide) continue;                 // refused on the host: cv2.cvtColor takes no f64 image
      float h, s, vv;
      rgb2hsv(px.c[0], px.c[1], px.c[2], h, s, vv);
      if (flags & 1) s = s * (float)v[0];    // RandomSaturation
      if (flags & 2) {                       // RandomHue: shift, then the two wraps in the reference's order
        h = h + (float)v[1];
        if (h > 360.f) h = h - 360.f;
        if (h < 0.f) h = h + 360.f;
      }
      hsv2rgb(h, s, vv, px.c[0], px.c[1], px.c[2]);
    } else if (kind == FS_AUGX_NOISE) {
      if (!px.wide) { px.d[0] = (double)px.c[0]; px.d[1] = (double)px.c[1]; px.d[2] = (double)px.c[2]; px.wide = true; }
      px.d[0] = px.d[0] + v[0]; px.d[1] = px.d[1] + v[1]; px.d[2] = px.d[2] + v[2];
    }
  }
}

// the window row of sample b: true inside the valid rectangle, with the canvas coordinate of output pixel (xo, yo)
__device__ __forceinline__ bool ext_window(const int32_t* w, int xo, int yo, int& x, int& y) {
  x = w[0] ? w[1] - xo : w[1] + xo;
  y = w[2] + yo;
  return xo >= w[3] && xo < w[5] && yo >= w[4] && yo < w[6];
}

template <bool WARP>
__global__ __launch_bounds__(256) void augment_ext_kernel(const FsAugExtArgs p) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.H * p.W) return;
  const int yo = i / p.W, xo = i - yo * p.W;
  const int32_t* d = p.dims + b * 4;
  // the sample's own extent, kept inside the buffer whatever the row says
  const int sh = min(max(d[0], 1), p.Hs), sw = min(max(d[1], 1), p.Ws);
  int x, y;
  const bool valid = ext_window(p.win + b * FS_AUGX_WIN, xo, yo, x, y);
  const int32_t* code = p.ops + b * FS_AUGX_OPS;
  const double* val = p.opv + b * FS_AUGX_OPS * 3;
  const long HW = (long)p.H * p.W;

  // taps and weights of this pixel, shared by the frames
  long t00 = 0, t01 = 0, t10 = 0, t11 = 0;
  bool k00 = false, k01 = false, k10 = false, k11 = false;
  float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f, fx = 0.f, fy = 0.f;
  double mv = 0.0;
  if (WARP) {
    const FsWarpFixed c0 = fs_warp_fixed(p.minv + b * 6, x, y);
    if (p.mask && valid) {
      long nx, ny;
      if (fs_warp_nearest(c0, sh, sw, nx, ny)) mv = p.mask_src ? (double)p.mask_src[((long)b * p.Hs + ny) * p.Ws + nx] : 1.0;
    }
    const long rd = (1 << AB_BITS) / INTER_TAB / 2;
    const long X = (c0.X + rd) >> (AB_BITS - INTER_BITS), Y = (c0.Y + rd) >> (AB_BITS - INTER_BITS);
    const long sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
    fx = (float)(X & (INTER_TAB - 1)) / (float)INTER_TAB; fy = (float)(Y & (INTER_TAB - 1)) / (float)INTER_TAB;
    w00 = (1.f - fy) * (1.f - fx); w01 = (1.f - fy) * fx; w10 = fy * (1.f - fx); w11 = fy * fx;
    const bool x0ok = sx >= 0 && sx < sw, x1ok = sx + 1 >= 0 && sx + 1 < sw;
    const bool y0ok = sy >= 0 && sy < sh, y1ok = sy + 1 >= 0 && sy + 1 < sh;
    k00 = valid && y0ok && x0ok; k01 = valid && y0ok && x1ok; k10 = valid && y1ok && x0ok; k11 = valid && y1ok && x1ok;
    t00 = (sy * p.Ws + sx) * 3; t01 = (sy * p.Ws + sx + 1) * 3;
    t10 = ((sy + 1) * p.Ws + sx) * 3; t11 = ((sy + 1) * p.Ws + sx + 1) * 3;
  } else {
    const int rh = d[2], rw = d[3];
    const bool inside = valid && rh > 0 && rw > 0 && x >= 0 && y >= 0 && y < rh && x < rw;   // else np.pad zeros
    int x0 = 0, y0 = 0;
    if (inside) {
      resize_coord(x, 1.0 / ((double)rw / (double)sw), sw, x0, fx);
      resize_coord(y, 1.0 / ((double)rh / (double)sh), sh, y0, fy);
      if (p.mask) {
        mv = 1.0;
        if (p.mask_src) {
          const int ny = min(max(fs_resize_nearest(y, rh, sh), 0), p.Hs - 1);
          const int nx = min(max(fs_resize_nearest(x, rw, sw), 0), p.Ws - 1);
          mv = (double)p.mask_src[((long)b * p.Hs + ny) * p.Ws + nx];
        }
      }
    }
    const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
    k00 = inside;
    t00 = ((long)y0 * p.Ws + x0) * 3; t01 = ((long)y0 * p.Ws + x1) * 3;
    t10 = ((long)y1 * p.Ws + x0) * 3; t11 = ((long)y1 * p.Ws + x1) * 3;
  }
  if (p.mask) p.mask[((long)b * p.H + yo) * p.W + xo] = mv;

  for (int f = 0; f < p.F; ++f) {
    const uint8_t* src = p.src + ((long)b * p.F + f) * p.Hs * p.Ws * 3;
    ExtPixel px;
    px.wide = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      px.d[k] = 0.0;
      if (WARP) {
        const float v00 = k00 ? (float)src[t00 + k] : 0.f, v01 = k01 ? (float)src[t01 + k] : 0.f;
        const float v10 = k10 ? (float)src[t10 + k] : 0.f, v11 = k11 ? (float)src[t11 + k] : 0.f;
        px.c[k] = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
      } else {
        float v = 0.f;
        if (k00) {
          const float v00 = (float)src[t00 + k], v01 = (float)src[t01 + k];
          const float v10 = (float)src[t10 + k], v11 = (float)src[t11 + k];
          const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
          v = top * (1.f - fy) + bot * fy;
        }
        px.c[k] = v;
      }
    }
    const long o = (((long)f * p.B + b) * 3) * HW + (long)yo * p.W + xo;
    ext_ops(px, code, val, 0, p.split);                     // Copy: the image as it is after `split` ops
    if (p.original) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p.original[o + k * HW] = ext_value(px, k) / 255.0f;      // Normalize(mean 0, std 1)
    }
    if (p.image) {
      ext_ops(px, code, val, p.split, p.n_ops);
#pragma unroll
      for (int k = 0; k < 3; ++k) p.image[o + k * HW] = (ext_value(px, k) / 255.0f - p.mean[k]) / p.std[k];
    }
  }
}

// the extra ground-truth images through the same window (fs_augment_masks of optflow.hip for the plain plans)
__global__ __launch_bounds__(256) void augment_masks_ext_kernel(const uint8_t* src, const double* minv,
                                                                 const int32_t* dims, const int32_t* win, float* out,
                                                                 int Hs, int Ws, int H, int W) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * W) return;
  const int yo = (int)(i / W), xo = (int)(i - (long)yo * W);
  const int32_t* d = dims + b * 4;
  const int sh = min(max(d[0], 1), Hs), sw = min(max(d[1], 1), Ws);
  int x, y;
  const bool valid = ext_window(win + b * FS_AUGX_WIN, xo, yo, x, y);
  const uint8_t* s = src + (long)b * Hs * Ws;
  float v = 0.f;
  if (valid && minv) {
    long sx, sy;
    if (fs_warp_nearest(fs_warp_fixed(minv + b * 6, x, y), sh, sw, sx, sy)) v = (float)s[sy * Ws + sx];
  } else if (valid) {
    const int rh = d[2], rw = d[3];
    if (rh > 0 && rw > 0 && x >= 0 && y >= 0 && y < rh && x < rw) {
      const int ny = min(max(fs_resize_nearest(y, rh, sh), 0), Hs - 1);
      const int nx = min(max(fs_resize_nearest(x, rw, sw), 0), Ws - 1);
      v = (float)s[(long)ny * Ws + nx];
    }
  }
  out[(long)b * H * W + i] = v;
}

int launch_ext(const FsAugExtArgs* a, bool warp, void* stream) {
  if (!a || !a->src || !a->dims || !a->win || (!a->image && !a->original)) return FS_EINVAL;
  if (warp != (a->minv != nullptr)) return FS_EINVAL;
  if (a->mask_src && !a->mask) return FS_EINVAL;
  if (a->B < 1 || a->F < 1 || a->H < 1 || a->W < 1 || a->Hs < 1 || a->Ws < 1) return FS_EINVAL;
  if (a->n_ops < 0 || a->n_ops > FS_AUGX_OPS || a->split < 0 || a->split > a->n_ops) return FS_EINVAL;
  if (a->n_ops > 0 && (!a->ops || !a->opv)) return FS_EINVAL;
  if ((long)a->Hs * a->Ws * 3 > 0x7fffffffL || (long)a->H * a->W > 0x7fffffffL) return FS_EINVAL;
  for (int k = 0; k < 3; ++k) if (a->std[k] == 0.f) return FS_EINVAL;
  dim3 grid((unsigned)(((long)a->H * a->W + 255) / 256), (unsigned)a->B);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (warp) hipLaunchKernelGGL(augment_ext_kernel<true>, grid, dim3(256), 0, st, *a);
  else hipLaunchKernelGGL(augment_ext_kernel<false>, grid, dim3(256), 0, st, *a);
  return fs_launch_status();
}

}  // namespace

extern "C" int fs_augment_frames_ext(const FsAugExtArgs* a, void* stream) { return launch_ext(a, true, stream); }

extern "C" int fs_resize_frames_ext(const FsAugExtArgs* a, void* stream) { return launch_ext(a, false, stream); }

extern "C" int fs_augment_masks_ext(const uint8_t* src, const double* minv, const int32_t* dims, const int32_t* win,
                                    float* out, int B, int Hs, int Ws, int H, int W, void* stream) {
  if (!src || !dims || !win || !out) return FS_EINVAL;
  if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return FS_EINVAL;
  if ((long)Hs * Ws >= (1L << 31) || (long)H * W >= (1L << 31)) return FS_EINVAL;
  dim3 grid((unsigned)(((long)H * W + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(augment_masks_ext_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, minv,
                     dims, win, out, Hs, Ws, H, W);
  return fs_launch_status();
}

extern "C" int fs_resize_frames(const FsResizeArgs* a, void* stream) { return launch_resize(a, nullptr, stream); }

extern "C" int fs_augment_frames(const FsAugArgs* a, void* stream) { return launch_augment(a, nullptr, stream); }

// the same launches with the batch's patched masks: a plane needs somewhere to go
extern "C" int fs_resize_frames_masked(const FsResizeArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !mask_src || !a->mask) return FS_EINVAL;
  return launch_resize(a, mask_src, stream);
}

extern "C" int fs_augment_frames_masked(const FsAugArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !mask_src || !a->mask) return FS_EINVAL;
  return launch_augment(a, mask_src, stream);
}
