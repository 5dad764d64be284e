// Training input pipeline on the device: one launch turns a batch of raw uint8 frames into the
// network / loss inputs.  Replaces, per sample and per frame, the DataLoader-worker chain of
// configs/kitti_wpose_example:129-155 (reference vision_base/data/augmentations/augmentations.py): ConvertToFloat
// :50-59, RandomWarpAffine :436-497 or Resize :112-198, RandomMirror :377-433, the colour ops :200-226 and :500-666,
// the crops and pads :228-375, Copy :668-680, Normalize :91-109, ConvertToTensor :62-88.  The random draws and the
// O(B) bookkeeping stay on the host in the mirrored classes (fsnet_amd/vision_base/data/augmentations); the kernels
// receive them as a per-sample plan.
// One frames kernel, instantiated for warp / resize and for the two plan forms: PlainPlan (mirror bit, three-slot fp32
// colour chain: FsAugArgs / FsResizeArgs, with or without a patched-mask plane) and WindowPlan (output window, op
// list with a Copy split and an f64 tail: FsAugExtArgs).  The sampling arithmetic (Sampler) and the per-frame store
// tail exist once; one masks kernel carries the other ground-truth images through the Sampler's nearest path.
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

// The colour ops of the extended launches — RandomHue :500-524, RandomEigenvalueNoise :594-626, PhotometricDistort
// :628-666 around a Copy :668-680 — as a list of up to FS_AUGX_OPS slots per sample.
struct ExtPixel {
  float c[3];
  double d[3] = {0.0, 0.0, 0.0};
  bool wide = false;  // RandomEigenvalueNoise added an f64 array: the image is f64 from there on (numpy promotion)
};

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

// ---- where an output pixel looks: canvas coordinate and the sample's extent ---------------------------------------
// The canvas is the warp's / resize's own output.  A window row (FsAugExtArgs::win: every crop, pad — CropTop :228-265,
// CropRight :268-301, Pad2Shape :304-324, RandomCropToWidth :343-375 — and mirror after the resampling stage, composed
// by the host) maps output pixel (xo, yo) to canvas pixel (x_off -+ xo, y_off + yo) inside its valid rectangle; outside
// it the pixel is np.pad's zero.  Without a row the canvas is the output, mirrored by iplan[4] (RandomMirror:
// out[:, xo] = canvas[:, W-1-xo]) and valid everywhere.
__device__ __forceinline__ bool canvas_coord(const int32_t* win, const int32_t* iplan, int b, int W, int xo, int yo,
                                             int& x, int& y) {
  if (win) {
    const int32_t* w = win + b * FS_AUGX_WIN;
    x = w[0] ? w[1] - xo : w[1] + xo;
    y = w[2] + yo;
    return xo >= w[3] && xo < w[5] && yo >= w[4] && yo < w[6];
  }
  x = (iplan && iplan[b * FS_AUG_IPLAN + 4]) ? W - 1 - xo : xo;
  y = yo;
  return true;
}

// sample b's own source extent sh x sw and, for a resize, the resized area rh x rw: the dims row, or iplan[5..6]
struct Extent { int sh, sw, rh, rw; };

__device__ __forceinline__ Extent dims_extent(const int32_t* dims, int b) {
  return {dims[b * 4], dims[b * 4 + 1], dims[b * 4 + 2], dims[b * 4 + 3]};
}

__device__ __forceinline__ Extent iplan_extent(const int32_t* iplan, int b) {
  return {iplan[b * FS_AUG_IPLAN + 5], iplan[b * FS_AUG_IPLAN + 6], 0, 0};
}

// OpenCV's float resize path (resize.cpp resizeGeneric_ / HResizeLinear / VResizeLinear): source coordinate
// (d + 0.5) * scale - 0.5 in f64, rounded to f32, floor + fraction; fraction 0 and index clamped at both borders
__device__ __forceinline__ void resize_coord(int d, double scale, int n, int& s0, float& f) {
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= n - 1) { fx = 0.f; sx = n - 1; }
  s0 = sx; f = fx;
}

// ---- the sampling arithmetic, once -----------------------------------------------------------------------------------
// Canvas pixel (x, y) of one sample, set up once and shared by its frames.
//   WARP:   cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) under the inverted map minv: four taps on the 1/32 grid,
//           each with its own inside-the-extent predicate.
//   resize: cv2.resize(float image, INTER_LINEAR) to rh x rw, zero-padded / cropped (augmentations.py:112-198): inside
//           the resized area the horizontal blend, then the vertical one, the second tap clamped; np.pad's zero outside
//           it (the zero passes the colour ops too).
// `near` is the INTER_NEAREST value of a uint8 plane in the frames' padded extent at the same pixel (the patched_mask,
// :163-164 and :484-487, or another ground-truth image): 1 without a plane, BORDER_CONSTANT / padding 0 outside.  It is
// formed only when `masked`.  The extent is clamped into the Hs x Ws plane and the resize's nearest index with it, so
// no row of a plan can make a tap or a mask read leave the buffer; on a valid plan (sh <= Hs, sw <= Ws) the clamps
// change nothing.
template <bool WARP>
struct Sampler {
  long t00 = 0, t01 = 0, t10 = 0, t11 = 0;                      // tap offsets inside one frame
  bool k00 = false, k01 = false, k10 = false, k11 = false;      // WARP: the tap exists; resize: k00 = inside
  float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;             // WARP: weights
  float fx = 0.f, fy = 0.f;                                     // resize: fractions
  int near = 0;

  __device__ __forceinline__ Sampler(int x, int y, bool valid, Extent e, int Hs, int Ws, const double* minv,
                                     bool masked, const uint8_t* plane) {
    const int sh = min(max(e.sh, 1), Hs), sw = min(max(e.sw, 1), Ws);
    if (WARP) {
      const FsWarpFixed c0 = fs_warp_fixed(minv, x, y);
      if (masked && valid) {
        long nx, ny;
        if (fs_warp_nearest(c0, sh, sw, nx, ny)) near = plane ? plane[ny * Ws + nx] : 1;
      }
      const long rd = (1 << AB_BITS) / INTER_TAB / 2;
      const long X = (c0.X + rd) >> (AB_BITS - INTER_BITS), Y = (c0.Y + rd) >> (AB_BITS - INTER_BITS);
      const long sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
      const float ax = (float)(X & (INTER_TAB - 1)) / (float)INTER_TAB, ay = (float)(Y & (INTER_TAB - 1)) / (float)INTER_TAB;
      w00 = (1.f - ay) * (1.f - ax); w01 = (1.f - ay) * ax; w10 = ay * (1.f - ax); w11 = ay * ax;
      const bool x0ok = sx >= 0 && sx < sw, x1ok = sx + 1 >= 0 && sx + 1 < sw;
      const bool y0ok = sy >= 0 && sy < sh, y1ok = sy + 1 >= 0 && sy + 1 < sh;
      k00 = valid && y0ok && x0ok; k01 = valid && y0ok && x1ok; k10 = valid && y1ok && x0ok; k11 = valid && y1ok && x1ok;
      t00 = (sy * Ws + sx) * 3; t01 = (sy * Ws + sx + 1) * 3;
      t10 = ((sy + 1) * Ws + sx) * 3; t11 = ((sy + 1) * Ws + sx + 1) * 3;
    } else {
      const int rh = e.rh, rw = e.rw;
      k00 = valid && rh > 0 && rw > 0 && x >= 0 && y >= 0 && y < rh && x < rw;
      int x0 = 0, y0 = 0;
      if (k00) {
        resize_coord(x, 1.0 / ((double)rw / (double)sw), sw, x0, fx);
        resize_coord(y, 1.0 / ((double)rh / (double)sh), sh, y0, fy);
        if (masked) {
          near = 1;
          if (plane) {
            const int ny = min(max(fs_resize_nearest(y, rh, sh), 0), Hs - 1);
            const int nx = min(max(fs_resize_nearest(x, rw, sw), 0), Ws - 1);
            near = plane[(long)ny * Ws + nx];
          }
        }
      }
      const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
      t00 = ((long)y0 * Ws + x0) * 3; t01 = ((long)y0 * Ws + x1) * 3;
      t10 = ((long)y1 * Ws + x0) * 3; t11 = ((long)y1 * Ws + x1) * 3;
    }
  }

  // channel k of the pixel from one [Hs][Ws][3] uint8 frame, 0..255 scale
  __device__ __forceinline__ float sample(const uint8_t* src, int k) const {
    if (WARP) {
      const float v00 = k00 ? (float)src[t00 + k] : 0.f, v01 = k01 ? (float)src[t01 + k] : 0.f;
      const float v10 = k10 ? (float)src[t10 + k] : 0.f, v11 = k11 ? (float)src[t11 + k] : 0.f;
      return v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
    }
    if (!k00) return 0.f;
    const float v00 = (float)src[t00 + k], v01 = (float)src[t01 + k];
    const float v10 = (float)src[t10 + k], v11 = (float)src[t11 + k];
    const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
    return top * (1.f - fy) + bot * fy;
  }
};

// ---- the two plan forms: what really differs between the launch families --------------------------------------------
// Both carry src [B][F][Hs][Ws][3], mask_src (NULL: ones), image / original [F][B][3][H][W], mask [B][H][W], mean / std
// and the sizes under the same names.  A plan adds where its pixels look (canvas, extent) and its colour ops around
// the point where `original` is taken (Copy: WindowPlan's split; the unaugmented frame for PlainPlan).
struct PlainPlan {
  const uint8_t* src; const double* minv; const int32_t* dims; const int32_t* iplan; const float* fplan;
  const uint8_t* mask_src; float* image; float* original; double* mask;
  float mean[3], std[3];
  int32_t B, F, Hs, Ws, H, W;
  struct Pixel { float c[3]; };

  __device__ __forceinline__ bool canvas(int b, int xo, int yo, int& x, int& y) const {
    return canvas_coord(nullptr, iplan, b, W, xo, yo, x, y);
  }
  __device__ __forceinline__ Extent extent(int b, bool warp) const {
    return warp ? iplan_extent(iplan, b) : dims_extent(dims, b);
  }
  __device__ __forceinline__ void ops_before_original(Pixel&, int) const {}
  __device__ __forceinline__ void ops_after_original(Pixel& px, int b) const {
    if (iplan) colour_chain(px.c, iplan + b * FS_AUG_IPLAN, fplan + b * FS_AUG_FPLAN);
  }
  __device__ __forceinline__ float value(const Pixel& px, int k) const { return px.c[k]; }
};

struct WindowPlan : FsAugExtArgs {
  using Pixel = ExtPixel;

  __device__ __forceinline__ bool canvas(int b, int xo, int yo, int& x, int& y) const {
    return canvas_coord(win, nullptr, b, W, xo, yo, x, y);
  }
  __device__ __forceinline__ Extent extent(int b, bool) const { return dims_extent(dims, b); }
  __device__ __forceinline__ void ops_before_original(Pixel& px, int b) const {
    ext_ops(px, ops + b * FS_AUGX_OPS, opv + b * FS_AUGX_OPS * 3, 0, split);
  }
  __device__ __forceinline__ void ops_after_original(Pixel& px, int b) const {
    ext_ops(px, ops + b * FS_AUGX_OPS, opv + b * FS_AUGX_OPS * 3, split, n_ops);
  }
  __device__ __forceinline__ float value(const Pixel& px, int k) const { return px.wide ? (float)px.d[k] : px.c[k]; }
};

// the per-frame tail: ('original_image', f) = pixel / 255 (Normalize with mean 0, std 1) at the plan's Copy point,
// ('image', f) = (pixel / 255 - mean) / std after the remaining colour ops, both HWC -> CHW into [F][B][3][H][W]
template <class Plan>
__device__ __forceinline__ void store_frame(const Plan& p, typename Plan::Pixel& px, int b, int f, int xo, int yo) {
  const long HW = (long)p.H * p.W;
  const long o = (((long)f * p.B + b) * 3) * HW + (long)yo * p.W + xo;
  p.ops_before_original(px, b);
  if (p.original) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.original[o + k * HW] = p.value(px, k) / 255.0f;
  }
  if (p.image) {
    p.ops_after_original(px, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) p.image[o + k * HW] = (p.value(px, k) / 255.0f - p.mean[k]) / p.std[k];
  }
}

template <bool WARP, class Plan>
__global__ __launch_bounds__(256) void frames_kernel(const Plan p) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.H * p.W) return;
  const int yo = i / p.W, xo = i - yo * p.W;
  int x, y;
  const bool valid = p.canvas(b, xo, yo, x, y);
  const Sampler<WARP> s(x, y, valid, p.extent(b, WARP), p.Hs, p.Ws, WARP ? p.minv + b * 6 : nullptr, p.mask != nullptr,
                        p.mask_src ? p.mask_src + (long)b * p.Hs * p.Ws : nullptr);
  if (p.mask) p.mask[((long)b * p.H + yo) * p.W + xo] = (double)s.near;     // the patched_mask rides with the frames
  for (int f = 0; f < p.F; ++f) {
    const uint8_t* src = p.src + ((long)b * p.F + f) * p.Hs * p.Ws * 3;
    typename Plan::Pixel px;
#pragma unroll
    for (int k = 0; k < 3; ++k) px.c[k] = s.sample(src, k);
    store_frame(p, px, b, f, xo, yo);
  }
}

// The other ground-truth images (e.g. a precomputed motion_mask) through the frames' plan: uint8 [B][Hs][Ws] -> fp32
// [B][H][W], the Sampler's nearest value at the canvas coordinate of the mirror bit (iplan) or the window row (win).
__global__ __launch_bounds__(256) void masks_kernel(const uint8_t* src, const double* minv, const int32_t* dims,
                                                     const int32_t* iplan, const int32_t* win, float* out, int Hs,
                                                     int Ws, int H, int W) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * W) return;
  const int yo = (int)(i / W), xo = (int)(i - (long)yo * W);
  int x, y;
  const bool valid = canvas_coord(win, iplan, b, W, xo, yo, x, y);
  const Extent e = dims ? dims_extent(dims, b) : iplan_extent(iplan, b);
  const uint8_t* plane = src + (long)b * Hs * Ws;
  const int v = minv ? Sampler<true>(x, y, valid, e, Hs, Ws, minv + b * 6, true, plane).near
                     : Sampler<false>(x, y, valid, e, Hs, Ws, nullptr, true, plane).near;
  out[(long)b * H * W + i] = (float)v;
}

// ---- host side -------------------------------------------------------------------------------------------------------
// what every frames launch refuses: a non-positive size, a frame or an output plane past the int indices, std 0
template <class Args>
bool frames_args_ok(const Args& a) {
  if (a.B < 1 || a.F < 1 || a.H < 1 || a.W < 1 || a.Hs < 1 || a.Ws < 1) return false;
  if ((long)a.Hs * a.Ws * 3 > 0x7fffffffL || (long)a.H * a.W > 0x7fffffffL) return false;
  for (int k = 0; k < 3; ++k) if (a.std[k] == 0.f) return false;
  return true;
}

dim3 pixel_grid(int H, int W, int B) { return dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)B); }

template <bool WARP, class Plan>
int launch_frames(const Plan& p, void* stream) {
  hipLaunchKernelGGL((frames_kernel<WARP, Plan>), pixel_grid(p.H, p.W, p.B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  return fs_launch_status();
}

// the fields FsAugArgs and FsResizeArgs share by name
template <class Args>
PlainPlan plain_plan(const Args& a, const uint8_t* mask_src) {
  PlainPlan p{};
  p.src = a.src; p.iplan = a.iplan; p.fplan = a.fplan; p.mask_src = mask_src;
  p.image = a.image; p.original = a.original; p.mask = a.mask;
  for (int k = 0; k < 3; ++k) { p.mean[k] = a.mean[k]; p.std[k] = a.std[k]; }
  p.B = a.B; p.F = a.F; p.Hs = a.Hs; p.Ws = a.Ws; p.H = a.H; p.W = a.W;
  return p;
}

int launch_resize(const FsResizeArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !a->src || !a->dims || !a->image) return FS_EINVAL;
  if ((a->iplan != nullptr) != (a->fplan != nullptr)) return FS_EINVAL;
  if (!frames_args_ok(*a)) return FS_EINVAL;
  PlainPlan p = plain_plan(*a, mask_src);
  p.dims = a->dims;
  return launch_frames<false>(p, stream);
}

int launch_augment(const FsAugArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !a->src || !a->minv || !a->iplan || !a->fplan || (!a->image && !a->original)) return FS_EINVAL;
  if (!frames_args_ok(*a)) return FS_EINVAL;
  PlainPlan p = plain_plan(*a, mask_src);
  p.minv = a->minv;
  return launch_frames<true>(p, stream);
}

int launch_ext(const FsAugExtArgs* a, bool warp, void* stream) {
  if (!a || !a->src || !a->dims || !a->win || (!a->image && !a->original)) return FS_EINVAL;
  if (warp != (a->minv != nullptr)) return FS_EINVAL;
  if (a->mask_src && !a->mask) return FS_EINVAL;
  if (!frames_args_ok(*a)) return FS_EINVAL;
  if (a->n_ops < 0 || a->n_ops > FS_AUGX_OPS || a->split < 0 || a->split > a->n_ops) return FS_EINVAL;
  if (a->n_ops > 0 && (!a->ops || !a->opv)) return FS_EINVAL;
  const WindowPlan p{*a};
  return warp ? launch_frames<true>(p, stream) : launch_frames<false>(p, stream);
}

int launch_masks(const uint8_t* src, const double* minv, const int32_t* dims, const int32_t* iplan, const int32_t* win,
                 float* out, int B, int Hs, int Ws, int H, int W, void* stream) {
  if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return FS_EINVAL;
  if ((long)Hs * Ws >= (1L << 31) || (long)H * W >= (1L << 31)) return FS_EINVAL;
  hipLaunchKernelGGL(masks_kernel, pixel_grid(H, W, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, minv,
                     dims, iplan, win, out, Hs, Ws, H, W);
  return fs_launch_status();
}

}  // namespace

extern "C" int fs_augment_frames(const FsAugArgs* a, void* stream) { return launch_augment(a, nullptr, stream); }

extern "C" int fs_resize_frames(const FsResizeArgs* a, void* stream) { return launch_resize(a, nullptr, stream); }

// the same launches with the batch's patched masks: a plane needs somewhere to go
extern "C" int fs_augment_frames_masked(const FsAugArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !mask_src || !a->mask) return FS_EINVAL;
  return launch_augment(a, mask_src, stream);
}

extern "C" int fs_resize_frames_masked(const FsResizeArgs* a, const uint8_t* mask_src, void* stream) {
  if (!a || !mask_src || !a->mask) return FS_EINVAL;
  return launch_resize(a, mask_src, stream);
}

extern "C" int fs_augment_frames_ext(const FsAugExtArgs* a, void* stream) { return launch_ext(a, true, stream); }

extern "C" int fs_resize_frames_ext(const FsAugExtArgs* a, void* stream) { return launch_ext(a, false, stream); }

// warp (minv, extent in iplan[5..6]) or resize (dims), then RandomMirror (iplan[4])
extern "C" int fs_augment_masks(const uint8_t* src, const double* minv, const int32_t* dims, const int32_t* iplan,
                                float* out, int B, int Hs, int Ws, int H, int W, void* stream) {
  if (!src || !out || (minv != nullptr) == (dims != nullptr) || (minv && !iplan)) return FS_EINVAL;
  return launch_masks(src, minv, dims, iplan, nullptr, out, B, Hs, Ws, H, W, stream);
}

extern "C" int fs_augment_masks_ext(const uint8_t* src, const double* minv, const int32_t* dims, const int32_t* win,
                                    float* out, int B, int Hs, int Ws, int H, int W, void* stream) {
  if (!src || !dims || !win || !out) return FS_EINVAL;
  return launch_masks(src, minv, dims, nullptr, win, out, B, Hs, Ws, H, W, stream);
}
