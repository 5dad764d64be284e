// Plane-sweep matching cost volume of the multi-frame depth encoder, one launch for a whole batch.
// Replaces (reference): ResnetEncoderMatching.match_features and the confidence / lowest-cost / masking lines of its
// forward (monodepth/networks/models/backbone/resnet_matching.py:83-173, 227-237) with BackprojectDepth / Project3D
// (monodepth/networks/utils/monodepth_utils.py:132-165) and F.grid_sample(bilinear, zeros, align_corners=True).
// The warped [D][C][h][w] features of the reference never exist: a tap is read, compared and summed in registers.
//
// Arithmetic, fp32 in the reference's operation order (no FMA: the library is built with -ffp-contract=off):
//   r = inv_K[:3,:3] (x, y, 1);  X = bin * r;  P = (K T)[:3,:];  c = P (X, 1);  p = c.xy / (c.z + 1e-7)   (no sign test)
//   g = (p / (w-1, h-1) - 0.5) * 2;  edge test on (g / 2 + 0.5) * (w-1, h-1): 2 <= x <= w-2, 2 <= y <= h-2, and the current
//   pixel inside [2:-2, 2:-2];  sample position ((g + 1) / 2) * (w-1, h-1) (grid_sample's own unnormalisation).
//   diff = mean_C |warped - current| where the test holds (else 0: its taps are not loaded); cost += diff, count += diff > 0
//   over the lookup frames whose 16 pose entries do not sum to exactly 0 (decided here: no host sync);
//   cost /= count + 1e-7;  missing = cost == 0;  missing bins take the pixel's maximum over the bins;
//   confidence = no bin missing;  lowest = 1 / bins[first argmin of the filled costs, exact zeros read as 100];
//   the value written into the concat buffer is cost * confidence.
//
// Layout.  One wave per current pixel, four pixels (neighbours along x) per block.  The 64 lanes are 64 / GL groups of
// GL = 16 (or 8) lanes; a group works on one depth bin at a time and its lanes split the channels in 16-byte units, so a
// tap is one contiguous read of GL * 16 bytes (256 B: 64 fp32 channels, or 128 bf16 channels) and wider feature maps take
// further passes.  The |.| sum over the channels is folded inside the group with DPP adds (no LDS).  The per-bin cost and
// count of the wave's pixel live in 1 KB of LDS private to the wave, so the reductions over D (maximum, any-missing,
// first argmin) are shuffles over the wave at the end of the same pass: nothing is re-read from memory.
#include "common.h"
#include "fsnet_hip_internal.h"

namespace {

constexpr int CV_MAX_BINS = 128;

struct CvArgs {
  const void* cur;
  const void* look;
  const float* K;
  const float* invK;
  const float* poses;
  const float* bins;
  void* cat;
  float* confidence;
  float* lowest;
  float* cost_f32;
  float* missing;
  int B, F, h, w, C, D, Ci_p;
};

template <int GL>
__device__ static inline float group_sum(float v) {   // every lane: the sum over its group of GL consecutive lanes
  v += dpp_mov<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);    // row_half_mirror: the other quad of the 8-lane half
  if (GL == 16) v += dpp_mov<0x140>(v);    // row_mirror: the other half of the 16-lane row
  return v;
}

__device__ static inline void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

template <typename T, int GL>
__global__ __launch_bounds__(256) void cost_volume_kernel(const CvArgs a) {
  constexpr int VEC = 16 / (int)sizeof(T);   // channels per lane and pass
  constexpr int NG = 64 / GL;                // depth bins in flight per wave
  constexpr int CPP = GL * VEC;              // channels per pass
  __shared__ float s_cost[4][CV_MAX_BINS];
  __shared__ float s_cnt[4][CV_MAX_BINS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane / GL, gl = lane % GL;
  const int h = a.h, w = a.w, C = a.C, D = a.D, F = a.F;
  const size_t hw = (size_t)h * w;
  const size_t pix = (size_t)blockIdx.x * 4 + wave;
  if (pix >= (size_t)a.B * hw) return;       // wave-uniform; the kernel has no block-wide barrier
  const int b = (int)(pix / hw);
  const int rem = (int)(pix - (size_t)b * hw);
  const int y = rem / w, x = rem - y * w;
  float* cost = s_cost[wave];
  float* cnt = s_cnt[wave];
  cost[lane] = 0.f; cost[lane + 64] = 0.f;
  cnt[lane] = 0.f; cnt[lane + 64] = 0.f;
  wave_lds_fence();

  const bool inside = x >= 2 && x < w - 2 && y >= 2 && y < h - 2;    // current_mask[:, 2:-2, 2:-2]
  if (inside) {
    const T* __restrict__ curp = static_cast<const T*>(a.cur) + pix * C;
    const float* __restrict__ iK = a.invK + (size_t)b * 16;
    const float* __restrict__ Km = a.K + (size_t)b * 16;
    const float fx = (float)x, fy = (float)y;
    const float r0 = iK[0] * fx + iK[1] * fy + iK[2];
    const float r1 = iK[4] * fx + iK[5] * fy + iK[6];
    const float r2 = iK[8] * fx + iK[9] * fy + iK[10];
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const float xhi = (float)(w - 2), yhi = (float)(h - 2);
    float c0[VEC];
    const int ch0 = gl * VEC;
    if (ch0 < C) loadv<T>(curp + ch0, c0);
    const int iters = (D + NG - 1) / NG;
    for (int f = 0; f < F; ++f) {
      const float* __restrict__ Tm = a.poses + ((size_t)b * F + f) * 16;
      float psum = 0.f;
      for (int i = 0; i < 16; ++i) psum += Tm[i];
      if (psum == 0.f) continue;             // a missing lookup frame (wave-uniform)
      float P[3][4];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
          P[i][j] = Km[i * 4 + 0] * Tm[j] + Km[i * 4 + 1] * Tm[4 + j] + Km[i * 4 + 2] * Tm[8 + j] + Km[i * 4 + 3] * Tm[12 + j];
      const T* __restrict__ lk = static_cast<const T*>(a.look) + ((size_t)b * F + f) * hw * C;
      for (int it = 0; it < iters; ++it) {
        const int d = it * NG + grp;
        const bool valid = d < D;
        const float dep = a.bins[valid ? d : 0];
        const float X = dep * r0, Y = dep * r1, Z = dep * r2;
        const float cx = P[0][0] * X + P[0][1] * Y + P[0][2] * Z + P[0][3];
        const float cy = P[1][0] * X + P[1][1] * Y + P[1][2] * Z + P[1][3];
        const float cz = P[2][0] * X + P[2][1] * Y + P[2][2] * Z + P[2][3];
        const float den = cz + 1e-7f;
        const float gx = (cx / den / wm1 - 0.5f) * 2.f;
        const float gy = (cy / den / hm1 - 0.5f) * 2.f;
        const float xv = (gx / 2.f + 0.5f) * wm1;
        const float yv = (gy / 2.f + 0.5f) * hm1;
        const bool ok = valid && xv >= 2.f && xv <= xhi && yv >= 2.f && yv <= yhi;    // a NaN fails
        float part = 0.f;
        if (ok) {
          const float ix = ((gx + 1.f) / 2.f) * wm1, iy = ((gy + 1.f) / 2.f) * hm1;
          const float x0f = floorf(ix), y0f = floorf(iy);
          // (the edge test keeps all four taps inside the image; the clamp only makes the addresses safe by construction)
          const int x0 = min(max((int)x0f, 0), w - 2), y0 = min(max((int)y0f, 0), h - 2);
          const float x1f = x0f + 1.f, y1f = y0f + 1.f;
          const float wnw = (x1f - ix) * (y1f - iy), wne = (ix - x0f) * (y1f - iy);
          const float wsw = (x1f - ix) * (iy - y0f), wse = (ix - x0f) * (iy - y0f);
          const T* __restrict__ t00 = lk + ((size_t)y0 * w + x0) * C;
          const T* __restrict__ t10 = t00 + (size_t)w * C;
          for (int ch = ch0; ch < C; ch += CPP) {
            float vc[VEC], nw[VEC], ne[VEC], sw[VEC], se[VEC];
            loadv<T>(t00 + ch, nw);
            loadv<T>(t00 + C + ch, ne);
            loadv<T>(t10 + ch, sw);
            loadv<T>(t10 + C + ch, se);
            if (ch == ch0) {
              for (int k = 0; k < VEC; ++k) vc[k] = c0[k];
            } else {
              loadv<T>(curp + ch, vc);
            }
            for (int k = 0; k < VEC; ++k) {
              const float wv = nw[k] * wnw + ne[k] * wne + sw[k] * wsw + se[k] * wse;
              part += fabsf(wv - vc[k]);
            }
          }
        }
        const float tot = group_sum<GL>(part);
        if (ok && gl == 0) {
          const float diff = tot / (float)C;
          cost[d] += diff;
          cnt[d] += diff > 0.f ? 1.f : 0.f;
        }
      }
    }
  }
  wave_lds_fence();

  // ---- the pixel's D bins: average, missing, maximum, confidence, first argmin (lane l: bins l and l + 64)
  float avg[2], filled[2];
  bool val[2], miss[2];
  float mx = 0.f;
  for (int k = 0; k < 2; ++k) {
    const int d = lane + 64 * k;
    val[k] = d < D;
    avg[k] = val[k] ? cost[d] / (cnt[d] + 1e-7f) : 0.f;
    miss[k] = val[k] && avg[k] == 0.f;
    mx = fmaxf(mx, avg[k]);                  // costs are >= 0
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  int any_miss = (miss[0] || miss[1]) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) any_miss |= __shfl_xor(any_miss, o);
  const float conf = any_miss ? 0.f : 1.f;
  float best = 3.0e38f;
  int best_d = CV_MAX_BINS;
  for (int k = 0; k < 2; ++k) {
    filled[k] = miss[k] ? mx : avg[k];
    const float viz = filled[k] == 0.f ? 100.f : filled[k];
    const int d = lane + 64 * k;
    if (val[k] && (viz < best || (viz == best && d < best_d))) { best = viz; best_d = d; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int od = __shfl_xor(best_d, o);
    if (ov < best || (ov == best && od < best_d)) { best = ov; best_d = od; }
  }
  T* __restrict__ dst = static_cast<T*>(a.cat) + pix * a.Ci_p + C;
  for (int k = 0; k < 2; ++k) {
    const int d = lane + 64 * k;
    if (!val[k]) continue;
    dst[d] = ElemTraits<T>::from_f(filled[k] * conf);
    if (a.cost_f32) {
      const size_t o = ((size_t)b * D + d) * hw + rem;
      a.cost_f32[o] = filled[k];
      a.missing[o] = miss[k] ? 1.f : 0.f;
    }
  }
  for (int c = D + lane; c < a.Ci_p - C; c += 64) dst[c] = ElemTraits<T>::from_f(0.f);   // the buffer's padding channels
  if (lane == 0) {
    a.confidence[pix] = conf;
    a.lowest[pix] = 1.f / a.bins[min(best_d, D - 1)];
  }
}

template <typename T>
int launch(const CvArgs& a, hipStream_t st) {
  const size_t pixels = (size_t)a.B * a.h * a.w;
  const unsigned blocks = (unsigned)((pixels + 3) / 4);
  if (a.C / (16 / (int)sizeof(T)) > 8)
    hipLaunchKernelGGL((cost_volume_kernel<T, 16>), dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((cost_volume_kernel<T, 8>), dim3(blocks), dim3(256), 0, st, a);
  return fs_launch_status();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int fs_cost_volume(const void* cur, const void* look, const float* K, const float* inv_K, const float* poses,
                              const float* bins, void* cat, float* confidence, float* lowest, float* cost_f32,
                              float* missing, int B, int F, int h, int w, int C, int D, int Ci_p, int dtype,
                              void* stream) {
  if (!cur || !look || !K || !inv_K || !poses || !bins || !cat || !confidence || !lowest) return FS_EINVAL;
  if ((cost_f32 == nullptr) != (missing == nullptr)) return FS_EINVAL;
  if (B < 1 || F < 1 || h < 5 || w < 5 || C < 16 || C % 16 || D < 1 || D > CV_MAX_BINS || Ci_p < C + D) return FS_EINVAL;
  if (dtype != FS_DTYPE_F32 && dtype != FS_DTYPE_BF16) return FS_EINVAL;
  if (!aligned16(cur) || !aligned16(look)) return FS_EINVAL;
  const int64_t pixels = (int64_t)B * h * w;
  if (pixels >= ((int64_t)1 << 31) || (int64_t)h * w * C >= ((int64_t)1 << 31)) return FS_EINVAL;
  CvArgs a;
  a.cur = cur; a.look = look; a.K = K; a.invK = inv_K; a.poses = poses; a.bins = bins; a.cat = cat;
  a.confidence = confidence; a.lowest = lowest; a.cost_f32 = cost_f32; a.missing = missing;
  a.B = B; a.F = F; a.h = h; a.w = w; a.C = C; a.D = D; a.Ci_p = Ci_p;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dtype == FS_DTYPE_BF16 ? launch<bf16>(a, st) : launch<float>(a, st);
}
