// Deformable convolution v1 / v2 (DCN, modulated DCN): forward, data-side backward and weight gradient.
//
// Replaces (reference): the CUDA extension under vision_base/networks/ops/dcn/src/cuda/ — the six kernels of
// deform_conv_cuda_kernel.cu: deformable_im2col (:84-243), deformable_col2im and deformable_col2im_coord (:280-465),
// modulated_deformable_im2col, modulated_deformable_col2im and modulated_deformable_col2im_coord (:571-866) — and the
// column-buffer GEMMs around them in deform_conv_cuda.cpp.  One template flag (V2) separates v1 (no mask) from v2 (mask).
//
// Semantics (identical for every kernel here; sample() below is the one statement of it):
//   h = ho * stride_h - pad_h + r * dil_h + offset[n][g*2RS + 2(rS+s)][ho][wo],  w likewise with channel 2(rS+s)+1
//   (:211-228, :600-616); value = 0 unless h > -1 && w > -1 && h < H && w < W (:229, :618); otherwise bilinear around
//   floor(h), floor(w) where each corner contributes only inside [0, H-1] x [0, W-1] (:89-113); v2 multiplies by
//   mask[n][g*RS + rS+s][ho][wo] (:627).  Gradients are the derivative of that expression (get_gradient_weight :118-143
//   used at :329 / :687, get_coordinate_weight :146-188 used at :427 / :755, the mask gradient :764-765; a position outside
//   the open range has none, :423 / :747).
// Offsets and masks are read as fp32 from their planar layout; x / out / dY are NHWC in the compute dtype T (bf16 or
// fp32) with padded channels, the weights are fs_pack_weights operands, every sum is fp32.
//
// All three kernels share one MFMA micro-kernel (16x16 tiles, "swapped" as in conv_igemm.hip: MFMA A = the row operand,
// B = the pixel-like operand, so a lane ends with 4 consecutive rows of one B row).  The reference's column buffer
// (Ci*R*S*M values) never exists in memory:
//   fs_dcn_fwd        A = w_f rows (co), B = columns made on the fly from four corner reads of 16 bytes each, blended in
//                     fp32 and rounded to T into LDS.  Corner offsets and blend weights (x mask) of a (pixel, tap) are
//                     computed once per deformable group into an LDS table and reused by every channel stage and by
//                     all (up to 256) output channels the block owns.
//   fs_dcn_bwd_data   d_col = dY * W^T per (group, tap, 64-channel chunk) by MFMA (A = w_d rows (ci), B = dY pixels, K over
//                     co), parked in LDS; then one wave per pixel, one lane per channel: the sample is recomputed,
//                     d_mask / d_offset are wave sums accumulated over the chunks in a fixed order and written once by
//                     their owner (no atomics), d_x takes mask * w_corner * d_col with one fp32 atomic add per lane —
//                     a wave instruction is one contiguous run of up to 64 channels (256 bytes).  blockIdx.y walks the
//                     (group, tap) pairs, so small maps still fill the chip.
//   fs_dcn_bwd_weight dW = dY^T * col with K over the pixels of a slab: both operands are transposed into LDS
//                     (pixel-contiguous), slabs go to the workspace as fp32 and an ordered reduce writes OIHW.  d_bias is
//                     the row sum of the dY^T tile, taken by the first column tile's blocks and reduced the same way
//                     (fs_channel_sum joins its blocks with float atomics: its sum is not reproducible bit for bit).
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

constexpr int DCN_P = 64;       // pixels per block (forward, data backward)
constexpr int DCN_FWD_CO = 256;  // output channels per forward block (4 tiles of 64)
constexpr int DCN_CB = 64;       // channel chunk of the backward kernels
constexpr int DCN_WG_CO = 128;   // output channels per weight-gradient block
constexpr int DCN_WG_PIX = 32;   // pixels per weight-gradient K stage

struct DcnP {
  const void* x;
  const float* offset;
  const float* mask;
  const void* w_f;
  const void* w_d;
  const float* bias;
  void* out;
  const void* dy;
  float* dx;
  float* d_offset;
  float* d_mask;
  float* ws;
  float* ws_bias;                          // weight gradient: [nsplit][Co_p] partial bias gradients, or NULL
  long w_f_row, w_d_row;
  int N, H, W, Ho, Wo, Ci, Ci_p, Co, Co_p, R, S, RS;
  int sh, sw, ph, pw, dh, dw, dg, cpg;     // cpg: channels of one deformable group in the padded buffer
  int M;
  int pps, nsplit;                         // weight gradient: pixels per slab, slabs
  int co_blk;                              // forward: output channels per block (64, 128 or 256)
};

struct Samp {
  int off[4];      // element offset of the corner's channel 0 in x, -1 = contributes nothing
  float w[4];      // bilinear weights (no mask)
  float lh, lw;
  float mask;
};

// the one statement of the sampling rule (see the header)
template <bool V2>
__device__ __forceinline__ void sample(const DcnP& p, int m, int g, int tap, Samp& s) {
  const int HoWo = p.Ho * p.Wo;
  const int n = m / HoWo;
  const int rem = m - n * HoWo;
  const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
  const int r = tap / p.S, sx = tap - r * p.S;
  const long ob = ((long)(n * p.dg + g) * 2 * p.RS + 2 * tap) * HoWo + rem;
  const float oh = p.offset[ob], ow = p.offset[ob + HoWo];
  s.mask = 1.f;
  if (V2) s.mask = p.mask[((long)(n * p.dg + g) * p.RS + tap) * HoWo + rem];
  const float h = (float)(ho * p.sh - p.ph + r * p.dh) + oh;
  const float w = (float)(wo * p.sw - p.pw + sx * p.dw) + ow;
  s.off[0] = s.off[1] = s.off[2] = s.off[3] = -1;
  s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
  s.lh = 0.f; s.lw = 0.f;
  if (!(h > -1.f && w > -1.f && h < (float)p.H && w < (float)p.W)) return;    // a NaN fails
  const float hlf = floorf(h), wlf = floorf(w);
  const int hl = (int)hlf, wl = (int)wlf, hh_i = hl + 1, wh_i = wl + 1;
  const float lh = h - hlf, lw = w - wlf, hh = 1.f - lh, hw = 1.f - lw;
  s.lh = lh; s.lw = lw;
  s.w[0] = hh * hw; s.w[1] = hh * lw; s.w[2] = lh * hw; s.w[3] = lh * lw;
  const int base = n * p.H;
  if (hl >= 0 && wl >= 0) s.off[0] = ((base + hl) * p.W + wl) * p.Ci_p;
  if (hl >= 0 && wh_i <= p.W - 1) s.off[1] = ((base + hl) * p.W + wh_i) * p.Ci_p;
  if (hh_i <= p.H - 1 && wl >= 0) s.off[2] = ((base + hh_i) * p.W + wl) * p.Ci_p;
  if (hh_i <= p.H - 1 && wh_i <= p.W - 1) s.off[3] = ((base + hh_i) * p.W + wh_i) * p.Ci_p;
}

// XOR swizzle of the 16-byte unit index of an operand row (conv_igemm.hip): conflict-free ds_read_b128 lane groups
template <int KG> __device__ __forceinline__ int swz(int row) {
  return KG == 4 ? (((row >> 3) & 1) << 1) : ((row >> 1) & 7);
}

// One K stage of the shared micro-kernel.  la: [NCT * 64 rows][KG units], lb: [64 rows][KG units]; a wave owns B rows
// wave * 16 .. + 15 and every A row: acc[ct][a][j] belongs to B row wave * 16 + li, A row ct * 64 + a * 16 + lg * 4 + j.
template <typename T, int NCT, int KG>
__device__ __forceinline__ void mma_stage(const uint4* la, const uint4* lb, f32x4 (&acc)[NCT][4], int nct, int wave,
                                          int li, int lg) {
#pragma unroll
  for (int kk = 0; kk < KG / 4; ++kk) {
    const int brow = wave * 16 + li;
    const uint4 fb = lb[brow * KG + ((kk * 4 + lg) ^ swz<KG>(brow))];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      if (ct < nct) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int arow = ct * 64 + a * 16 + li;
          const uint4 fa = la[arow * KG + ((kk * 4 + lg) ^ swz<KG>(arow))];
          if constexpr (sizeof(T) == 2) {
            acc[ct][a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa),
                                                                 __builtin_bit_cast(bf16x8, fb), acc[ct][a], 0, 0, 0);
          } else {
            const f32x4 va = __builtin_bit_cast(f32x4, fa);
            const f32x4 vb = __builtin_bit_cast(f32x4, fb);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[ct][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[j], vb[j], acc[ct][a], 0, 0, 0);
          }
        }
      }
    }
  }
}

__device__ __forceinline__ uint4 ld16(const void* base, long elem, int esz) {
  return *reinterpret_cast<const uint4*>(static_cast<const char*>(base) + elem * esz);
}

// EG blended channels of one (pixel, tap) from up to four 16-byte corner reads; wk = blend weights (mask folded in)
template <typename T>
__device__ __forceinline__ uint4 blend_unit(const void* x, const int (&off)[4], const float (&wk)[4], int c) {
  constexpr int EG = Unit<T>::N;
  float v[EG];
#pragma unroll
  for (int k = 0; k < EG; ++k) v[k] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (off[q] >= 0) {
      float xv[EG];
      Unit<T>::unpack(ld16(x, (long)off[q] + c, sizeof(T)), xv);
#pragma unroll
      for (int k = 0; k < EG; ++k) v[k] += wk[q] * xv[k];
    }
  }
  return Unit<T>::pack(v);
}

// ---------------------------------------------------------------------------------------------------------- forward
template <typename T, bool V2>
__global__ __launch_bounds__(256) void dcn_fwd_kernel(const DcnP p) {
  constexpr int EG = Unit<T>::N, KG = 4, NCT = DCN_FWD_CO / 64;
  __shared__ uint4 lds_a[2][DCN_FWD_CO * KG];
  __shared__ uint4 lds_b[2][DCN_P * KG];
  __shared__ int4 s_off[DCN_P * 9];
  __shared__ float4 s_w[DCN_P * 9];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
  const int pix0 = blockIdx.x * DCN_P, co0 = blockIdx.y * p.co_blk;
  const int nct = min(p.co_blk / 64, (p.Co_p - co0 + 63) / 64);
  const int nunits = p.cpg / EG;               // 16-byte channel units of one deformable group
  const int ncc = (nunits + KG - 1) / KG;

  f32x4 acc[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[ct][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  int st = 0;
  for (int g = 0; g < p.dg; ++g) {
    __syncthreads();
    for (int i = t; i < DCN_P * p.RS; i += 256) {
      const int pl = i / p.RS, tap = i - pl * p.RS;
      int4 o = make_int4(-1, -1, -1, -1);
      float4 wv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pix0 + pl < p.M) {
        Samp s;
        sample<V2>(p, pix0 + pl, g, tap, s);
        o = make_int4(s.off[0], s.off[1], s.off[2], s.off[3]);
        wv = make_float4(s.w[0] * s.mask, s.w[1] * s.mask, s.w[2] * s.mask, s.w[3] * s.mask);
      }
      s_off[pl * 9 + tap] = o;
      s_w[pl * 9 + tap] = wv;
    }
    __syncthreads();
    for (int tap = 0; tap < p.RS; ++tap) {
      for (int cc = 0; cc < ncc; ++cc, ++st) {
        const int buf = st & 1;
        const int u = t & 3;
        const bool uok = cc * KG + u < nunits;
        const int c = g * p.cpg + (cc * KG + u) * EG;
        {
          const int pl = t >> 2;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (uok) {
            const int4 o = s_off[pl * 9 + tap];
            const float4 wv = s_w[pl * 9 + tap];
            const int off[4] = {o.x, o.y, o.z, o.w};
            const float wk[4] = {wv.x, wv.y, wv.z, wv.w};
            v = blend_unit<T>(p.x, off, wk, c);
          }
          lds_b[buf][pl * KG + (u ^ swz<KG>(pl))] = v;
        }
#pragma unroll
        for (int q = 0; q < NCT; ++q) {
          if (q < nct) {
            const int row = q * 64 + (t >> 2);
            const int co = co0 + row;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (uok && co < p.Co_p) v = ld16(p.w_f, (long)co * p.w_f_row + (long)tap * p.Ci_p + c, sizeof(T));
            lds_a[buf][row * KG + (u ^ swz<KG>(row))] = v;
          }
        }
        __syncthreads();
        mma_stage<T, NCT, KG>(lds_a[buf], lds_b[buf], acc, nct, wave, li, lg);
      }
    }
  }

  const int m = pix0 + wave * 16 + li;
  if (m >= p.M) return;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct >= nct) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int co = co0 + ct * 64 + a * 16 + lg * 4;
      if (co >= p.Co_p) continue;
      float v[4] = {acc[ct][a][0], acc[ct][a][1], acc[ct][a][2], acc[ct][a][3]};
      if (p.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (co + j < p.Co) v[j] += p.bias[co + j];
      }
      store4<T>(static_cast<T*>(p.out) + (long)m * p.Co_p + co, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------- backward, data side
template <typename T, bool V2>
__global__ __launch_bounds__(256) void dcn_bwd_data_kernel(const DcnP p) {
  constexpr int EG = Unit<T>::N, KG = 4;
  __shared__ uint4 lds_a[2][DCN_CB * KG];
  __shared__ uint4 lds_b[2][DCN_P * KG];
  __shared__ float s_dcol[DCN_P][DCN_CB + 1];
  __shared__ float s_red[DCN_P][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
  const int pix0 = blockIdx.x * DCN_P;
  const int nchunk = (p.cpg + DCN_CB - 1) / DCN_CB;
  const int nks = (p.Co_p + KG * EG - 1) / (KG * EG);     // K stages over the output channels
  const int HoWo = p.Ho * p.Wo;
  const T* xT = static_cast<const T*>(p.x);

  int st = 0;
  // blockIdx.y walks the (group, tap) pairs: a block owns every channel of its pairs, so d_offset / d_mask keep one owner
  for (int gt = blockIdx.y; gt < p.dg * p.RS; gt += gridDim.y) {
    const int g = gt / p.RS, tap = gt - g * p.RS;
    {
      if (t < DCN_P * 3) s_red[t / 3][t % 3] = 0.f;
      for (int ch = 0; ch < nchunk; ++ch) {
        f32x4 acc[1][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[0][a] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < nks; ++ks, ++st) {
          const int buf = st & 1;
          const int row = t >> 2, u = t & 3;
          const int co = (ks * KG + u) * EG;
          const bool cok = co < p.Co_p;
          uint4 vb = make_uint4(0, 0, 0, 0), va = make_uint4(0, 0, 0, 0);
          if (cok && pix0 + row < p.M) vb = ld16(p.dy, (long)(pix0 + row) * p.Co_p + co, sizeof(T));
          const int cl = ch * DCN_CB + row;
          if (cok && cl < p.cpg) va = ld16(p.w_d, (long)(g * p.cpg + cl) * p.w_d_row + (long)tap * p.Co_p + co, sizeof(T));
          lds_b[buf][row * KG + (u ^ swz<KG>(row))] = vb;
          lds_a[buf][row * KG + (u ^ swz<KG>(row))] = va;
          __syncthreads();
          mma_stage<T, 1, KG>(lds_a[buf], lds_b[buf], acc, 1, wave, li, lg);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int j = 0; j < 4; ++j) s_dcol[wave * 16 + li][a * 16 + lg * 4 + j] = acc[0][a][j];
        __syncthreads();
        // one wave per pixel, one lane per channel of the chunk
        const int cl = ch * DCN_CB + lane;
        const bool chok = cl < p.cpg;
        const int c = g * p.cpg + cl;
        for (int q = 0; q < 16; ++q) {
          const int pl = wave * 16 + q;
          const int m = pix0 + pl;
          if (m >= p.M) break;                         // wave-uniform
          Samp s;
          sample<V2>(p, m, g, tap, s);
          const float dc = chok ? s_dcol[pl][lane] : 0.f;
          float xv[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            xv[k] = 0.f;
            if (chok && s.off[k] >= 0) {
              xv[k] = ElemTraits<T>::to_f(xT[(long)s.off[k] + c]);
              atomicAdd(p.dx + (long)s.off[k] + c, (s.mask * s.w[k]) * dc);
            }
          }
          const float hh = 1.f - s.lh, hw = 1.f - s.lw;
          const float val = s.w[0] * xv[0] + s.w[1] * xv[1] + s.w[2] * xv[2] + s.w[3] * xv[3];
          const float gh = (hw * xv[2] + s.lw * xv[3]) - (hw * xv[0] + s.lw * xv[1]);
          const float gw = (hh * xv[1] + s.lh * xv[3]) - (hh * xv[0] + s.lh * xv[2]);
          const float sm = wave_sum(dc * val), sgh = wave_sum(dc * gh), sgw = wave_sum(dc * gw);
          if (lane == 0) {
            s_red[pl][0] += sgh; s_red[pl][1] += sgw; s_red[pl][2] += sm;
          }
        }
        __syncthreads();
      }
      // owner write: thread pl < 64 owns pixel pl of this (group, tap)
      if (t < DCN_P && pix0 + t < p.M) {
        const int m = pix0 + t;
        const int n = m / HoWo, rem = m - n * HoWo;
        float mk = 1.f;
        if (V2) {
          const long mo = ((long)(n * p.dg + g) * p.RS + tap) * HoWo + rem;
          mk = p.mask[mo];
          p.d_mask[mo] = s_red[t][2];
        }
        const long ob = ((long)(n * p.dg + g) * 2 * p.RS + 2 * tap) * HoWo + rem;
        p.d_offset[ob] = mk * s_red[t][0];
        p.d_offset[ob + HoWo] = mk * s_red[t][1];
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------- weight gradient
template <typename T, bool V2>
__global__ __launch_bounds__(256) void dcn_bwd_weight_kernel(const DcnP p) {
  constexpr int EG = Unit<T>::N, NCT = DCN_WG_CO / 64;
  constexpr int KG = DCN_WG_PIX * (int)sizeof(T) / 16;       // units of one pixel-contiguous operand row
  __shared__ uint4 lds_a[2][DCN_WG_CO * KG];
  __shared__ uint4 lds_b[2][DCN_CB * KG];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
  const int nchunk = (p.cpg + DCN_CB - 1) / DCN_CB;
  int bx = blockIdx.x;
  const int ch = bx % nchunk; bx /= nchunk;
  const int tap = bx % p.RS;
  const int g = bx / p.RS;
  const int co0 = blockIdx.y * DCN_WG_CO;
  const int nct = min(NCT, (p.Co_p - co0 + 63) / 64);
  const int m0 = blockIdx.z * p.pps, m1 = min(p.M, m0 + p.pps);

  f32x4 acc[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[ct][a] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the bias gradient rides on the dY^T tile of the first column tile's blocks: thread = output channel
  const bool do_bias = p.ws_bias != nullptr && blockIdx.x == 0 && t < nct * 64;
  float bsum = 0.f;

  // element (row, k) of a pixel-contiguous operand tile
  auto put = [&](uint4* tile, int row, int k, T v) {
    const int unit = (k * (int)sizeof(T)) >> 4;
    T* base = reinterpret_cast<T*>(tile + row * KG + (unit ^ swz<KG>(row)));
    base[k & (EG - 1)] = v;
  };

  int st = 0;
  for (int ms = m0; ms < m1; ms += DCN_WG_PIX, ++st) {
    const int buf = st & 1;
    // B: col^T, rows = 64 channels of the chunk, K = 32 pixels
    for (int i = t; i < DCN_WG_PIX * (DCN_CB / EG); i += 256) {
      const int pl = i % DCN_WG_PIX, u = i / DCN_WG_PIX;
      const int cl = ch * DCN_CB + u * EG;
      float v[EG];
#pragma unroll
      for (int k = 0; k < EG; ++k) v[k] = 0.f;
      if (ms + pl < m1 && cl < p.cpg) {
        Samp s;
        sample<V2>(p, ms + pl, g, tap, s);
        const float wk[4] = {s.w[0] * s.mask, s.w[1] * s.mask, s.w[2] * s.mask, s.w[3] * s.mask};
        Unit<T>::unpack(blend_unit<T>(p.x, s.off, wk, g * p.cpg + cl), v);
      }
#pragma unroll
      for (int k = 0; k < EG; ++k) put(lds_b[buf], u * EG + k, pl, ElemTraits<T>::from_f(v[k]));
    }
    // A: dY^T, rows = output channels, K = 32 pixels
    for (int i = t; i < DCN_WG_PIX * (nct * 64 / EG); i += 256) {
      const int pl = i % DCN_WG_PIX, u = i / DCN_WG_PIX;
      const int co = co0 + u * EG;
      float v[EG];
#pragma unroll
      for (int k = 0; k < EG; ++k) v[k] = 0.f;
      if (ms + pl < m1 && co < p.Co_p) Unit<T>::unpack(ld16(p.dy, (long)(ms + pl) * p.Co_p + co, sizeof(T)), v);
#pragma unroll
      for (int k = 0; k < EG; ++k) put(lds_a[buf], u * EG + k, pl, ElemTraits<T>::from_f(v[k]));
    }
    __syncthreads();
    if (do_bias) {
      // the stage's 32 values as a balanced tree (pairs, units, stage), then one add per stage: the error of a long
      // running sum would dominate this gradient's budget
      float us[KG];
#pragma unroll
      for (int u = 0; u < KG; ++u) {
        float v[EG];
        Unit<T>::unpack(lds_a[buf][t * KG + (u ^ swz<KG>(t))], v);
#pragma unroll
        for (int w = 1; w < EG; w *= 2)
#pragma unroll
          for (int k = 0; k < EG; k += 2 * w) v[k] += v[k + w];
        us[u] = v[0];
      }
#pragma unroll
      for (int w = 1; w < KG; w *= 2)
#pragma unroll
        for (int u = 0; u < KG; u += 2 * w) us[u] += us[u + w];
      bsum += us[0];
    }
    mma_stage<T, NCT, KG>(lds_a[buf], lds_b[buf], acc, nct, wave, li, lg);
  }
  if (do_bias && co0 + t < p.Co_p) p.ws_bias[(long)blockIdx.z * p.Co_p + co0 + t] = bsum;

  // slab [split][Co_p][RS * Ci_p]
  const int cl = ch * DCN_CB + wave * 16 + li;
  if (cl >= p.cpg) return;
  const long ktot = (long)p.RS * p.Ci_p;
  const long kcol = (long)tap * p.Ci_p + g * p.cpg + cl;
  float* slab = p.ws + (long)blockIdx.z * p.Co_p * ktot;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct >= nct) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = co0 + ct * 64 + a * 16 + lg * 4 + j;
        if (co < p.Co_p) slab[(long)co * ktot + kcol] = acc[ct][a][j];
      }
  }
}

// dw[co][ci][r][s] = sum over the slabs, in slab order; the threads behind them: d_bias[co] likewise
__global__ __launch_bounds__(256) void dcn_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                               const float* __restrict__ ws_bias,
                                                               float* __restrict__ d_bias, int nsplit, int Co, int Ci,
                                                               int RS, int Co_p, int Ci_p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)Co * Ci * RS;
  if (i >= total) {
    if (d_bias && i - total < Co) {
      float s = 0.f;
      for (int z = 0; z < nsplit; ++z) s += ws_bias[(long)z * Co_p + (i - total)];
      d_bias[i - total] = s;
    }
    return;
  }
  const int tap = (int)(i % RS);
  const long q = i / RS;
  const int ci = (int)(q % Ci), co = (int)(q / Ci);
  const long ktot = (long)RS * Ci_p;
  const long e = (long)co * ktot + (long)tap * Ci_p + ci;
  const long slab = (long)Co_p * ktot;
  float s = 0.f;
  for (int z = 0; z < nsplit; ++z) s += ws[z * slab + e];
  dw[i] = s;
}

// ------------------------------------------------------------------------------------------------------------- host
int out_extent(int in, int pad, int dil, int k, int stride) { return (in + 2 * pad - (dil * (k - 1) + 1)) / stride + 1; }

// everything but the pointers; fills the geometry of p
int check_geometry(const FsDcnArgs* a, int dtype, DcnP& p) {
  if (!a) return FS_EINVAL;
  if (dtype != FS_DTYPE_F32 && dtype != FS_DTYPE_BF16) return FS_EINVAL;
  const int eg = dtype == FS_DTYPE_BF16 ? 8 : 4;
  if (a->groups != 1) return FS_EINVAL;
  if (a->R < 1 || a->R > 3 || a->S < 1 || a->S > 3) return FS_EINVAL;
  if ((a->stride_h != 1 && a->stride_h != 2) || (a->stride_w != 1 && a->stride_w != 2)) return FS_EINVAL;
  if (a->pad_h < 0 || a->pad_w < 0 || a->pad_h > 64 || a->pad_w > 64) return FS_EINVAL;
  if (a->dil_h < 1 || a->dil_w < 1 || a->dil_h > 64 || a->dil_w > 64) return FS_EINVAL;
  if (a->N < 1 || a->H < 1 || a->W < 1 || a->Ci < 1 || a->Co < 1) return FS_EINVAL;
  if (a->Ci_p < a->Ci || a->Ci_p % eg != 0 || a->Co_p < a->Co || a->Co_p % 16 != 0) return FS_EINVAL;
  const int dg = a->deformable_groups;
  if (dg < 1 || a->Ci % dg != 0) return FS_EINVAL;
  if (dg > 1 && (a->Ci_p != a->Ci || (a->Ci / dg) % eg != 0)) return FS_EINVAL;
  if ((int64_t)a->H + 2 * a->pad_h < (int64_t)a->dil_h * (a->R - 1) + 1) return FS_EINVAL;
  if ((int64_t)a->W + 2 * a->pad_w < (int64_t)a->dil_w * (a->S - 1) + 1) return FS_EINVAL;
  if (a->Ho != out_extent(a->H, a->pad_h, a->dil_h, a->R, a->stride_h)) return FS_EINVAL;
  if (a->Wo != out_extent(a->W, a->pad_w, a->dil_w, a->S, a->stride_w)) return FS_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t M = (int64_t)a->N * a->Ho * a->Wo;
  const int RS = a->R * a->S;
  if ((int64_t)a->N * a->H * a->W * a->Ci_p >= lim || M * a->Co_p >= lim || M * dg * 2 * RS >= lim) return FS_EINVAL;
  if ((int64_t)a->Co_p * RS * a->Ci_p >= lim) return FS_EINVAL;
  p.N = a->N; p.H = a->H; p.W = a->W; p.Ho = a->Ho; p.Wo = a->Wo;
  p.Ci = a->Ci; p.Ci_p = a->Ci_p; p.Co = a->Co; p.Co_p = a->Co_p; p.R = a->R; p.S = a->S; p.RS = RS;
  p.sh = a->stride_h; p.sw = a->stride_w; p.ph = a->pad_h; p.pw = a->pad_w; p.dh = a->dil_h; p.dw = a->dil_w;
  p.dg = dg; p.cpg = a->Ci_p / dg;
  p.M = (int)M;
  // weight-gradient slabs: enough blocks to fill the chip, whole K stages per slab, a fixed function of the shape
  const int tiles = dg * RS * ((p.cpg + DCN_CB - 1) / DCN_CB) * ((p.Co_p + DCN_WG_CO - 1) / DCN_WG_CO);
  const int stages = (p.M + DCN_WG_PIX - 1) / DCN_WG_PIX;
  int want = (1024 + tiles - 1) / tiles;
  want = std::max(1, std::min(std::min(want, 256), (stages + 3) / 4));
  const int sps = (stages + want - 1) / want;
  p.pps = sps * DCN_WG_PIX;
  p.nsplit = (stages + sps - 1) / sps;
  // forward: a block reuses its gathered columns for up to 256 output channels; with few pixel tiles the channels are
  // spread over more blocks instead (the gather is repeated, the chip is filled)
  const int ptiles = (p.M + DCN_P - 1) / DCN_P;
  p.co_blk = DCN_FWD_CO;
  while (p.co_blk > 64 && (long)ptiles * ((p.Co_p + p.co_blk - 1) / p.co_blk) < 256) p.co_blk /= 2;
  return FS_OK;
}

bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

int fill_common(const FsDcnArgs* a, int dtype, DcnP& p) {
  const int r = check_geometry(a, dtype, p);
  if (r != FS_OK) return r;
  if (!a->x || !a->offset || !al16(a->x)) return FS_EINVAL;
  p.x = a->x; p.offset = a->offset; p.mask = a->mask; p.w_f = a->w_f; p.w_d = a->w_d; p.bias = a->bias;
  p.out = a->out; p.dy = a->dy; p.dx = a->dx; p.d_offset = a->d_offset; p.d_mask = a->d_mask;
  p.ws = static_cast<float*>(a->workspace);
  p.ws_bias = nullptr;
  p.w_f_row = a->w_f_row; p.w_d_row = a->w_d_row;
  return FS_OK;
}

}  // namespace

extern "C" int fs_dcn_tile(int which, int32_t* pixels, int32_t* channels) {
  if (!pixels || !channels || which < 0 || which > 2) return FS_EINVAL;
  if (which == 0) { *pixels = DCN_P; *channels = DCN_FWD_CO; }
  if (which == 1) { *pixels = DCN_P; *channels = DCN_CB; }
  if (which == 2) { *pixels = DCN_WG_PIX; *channels = DCN_WG_CO; }
  return FS_OK;
}

extern "C" int fs_dcn_fwd_channels(const FsDcnArgs* args, int dtype) {
  DcnP p;
  if (check_geometry(args, dtype, p) != FS_OK) return -1;
  return p.co_blk;
}

// dW slabs, then the bias-gradient partials
static int64_t slab_floats(const DcnP& p) { return (int64_t)p.nsplit * p.Co_p * p.RS * p.Ci_p; }

extern "C" int64_t fs_dcn_workspace_bytes(const FsDcnArgs* args, int dtype) {
  DcnP p;
  if (check_geometry(args, dtype, p) != FS_OK) return -1;
  return (slab_floats(p) + (int64_t)p.nsplit * p.Co_p) * (int64_t)sizeof(float);
}

extern "C" int fs_dcn_fwd(const FsDcnArgs* args, int dtype, void* stream) {
  DcnP p;
  int r = fill_common(args, dtype, p);
  if (r != FS_OK) return r;
  const int eg = dtype == FS_DTYPE_BF16 ? 8 : 4;
  if (!p.w_f || !p.out || !al16(p.w_f) || !al16(p.out)) return FS_EINVAL;
  if (p.w_f_row < (long)p.RS * p.Ci_p || p.w_f_row % eg != 0) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((p.M + DCN_P - 1) / DCN_P, (p.Co_p + p.co_blk - 1) / p.co_blk);
  const bool v2 = p.mask != nullptr;
  if (dtype == FS_DTYPE_BF16) {
    if (v2) hipLaunchKernelGGL((dcn_fwd_kernel<bf16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_fwd_kernel<bf16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (v2) hipLaunchKernelGGL((dcn_fwd_kernel<float, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_fwd_kernel<float, false>), grid, dim3(256), 0, st, p);
  }
  return fs_launch_status();
}

extern "C" int fs_dcn_bwd_data(const FsDcnArgs* args, int dtype, void* stream) {
  DcnP p;
  int r = fill_common(args, dtype, p);
  if (r != FS_OK) return r;
  const int eg = dtype == FS_DTYPE_BF16 ? 8 : 4;
  if (!p.w_d || !p.dy || !p.dx || !p.d_offset || !al16(p.w_d) || !al16(p.dy)) return FS_EINVAL;
  if ((p.mask != nullptr) != (p.d_mask != nullptr)) return FS_EINVAL;
  if (p.w_d_row < (long)p.RS * p.Co_p || p.w_d_row % eg != 0) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(p.dx, 0, (size_t)p.N * p.H * p.W * p.Ci_p * sizeof(float), st) != hipSuccess) return FS_ELAUNCH;
  const dim3 grid((p.M + DCN_P - 1) / DCN_P, std::min(p.dg * p.RS, 65535));
  const bool v2 = p.mask != nullptr;
  if (dtype == FS_DTYPE_BF16) {
    if (v2) hipLaunchKernelGGL((dcn_bwd_data_kernel<bf16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_bwd_data_kernel<bf16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (v2) hipLaunchKernelGGL((dcn_bwd_data_kernel<float, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_bwd_data_kernel<float, false>), grid, dim3(256), 0, st, p);
  }
  return fs_launch_status();
}

extern "C" int fs_dcn_bwd_weight(const FsDcnArgs* args, int dtype, void* stream) {
  DcnP p;
  int r = fill_common(args, dtype, p);
  if (r != FS_OK) return r;
  if (!p.dy || !args->dw || !p.ws || !al16(p.dy)) return FS_EINVAL;
  if (args->workspace_bytes < fs_dcn_workspace_bytes(args, dtype)) return FS_EINVAL;
  p.ws_bias = args->d_bias ? p.ws + slab_floats(p) : nullptr;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nchunk = (p.cpg + DCN_CB - 1) / DCN_CB;
  const dim3 grid(p.dg * p.RS * nchunk, (p.Co_p + DCN_WG_CO - 1) / DCN_WG_CO, p.nsplit);
  const bool v2 = p.mask != nullptr;
  if (dtype == FS_DTYPE_BF16) {
    if (v2) hipLaunchKernelGGL((dcn_bwd_weight_kernel<bf16, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_bwd_weight_kernel<bf16, false>), grid, dim3(256), 0, st, p);
  } else {
    if (v2) hipLaunchKernelGGL((dcn_bwd_weight_kernel<float, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((dcn_bwd_weight_kernel<float, false>), grid, dim3(256), 0, st, p);
  }
  r = fs_launch_status();
  if (r != FS_OK) return r;
  const long total = (long)p.Co * p.Ci * p.RS;
  hipLaunchKernelGGL(dcn_wgrad_reduce_kernel, dim3((unsigned)((total + p.Co + 255) / 256)), dim3(256), 0, st, p.ws,
                     args->dw, p.ws_bias, args->d_bias, p.nsplit, p.Co, p.Ci, p.RS, p.Co_p, p.Ci_p);
  return fs_launch_status();
}
