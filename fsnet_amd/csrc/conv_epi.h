// What the forward / data-gradient convolution kernels share outside their main loops (conv_igemm.hip, conv1x1.hip,
// conv1x1_gemm.hip, conv3x3_halo.hip, conv3x3_p1.hip, conv3x3_t32.hip, conv3x3_s2d.hip, conv_stem.hip), stated once:
//   * the operand load, the LDS-only barrier, the block -> (pixel tile, channel tile) mapping and its host twin;
//   * the epilogue's value pipeline of the 32x32-layout kernels (epi_value: bias, addend, ReLU, ReLU-backward mask,
//     derived BatchNorm mask, then the statistics or BatchNorm-backward sums, on 8 channels of a pixel read back through
//     LDS).  Offsets and the store stay with the kernel;
//   * the block's statistics tail (epi_row_sums, epi_stats_tail): 16 pixel lanes by DPP, the pixel waves through LDS,
//     ONE f64 atomic per channel and moment into slot `tile % FS_STAT_SLOTS` of the tile's statistics group
//     (same-address atomics cost ~12 ns each on MI355X; slots + block reduce keep the chain per address short);
//   * the host's pixel-tile picker (conv_pick_tile) and the grid of a tiled launch (conv_tile_grid).
// DESIGN section 24 has the resource table and what was kept per kernel.  Reference semantics: nn.Conv2d (+ bias, the
// residual add and ReLU of resnet.py:33-50) and the autograd backward of the ReLU / BatchNorm behind it.
#pragma once
#include "common.h"
#include "fsnet_hip_internal.h"
#include <algorithm>

namespace {

__device__ __forceinline__ uint4 conv_load16(__amdgpu_buffer_rsrc_t rsrc, int voff) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
}

// workgroup barrier that orders LDS traffic only.  __syncthreads() also carries a workgroup-scope fence, which on
// gfx9 is `s_waitcnt vmcnt(0)`: every barrier then waits for the block's outstanding global loads AND stores (one
// L2 round trip per barrier — PMC on the layer-1 shapes: waves parked 58 % of their cycles).  LDS hand-offs between
// the waves of a block only need the DS counter drained.
__device__ __forceinline__ void conv_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// XCD-aware tile mapping (block b runs on XCD b % 8, each XCD has a private 4 MB L2): all pixel tiles of one channel
// tile go to the same XCD(s), so a weight tile is fetched from HBM/MALL once per XCD and then hit in L2.  pix_major
// (activations outweigh the weights: layer 1 / 2, the decoder): the channel tiles of ONE pixel tile run on the same XCD
// in consecutive slots instead, so the halo is fetched across the fabric once and re-read from that L2.
// false: the block is padding of the grid (conv_xcd_blocks rounds up).
__device__ __forceinline__ bool conv_xcd_tile(int bid, int nco, int npix, int pix_major, int& px, int& cy) {
  const int xcd = bid & 7, slot = bid >> 3;
  if (pix_major) { cy = slot % nco; px = (slot / nco) * 8 + xcd; }
  else if (nco % 8 == 0) { const int q = nco >> 3; cy = xcd + 8 * (slot % q); px = slot / q; }
  else if (8 % nco == 0) { const int q = 8 / nco; cy = xcd % nco; px = slot * q + xcd / nco; }
  else { cy = bid % nco; px = bid / nco; }
  return px < npix;
}
// blocks of the grid that conv_xcd_tile decodes
inline int conv_xcd_blocks(int npix, int nco, int pix_major) {
  if (pix_major) return 8 * ((npix + 7) / 8) * nco;
  if (nco % 8 != 0 && 8 % nco == 0) { const int q = 8 / nco; return 8 * ((npix + q - 1) / q); }
  return npix * nco;
}

inline int conv_cu_count() {
  static const int n = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t pr;
      if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) cus = pr.multiProcessorCount;
    }
    return cus;
  }();
  return n;
}

// ---- NV = 4 / 8 consecutive channels of one pixel <-> floats ----
template <typename T> __device__ __forceinline__ void load8(const T* p, float* v);
template <> __device__ __forceinline__ void load8<bf16>(const bf16* p, float* v) {
  Unit<bf16>::unpack(*reinterpret_cast<const uint4*>(p), v);
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float* v);
template <> __device__ __forceinline__ void store8<bf16>(bf16* p, const float* v) {
  *reinterpret_cast<uint4*>(p) = Unit<bf16>::pack(v);
}
template <> __device__ __forceinline__ void store8<float>(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <typename T, int NV> __device__ __forceinline__ void epi_load(const T* p, float* v) {
  if constexpr (NV == 4) load4<T>(p, v); else load8<T>(p, v);
}

// the channel-only operands of a lane's NV channels; the kernel loads what its options need, once per channel tile
template <int NV> struct EpiCh { float bias[NV], scale[NV], shift[NV]; };
template <int NV> __device__ __forceinline__ void epi_load_ch(const float* p, float (&v)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; j += 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + j);
    v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
  }
}

// Epilogue options as plain bools: compile-time constants fold (T32_FLAG).
//   bias   add k.bias (a kernel that adds a zero vector when there is none says true: x + 0 is not x for x = -0)
//   add    + addend            relu   max(v, 0)
//   mask   ReLU backward of the producing layer: pass the gradient where its output was > 0
//   bnb    BatchNorm-backward sums of the layer this gradient flows into (bnb_x = its input, laid out as dst)
//   mbn    (with bnb) ReLU mask of a folded BatchNorm: the sign of the forward prologue's own expression
//   stats  (without bnb) output statistics (sum v, sum v^2)
struct EpiOpt { bool bias, add, relu, mask, bnb, mbn, stats; };

// The value pipeline of NV consecutive channels of one pixel, as the kernels that read their accumulators back through
// LDS run it (conv3x3_t32.hip, conv3x3_s2d.hip: NV = 8).  BatchNorm-backward sums in the f64 form: s2 += v * x here,
// epi_stats_tail forms (sum v x - mean sum v) invstd.  (The 16x16-layout kernels add v * (x - mean) * invstd per element
// in fp32 instead — different arithmetic that stays; they keep their 4-channel pipeline in their own lines, DESIGN section
// 24 says why.)  addend / mask / bnb_x are the tensors' base pointers and aoff / moff / xoff the element offsets of the
// lane's first channel; only the enabled ones are read.
template <typename T, int NV>
__device__ __forceinline__ void epi_value(float (&v)[NV], const EpiOpt o, const EpiCh<NV>& k, const void* addend, long aoff,
                                          const void* mask, long moff, const void* bnb_x, long xoff, float (&s1)[NV],
                                          float (&s2)[NV]) {
  if (o.bias) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] += k.bias[j];
  }
  if (o.add) {
    float av[NV];
    epi_load<T, NV>(reinterpret_cast<const T*>(addend) + aoff, av);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] += av[j];
  }
  if (o.relu) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = fmaxf(v[j], 0.f);
  }
  if (o.mask) {
    float mv[NV];
    epi_load<T, NV>(reinterpret_cast<const T*>(mask) + moff, mv);
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = mv[j] > 0.f ? v[j] : 0.f;
  }
  if (o.bnb) {
    float cv[NV];
    epi_load<T, NV>(reinterpret_cast<const T*>(bnb_x) + xoff, cv);
    if (o.mbn) {
#pragma unroll
      for (int j = 0; j < NV; ++j) v[j] = (cv[j] * k.scale[j] + k.shift[j]) > 0.f ? v[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) { s1[j] += v[j]; s2[j] += v[j] * cv[j]; }
  } else if (o.stats) {
#pragma unroll
    for (int j = 0; j < NV; ++j) { s1[j] += v[j]; s2[j] += v[j] * v[j]; }
  }
}

// 16x16 layout: the sums of the 16 pixel lanes of each channel (DPP, no LDS) into this wave's row red[CO][2];
// cbase = the wave's first channel inside the block's channel tile
template <int TC>
__device__ __forceinline__ void epi_row_sums(const float (&s1)[TC][4], const float (&s2)[TC][4], float* red, int cbase,
                                             int li, int lg) {
#pragma unroll
  for (int a = 0; a < TC; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float u = row16_sum(s1[a][j]), w = row16_sum(s2[a][j]);
      if (li == 0) {
        const int cl = cbase + a * 16 + lg * 4 + j;
        red[cl * 2] = u; red[cl * 2 + 1] = w;
      }
    }
}

// slot of statistics group sg that pixel tile `tile` adds to
__device__ __forceinline__ double* epi_stat_slot(double* stats, long sg, int tile, int Co) {
  return stats + (sg * FS_STAT_SLOTS + tile % FS_STAT_SLOTS) * 2 * Co;
}

// red[WP][CO][2] (complete behind a barrier of the caller's) -> the two f64 atomics of channel co0 + t.
// mean != nullptr: the second sum is (sum v x) and leaves as (sum v x - mean sum v) invstd, formed in f64.
template <int CO, int WP>
__device__ __forceinline__ void epi_stats_tail(const float* red, int t, int co0, int Co, double* stats, long sg, int tile,
                                               const float* mean = nullptr, const float* invstd = nullptr) {
  if (t < CO) {
    float u = 0.f, w = 0.f;
#pragma unroll
    for (int k = 0; k < WP; ++k) { u += red[(k * CO + t) * 2]; w += red[(k * CO + t) * 2 + 1]; }
    const int co = co0 + t;
    if (co < Co) {
      double* sl = epi_stat_slot(stats, sg, tile, Co);
      double wd = (double)w;
      if (mean) wd = (wd - (double)mean[sg * Co + co] * (double)u) * (double)invstd[sg * Co + co];
      atomicAdd(sl + co, (double)u);
      atomicAdd(sl + Co + co, wd);
    }
  }
}

// ---- host: the pixel tile of the LDS-halo kernels ----
// TH x TW <= PIX output pixels whose (TH + border) x (TW + border) halo fits hmax slots, chosen by
// cost = (MFMA lanes spent per useful pixel) * (1 + 0.15 * halo fetch overhead); prefer32: 2 % against widths that are
// neither a multiple of 32 nor the whole row (a 32-pixel MFMA tile that is one image row reads its halo conflict-free).
// G: the kernel's geometry struct (TH, TW, tiles_x, tiles_y, mTW, mHW, dTX, dTY + its own fields, zeroed); TH = 0: none fits.
template <typename G>
inline G conv_pick_tile(int Hd, int Wd, int PIX, int hmax, int border, bool prefer32) {
  G best{};
  double best_cost = 1e30;
  for (int tw = std::min(4, Wd); tw <= std::min(Wd, 64); ++tw) {
    const int th = std::min(PIX / tw, Hd);
    if (th < 1 || (th + border) * (tw + border) > hmax) continue;
    const int tx = (Wd + tw - 1) / tw, ty = (Hd + th - 1) / th;
    const double waste = (double)tx * ty * PIX / ((double)Hd * Wd);
    const double halo = (double)(th + border) * (tw + border) / ((double)th * tw);
    double cost = waste * (1.0 + 0.15 * halo);
    if (prefer32 && tw % 32 != 0 && tw != Wd) cost *= 1.02;
    if (cost < best_cost - 1e-9) { best_cost = cost; best.TH = th; best.TW = tw; best.tiles_x = tx; best.tiles_y = ty; }
  }
  if (best.TW > 0) {
    best.mTW = fs_div_magic(best.TW); best.mHW = fs_div_magic(best.TW + border);
    best.dTX = fs_make_div(best.tiles_x); best.dTY = fs_make_div(best.tiles_y);
  }
  return best;
}

// images per BatchNorm statistics group of a launch whose groups are whole images; false: they are not
inline bool conv_stat_group_div(const FsConvArgs& a, FsDiv& dIPG) {
  if (a.stat_group_rows <= 0) return true;
  const long hw = (long)a.Hd * a.Wd;
  if (a.stat_group_rows % hw != 0) return false;
  dIPG = fs_make_div((int)(a.stat_group_rows / hw));
  return true;
}

// the rest of a picked geometry (dIPG, pix_major) and the grid; 0 blocks: the arguments do not fit this tiling
template <typename G>
inline int conv_tile_grid(const FsConvArgs& a, G& g, int CO) {
  if (g.TH == 0 || !conv_stat_group_div(a, g.dIPG)) return 0;
  const int npix = a.N * g.tiles_x * g.tiles_y, nco = a.Co_p / CO;
  // which operand is worth keeping XCD-local: the input activation (fetched once per channel tile) or the weights
  g.pix_major = (nco > 1 && a.src_bytes > 2 * a.wgt_bytes) ? 1 : 0;
  return conv_xcd_blocks(npix, nco, g.pix_major);
}

}  // namespace
