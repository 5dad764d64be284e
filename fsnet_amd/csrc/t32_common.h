// Pieces of the 32x32-MFMA-tile 3x3 convolution kernels (conv3x3_t32.hip, conv3x3_s2d.hip) on top of conv_epi.h: operand
// units, the v_permlane32_swap accumulator transposition and the halving statistics reduction.
#pragma once
#include "conv_epi.h"
#include <cstdlib>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ void t32_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

struct T32Geom {
  int TH, TW;
  int tiles_x, tiles_y;
  unsigned mTW, mHW;
  FsDiv dTX, dTY;
  FsDiv dIPG;      // images per BatchNorm statistics group
  FsDiv dPRG;      // images per prologue coefficient group
  int pix_major;
};

enum : int { EP_BIAS = 1, EP_ADDEND = 2, EP_RELU = 4, EP_MASK = 8, EP_STATS = 16, EP_BNB = 32, EP_F32 = 64,
             EP_MASKBN = 128 };

template <typename T> struct Mma32;
template <> struct Mma32<bf16> {
  static __device__ __forceinline__ void run(f32x16& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
};
template <> struct Mma32<float> {
  static __device__ __forceinline__ void run(f32x16& acc, const uint4& a, const uint4& b) {
    const f32x4 va = __builtin_bit_cast(f32x4, a), vb = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[j], vb[j], acc, 0, 0, 0);
  }
};

#define T32_FLAG(bit, rt) (EP < 0 ? (rt) : ((EP & (bit)) != 0))

constexpr int t32_hmax(int PIX) { return PIX == 256 ? 360 : 208; }
constexpr int t32_lds_units(int PIX, int CO) { return t32_hmax(PIX) * 5 + 9 * CO * 4; }
// blocks per CU the LDS footprint admits (= waves per SIMD: a block is one wave per SIMD)
constexpr int t32_occupancy(int PIX, int CO) {
  return 163840 / (t32_lds_units(PIX, CO) * 16) > 4 ? 4 : 163840 / (t32_lds_units(PIX, CO) * 16);
}

// v_permlane32_swap: lanes 32-63 of `lo_dst` <-> lanes 0-31 of `hi_src` (checked on the device:
// tools/probes/permlane_probe.hip).  Inline asm because hipcc (ROCm 7.2) loses the instruction's second result when
// both come back into elements of an accumulator tuple — it re-uses the tied source register without copying it out
// (seen in the ISA; every second channel quad of the output was garbage).  hipcc pads nothing inside an asm
// statement: the s_nop before covers a VALU write of either operand right in front of it, the one after a read of
// the results right behind.
__device__ __forceinline__ void t32_swap32(float& lo_dst, float& hi_src) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo_dst), "+v"(hi_src));
}
// Sum of 16 per-lane values over the 32 lanes of a wave half, by a halving exchange: in each of four steps a lane
// keeps half of its values, hands the other half to a partner that keeps exactly those, and adds what it receives —
// 8 + 4 + 2 + 1 DPP adds instead of 16 x 5 for sixteen full butterflies (the statistics reduction was 390 of the 553
// vector instructions of an epilogue).  Partners: row_mirror (lane i <-> 15 - i), row_half_mirror (i <-> 7 - i),
// quad_perm xor 2, xor 1 — each flips the selecting lane bit and none of the bits used before it.  A last exchange
// (v_permlane16_swap) adds the two 16-lane rows of the half.  Every lane ends up with the total of ONE input index:
// idx = 8*(lane & 1) + 4*((lane >> 1) & 1) + 2*((lane >> 2) & 1) + ((lane >> 3) & 1).
template <int CTRL>
__device__ __forceinline__ float t32_xadd(float keep, float send) {
  return keep + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), CTRL, 0xf, 0xf, true));
}
// (the four row-level steps alone: the sum over the 16 lanes of a DPP row)
__device__ __forceinline__ float t32_reduce16_row(const float* v, int lane) {
  const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
  float w8[8], w4[4], w2[2];
#pragma unroll
  for (int k = 0; k < 8; ++k) w8[k] = t32_xadd<0x140>(b3 ? v[2 * k + 1] : v[2 * k], b3 ? v[2 * k] : v[2 * k + 1]);
#pragma unroll
  for (int k = 0; k < 4; ++k) w4[k] = t32_xadd<0x141>(b2 ? w8[2 * k + 1] : w8[2 * k], b2 ? w8[2 * k] : w8[2 * k + 1]);
#pragma unroll
  for (int k = 0; k < 2; ++k) w2[k] = t32_xadd<0x4E>(b1 ? w4[2 * k + 1] : w4[2 * k], b1 ? w4[2 * k] : w4[2 * k + 1]);
  return t32_xadd<0xB1>(b0 ? w2[1] : w2[0], b0 ? w2[0] : w2[1]);
}
__device__ __forceinline__ float t32_reduce16(const float* v, int lane) {
  const float w1 = t32_reduce16_row(v, lane);
  // rows 1, 3 of x <-> rows 0, 2 of y (inline asm for the same reason as t32_swap32)
  float x = w1, y = w1;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
  return w1 + ((lane & 16) ? x : y);
}

struct T32Item { int n, y0, x0, co0, px; };

// scheduling groups of one pipelined k-step: NR fragment reads spread evenly between its NM MFMAs
template <int NR, int NM, int K = 0>
__device__ __forceinline__ void t32_sched_step() {
  if constexpr (K < NR) {
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    constexpr int m = (NM * (K + 1)) / NR - (NM * K) / NR;
    if constexpr (m > 0) __builtin_amdgcn_sched_group_barrier(0x008, m, 0);
    t32_sched_step<NR, NM, K + 1>();
  }
}

// pixel tile (conv_epi.h): a 2-pixel halo border, 32-wide tiles preferred
inline T32Geom t32_pick_geom(int Hd, int Wd, int PIX, int hmax) { return conv_pick_tile<T32Geom>(Hd, Wd, PIX, hmax, 2, true); }

inline int t32_ep_mask(const FsConvArgs& a) {
  int m = 0;
  if (a.bias) m |= EP_BIAS;
  if (a.addend) m |= EP_ADDEND;
  if (a.relu) m |= EP_RELU;
  if (a.mask) m |= EP_MASK;
  if (a.bnb_x) m |= EP_BNB;
  else if (a.stats) m |= EP_STATS;
  if (a.out_f32) m |= EP_F32;
  if (a.bnb_x && a.bnb_scale) m |= EP_MASKBN;
  return m;
}

}  // namespace
