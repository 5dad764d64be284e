// Operand prologue of the 3x3 / stride-1 LDS-halo convolution kernels (conv3x3_t32.hip, conv3x3_halo.hip): the
// BatchNorm (+ ReLU) in front of a convolution (pro_mode 1), applied to 16-byte units while they travel from the load
// registers to LDS.  FsConvArgs documents it (include/fsnet_hip.h).  (Mode 2 — the second pass of the backward of the
// BatchNorm behind the convolution, in the data gradient's staging — existed in rounds 3-4, measured slower and is gone.)  The per-channel coefficients live in a small LDS table that every block fills itself — from
// the f64 sums the producing kernel's epilogue left (bn_coeffs.h: the arithmetic of bn_apply_kernel's preamble,
// bn.hip: no fs_bn_finalize launch and no BatchNorm pass between two convolutions), or from coefficient arrays
// handed in.  Reference: nn.BatchNorm2d in train mode between conv1 and conv2 of a BasicBlock and its autograd
// backward, vision_base/networks/models/backbone/resnet.py:33-50.
#pragma once
#include "bn_coeffs.h"

namespace {

template <int PRO> constexpr int pro_ncoef() { return PRO == 1 ? 2 : 0; }
// dynamic LDS a launch with this prologue needs
template <int PRO> inline unsigned pro_lds_bytes(const FsConvArgs& a) { return (unsigned)(pro_ncoef<PRO>() * a.Cs * sizeof(float)); }

// mode 1, channel c of statistics group g (bn_coeffs.h: the arithmetic bn.hip's kernels use)
__device__ inline BnCoeffs pro1_channel(const FsConvArgs& p, int g, int c) {
  const int C = p.Cs;
  double s1, s2, m, v;
  bn_sum_slots(p.pro_stats + (long)g * FS_STAT_SLOTS * 2 * C, C, c, s1, s2);
  bn_moments(s1, s2, p.pro_count, m, v);
  return bn_coeffs(m, v, p.pro_eps, p.pro_gamma[c], p.pro_beta[c]);
}

// fills tab[ncoef][Cs] for statistics group grp (all threads of the block; a barrier must follow before it is read)
template <int PRO>
__device__ inline void pro_build_table(const FsConvArgs& p, float* tab, int grp, int t, int nt) {
  const int C = p.Cs;
  if (p.pro_stats) {
    for (int c = t; c < C; c += nt) {
      const BnCoeffs k = pro1_channel(p, grp, c);
      tab[c] = k.scale; tab[C + c] = k.shift;
    }
  } else {
    for (int c = t; c < C; c += nt) { tab[c] = p.pro_a[grp * C + c]; tab[C + c] = p.pro_b[grp * C + c]; }
  }
}

// what ONE block of the launch does besides its tile when the coefficients are derived in the kernel: mode 1 — saved
// statistics, the affine form for the backward's consumers, running statistics (one momentum update per group, in
// group order: the loop is this function's own because every group's saved state is written on the way, the step is
// bn_coeffs.h's)
template <int PRO>
__device__ inline void pro_block0(const FsConvArgs& p, int t, int nt) {
  if (!p.pro_stats) return;
  const int C = p.Cs;
  const int G = p.pro_group_imgs > 0 ? p.N / p.pro_group_imgs : 1;
  if constexpr (PRO == 1) {
    const bool track = p.pro_running_mean != nullptr;
    for (int c = t; c < C; c += nt) {
      float rm = track ? p.pro_running_mean[c] : 0.f, rv = track ? p.pro_running_var[c] : 0.f;
      for (int g = 0; g < G; ++g) {
        const BnCoeffs k = pro1_channel(p, g, c);
        if (p.pro_mean) { p.pro_mean[g * C + c] = k.mean; p.pro_invstd[g * C + c] = k.invstd; }
        if (p.pro_save_a) { p.pro_save_a[g * C + c] = k.scale; p.pro_save_b[g * C + c] = k.shift; }
        const double unb = bn_unbiased(k.var_b, p.pro_count);
        rm = bn_momentum(rm, k.mean, p.pro_momentum);
        rv = bn_momentum(rv, (float)unb, p.pro_momentum);
      }
      if (track) { p.pro_running_mean[c] = rm; p.pro_running_var[c] = rv; }
    }
    if (t == 0 && p.pro_nbt) *p.pro_nbt += G;
  }
}

// argument checks shared by the two kernels' entry points
inline bool pro_args_ok(const FsConvArgs& a) {
  // (retired slots of the round 3-4 backward prologue: header rule — they stay NULL whatever the mode)
  if (a.pro_c || a.pro_m || a.pro_src2 || a.pro_stats_local || a.pro_dgamma || a.pro_dbeta || a.pro_dst) return false;
  if (a.pro_mode == 0) return true;
  if (a.pro_mode != 1) return false;
  // (the coefficient table is dynamic LDS on top of 38-78 KB of static LDS: 2 floats per source channel; the widest 3x3
  // layer of the networks has 512 — wider layers are declined here, the callers' can_fold_* then never ask)
  if (a.Cs % 4 != 0 || a.Cs > 512) return false;
  if (a.pro_group_imgs < 0 || (a.pro_group_imgs > 0 && a.N % a.pro_group_imgs != 0)) return false;
  if (a.pro_stats) {
    if (!a.pro_gamma || !a.pro_beta || !(a.pro_count > 0.0)) return false;
    if ((a.pro_mean == nullptr) != (a.pro_invstd == nullptr) || (a.pro_save_a == nullptr) != (a.pro_save_b == nullptr)) return false;
    if ((a.pro_running_mean == nullptr) != (a.pro_running_var == nullptr)) return false;
  } else {
    if (!a.pro_a || !a.pro_b) return false;
  }
  return true;
}

}  // namespace
