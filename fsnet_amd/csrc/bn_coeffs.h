// The statistics arithmetic of train-mode BatchNorm, stated once: f64 slot sums -> moments -> per-channel coefficients,
// and the running-statistics momentum update.  Every kernel that derives coefficients itself goes through these
// (bn.hip: bn_finalize / bn_apply / bn_apply_pool and the backward preamble; conv_pro.h: the operand prologue of the
// 3x3 convolutions), which is what keeps their results bit-identical (tests/test_bn_fold_gpu.py,
// test_conv_fold_gpu.py, test_ops_gpu.py::test_stem_batchnorm_relu_maxpool_in_one_pass compare them with torch.equal).
#pragma once
#include "common.h"
#include "fsnet_hip_internal.h"

namespace {

// one statistics group's slot sums [FS_STAT_SLOTS][2][C] -> the two totals of channel c
__device__ inline void bn_sum_slots(const double* st, int C, int c, double& s1, double& s2) {
  s1 = 0.0; s2 = 0.0;
#pragma unroll
  for (int k = 0; k < FS_STAT_SLOTS; ++k) { s1 += st[(long)k * 2 * C + c]; s2 += st[(long)k * 2 * C + C + c]; }
}

// (sum x, sum x^2) over `count` elements -> mean and biased variance
__device__ inline void bn_moments(double s1, double s2, double count, double& m, double& v) {
  m = s1 / count; v = s2 / count - m * m;
}

struct BnCoeffs { float mean, var_b, invstd, scale, shift; };      // y = scale * x + shift

__device__ inline BnCoeffs bn_coeffs(double m, double v, float eps, float gamma, float beta) {
  if (v < 0) v = 0;
  BnCoeffs k;
  k.mean = (float)m;
  k.var_b = (float)v;
  k.invstd = (float)(1.0 / sqrt(v + (double)eps));
  k.scale = gamma * k.invstd;
  k.shift = beta - k.mean * k.scale;
  return k;
}

// train mode: st = the group's slot sums; eval mode (st == NULL): the running statistics
__device__ inline BnCoeffs bn_channel_coeffs(const double* st, const float* rmean, const float* rvar, int C, int c,
                                             double count, float eps, float gamma, float beta) {
  double m, v;
  if (st) {
    double s1, s2;
    bn_sum_slots(st, C, c, s1, s2);
    bn_moments(s1, s2, count, m, v);
  }
  else { m = rmean[c]; v = rvar[c]; }
  return bn_coeffs(m, v, eps, gamma, beta);
}

// one invocation of the module updates both running statistics with bn_momentum, the variance with its unbiased form.
// (Two value-returning pieces and not one step with reference results: that form compiled to different code in the
// 3x3 convolution kernels, whose assembly the factoring must leave as it was.)
__device__ inline double bn_unbiased(float var_b, double count) {
  return count > 1.0 ? (double)var_b * count / (count - 1.0) : (double)var_b;
}
__device__ inline float bn_momentum(float running, float batch, float momentum) {
  return (1.f - momentum) * running + momentum * batch;
}

// one momentum step per statistics group, in group order (= the order the reference calls the module in).  stats: the
// slot sums of all G groups; k0: group 0's coefficients, which every caller has at hand.  The caller decides which
// thread does this once per channel, and adds G to num_batches_tracked.
__device__ inline void bn_running_update(const BnCoeffs& k0, const double* stats, int G, int C, int c, double count,
                                         float eps, float momentum, float* running_mean, float* running_var) {
  float rm = running_mean[c], rv = running_var[c];
  for (int g = 0; g < G; ++g) {
    const BnCoeffs k = g == 0 ? k0 : bn_channel_coeffs(stats + g * ((long)FS_STAT_SLOTS * 2 * C), nullptr, nullptr, C, c,
                                                        count, eps, 1.f, 0.f);
    const double unb = bn_unbiased(k.var_b, count);
    rm = bn_momentum(rm, k.mean, momentum);
    rv = bn_momentum(rv, (float)unb, momentum);
  }
  running_mean[c] = rm; running_var[c] = rv;
}

}  // namespace
