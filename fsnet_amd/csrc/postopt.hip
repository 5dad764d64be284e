// Sparse-VO depth post-optimisation on the device (monodepth/networks/utils/postopt_utils.py:8-11, 94-226; the
// refinement stage of KittiEvaluationHook_postopt, base_evaluation_hooks.py:69-127): per image, denorm -> Lab -> SLIC
// over (Lab, x, y, depth) -> VO point selection -> per-segment log-scale targets -> the smoothness-coupled K x K
// system -> exp(log depth + per-segment shift).
//
// One fixed launch sequence per batch (the image index is blockIdx.y), no host round trip, so the whole call can be
// captured into a hipGraph:
//   postopt_prepare        per pixel: denorm (f64), Lab (f64 -> fp32), |log d - log vo| and the VO validity bit
//   postopt_centres_init   per image: the K initial centres (grid_sample bilinear, zeros, align_corners); zeroes state
//   postopt_assign x iters per pixel: nearest centre (K centres in LDS) + fixed-point sums per centre; at its head each
//                          block forms the centres from the previous iteration's sums and stops the image on the
//                          device when the P-means did not move (the reference's early break)
//   postopt_vo_select      per image: the max_points smallest |log d - log vo| by a radix select over the bit patterns
//   postopt_segment_stats  per pixel: fixed-point per-segment sums of log d and of (log vo - log d) over the VO mask
//   postopt_solve          per image, one workgroup: W, right-hand side, Jacobi-preconditioned CG in fp64
//   postopt_apply          per pixel: exp(log d + shift of its segment), compacted labels
//
// Determinism: every per-centre / per-segment sum is an exact integer sum (64-bit fixed point: Lab and log values at
// 2^-24, depth at 2^-20, pixel coordinates as integers), so the order of the atomics does not matter; the CG dot products
// are reduced in a fixed tree.  The output is bit-identical from run to run and independent of the batching.
#include "common.h"
#include "fsnet_hip_internal.h"

namespace {

constexpr int KMAX = 1024;           // segment slots (one solve thread per slot)
constexpr int PIX = 4;               // pixels per thread in the assign / stats kernels
constexpr int SUMW = 8;              // int64 words per centre sum: n, L, a, b, x, y, z, (pad)
constexpr int STW = 4;               // int64 words per segment stat: n, sum lp, n masked, sum (lv - lp) masked
constexpr double FIX24 = 16777216.0;            // 2^24
constexpr double FIX20 = 1048576.0;             // 2^20
constexpr float LOG80F = 4.382026634673881f;    // np.log(80) compared in fp32
constexpr float LOG3F = 1.0986122886681098f;    // np.log(3)

struct Ctx {
  const float* image; const float* depth; const float* vo; const float* ctab;
  float* out; int32_t* labels; int32_t* nseg;
  float4* lab4;            // [B][N] (L, a, b, depth)
  unsigned* dv;            // [B][N] bits of |lp - lv|, bit 31 = VO valid
  int32_t* raw;            // [B][N] centre index
  long long* sums;         // [3][B][K][SUMW]
  float4* cen;             // [2][B][K][2] (L, a, b, z), (x, y, -, -)
  long long* stats;        // [B][K][STW]
  float* shift;            // [B][K]
  int32_t* compact;        // [B][K]
  float* wmat;             // [B][K][K]
  int32_t* state;          // [B][8]: stop, last iteration, T bits, tie cut, n valid, n segments
  double mean[3], std[3];
  float lw, dw, iw;
  double l0, l1, l2;
  int B, H, W, K, max_points;
  long long N;
};

__device__ __forceinline__ long long fix(float v, double s) { return (long long)__double2ll_rn((double)v * s); }
__device__ __forceinline__ float unfix(long long v, double s) { return (float)((double)v / s); }

__device__ __forceinline__ unsigned vo_bits(float d, float v) {
  const float lp = logf(d), lv = logf(v);
  const unsigned valid = (lv < LOG80F && lv > LOG3F) ? 0x80000000u : 0u;
  return (__float_as_uint(fabsf(lp - lv)) & 0x7fffffffu) | valid;
}

// the centre a sum row stands for: sum / (count + 1e-4) in fp32 (postopt_utils.py:137-140)
__device__ __forceinline__ void centre_of(const long long* s, float4& a, float4& q) {
  const float div = (float)s[0] + 1e-4f;
  a = make_float4(unfix(s[1], FIX24) / div, unfix(s[2], FIX24) / div, unfix(s[3], FIX24) / div,
                  unfix(s[6], FIX20) / div);
  q = make_float4((float)s[4] / div, (float)s[5] / div, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void postopt_prepare(Ctx c) {
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= c.N) return;
  const long long o = (long long)b * c.N + p;
  const float* im = c.image + (long long)b * 3 * c.N + p;
  double lin[3];
  for (int ch = 0; ch < 3; ++ch) {
    // np.clip((img * std + mean) * 255, 0, 255) in float64, then the truncating uint8 cast
    double v = ((double)im[ch * c.N] * c.std[ch] + c.mean[ch]) * 255.0;
    v = fmin(fmax(v, 0.0), 255.0);
    const double t = (double)(unsigned)v / 255.0;
    lin[ch] = t > 0.04045 ? pow((t + 0.055) / 1.055, 2.4) : t / 12.92;
  }
  const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169},
                          {0.019334, 0.119193, 0.950227}};
  const double white[3] = {0.95047, 1.0, 1.08883};
  double f[3];
  for (int i = 0; i < 3; ++i) {
    const double t = (lin[0] * M[i][0] + lin[1] * M[i][1] + lin[2] * M[i][2]) / white[i];
    f[i] = t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
  }
  const float d = c.depth[o];
  c.lab4[o] = make_float4((float)(116.0 * f[1] - 16.0), (float)(500.0 * (f[0] - f[1])), (float)(200.0 * (f[1] - f[2])),
                          d);
  c.dv[o] = vo_bits(d, c.vo[o]);
}

// grid_sample(bilinear, zeros, align_corners=True) of one channel at (ix, iy), weights formed like torch's CPU kernel
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float wx, float wy) {
  const float e = 1.f - wx, s = 1.f - wy;
  return v00 * (s * e) + v01 * (s * wx) + v10 * (wy * e) + v11 * (wy * wx);
}

__global__ __launch_bounds__(256) void postopt_centres_init(Ctx c) {
  const int b = blockIdx.y, K = c.K, H = c.H, W = c.W;
  const float4* lab = c.lab4 + (long long)b * c.N;
  for (int k = threadIdx.x; k < K; k += 256) {
    // component 0 of the table (the h-range) is grid_sample's x, the width axis (postopt_utils.py:108-117)
    const float ix = (c.ctab[2 * k] + 1.f) * ((float)(W - 1) / 2.f);
    const float iy = (c.ctab[2 * k + 1] + 1.f) * ((float)(H - 1) / 2.f);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float wx = ix - fx0, wy = iy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    float v[4][7];   // corners nw, ne, sw, se x (L, a, b, z, x, y)
    for (int q = 0; q < 4; ++q) {
      const int xx = x0 + (q & 1), yy = y0 + (q >> 1);
      const bool in = xx >= 0 && xx < W && yy >= 0 && yy < H;
      const float4 l = in ? lab[(long long)yy * W + xx] : make_float4(0.f, 0.f, 0.f, 0.f);
      v[q][0] = l.x; v[q][1] = l.y; v[q][2] = l.z; v[q][3] = l.w;
      v[q][4] = in ? (float)xx : 0.f; v[q][5] = in ? (float)yy : 0.f;
    }
    float r[6];
    for (int j = 0; j < 6; ++j) r[j] = bilerp(v[0][j], v[1][j], v[2][j], v[3][j], wx, wy);
    float4* cc = c.cen + ((long long)b * K + k) * 2;
    cc[0] = make_float4(r[0], r[1], r[2], r[3]);
    cc[1] = make_float4(r[4], r[5], 0.f, 0.f);
  }
  long long* s0 = c.sums + (long long)b * K * SUMW;
  for (int i = threadIdx.x; i < K * SUMW; i += 256) s0[i] = 0;
  long long* st = c.stats + (long long)b * K * STW;
  for (int i = threadIdx.x; i < K * STW; i += 256) st[i] = 0;
  if (threadIdx.x < 8) c.state[b * 8 + threadIdx.x] = 0;
}

// one SLIC iteration (postopt_utils.py:119-142).  Dynamic LDS: K x 2 float4 centres + K x 7 int64 sums.
__global__ __launch_bounds__(256) void postopt_assign(Ctx c, int it) {
  extern __shared__ float4 smem[];
  const int b = blockIdx.y, K = c.K, W = c.W;
  int32_t* st = c.state + b * 8;
  if (st[0]) return;                                   // the image stopped in an earlier iteration
  float4* cA = smem;
  float4* cB = smem + K;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + 2 * K);
  const long long slot = (long long)c.B * K * SUMW;
  if (it > 0) {
    const long long* prev = c.sums + ((it + 2) % 3) * slot + (long long)b * K * SUMW;
    const float4* old = c.cen + ((long long)((it - 1) & 1) * c.B * K + (long long)b * K) * 2;
    int moved = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
      float4 a, q;
      centre_of(prev + (long long)k * SUMW, a, q);
      const float4 oa = old[2 * k], oq = old[2 * k + 1];
      moved |= (a.w != oa.w) | (q.x != oq.x) | (q.y != oq.y);
      cA[k] = a; cB[k] = q;
    }
    if (!__syncthreads_or(moved)) {                    // new P-means == current ones: the reference breaks here
      if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = 1;
      return;
    }
    if (blockIdx.x == 0) {
      float4* cur = c.cen + ((long long)(it & 1) * c.B * K + (long long)b * K) * 2;
      for (int k = threadIdx.x; k < K; k += 256) { cur[2 * k] = cA[k]; cur[2 * k + 1] = cB[k]; }
    }
  } else {
    const float4* cur = c.cen + (long long)b * K * 2;
    for (int k = threadIdx.x; k < K; k += 256) { cA[k] = cur[2 * k]; cB[k] = cur[2 * k + 1]; }
  }
  if (blockIdx.x == 0) {
    long long* nxt = c.sums + ((it + 1) % 3) * slot + (long long)b * K * SUMW;
    for (int i = threadIdx.x; i < K * SUMW; i += 256) nxt[i] = 0;
    if (threadIdx.x == 0) st[1] = it;
  }
  for (int i = threadIdx.x; i < K * 7; i += 256) acc[i] = 0ull;
  __syncthreads();

  const long long p0 = (long long)blockIdx.x * (256 * PIX) + threadIdx.x;
  float L[PIX], A[PIX], Bb[PIX], Z[PIX], X[PIX], Y[PIX], best[PIX];
  int bi[PIX];
  for (int j = 0; j < PIX; ++j) {
    const long long p = p0 + j * 256;
    const bool in = p < c.N;
    const float4 l = in ? c.lab4[(long long)b * c.N + p] : make_float4(0.f, 0.f, 0.f, 0.f);
    L[j] = l.x; A[j] = l.y; Bb[j] = l.z; Z[j] = l.w;
    const int y = in ? (int)(p / W) : 0;
    Y[j] = (float)y; X[j] = in ? (float)(int)(p - (long long)y * W) : 0.f;
    best[j] = INFINITY; bi[j] = 0;
  }
  const float lw = c.lw, dw = c.dw, iw = c.iw;
  for (int k = 0; k < K; ++k) {
    const float4 a = cA[k], q = cB[k];
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const float dl = L[j] - a.x, da = A[j] - a.y, db = Bb[j] - a.z;
      const float rgb = sqrtf(dl * dl + da * da + db * db);
      const float dz = fabsf(Z[j] - a.w);
      const float dx = X[j] - q.x, dy = Y[j] - q.y;
      const float img = sqrtf(dx * dx + dy * dy);
      const float t = rgb * lw + dz * dw + img * iw;
      if (t < best[j]) { best[j] = t; bi[j] = k; }        // first index on ties (torch.min)
    }
  }
  for (int j = 0; j < PIX; ++j) {
    const long long p = p0 + j * 256;
    if (p >= c.N) continue;
    c.raw[(long long)b * c.N + p] = bi[j];
    unsigned long long* s = acc + bi[j] * 7;
    atomicAdd(s + 0, 1ull);
    atomicAdd(s + 1, (unsigned long long)fix(L[j], FIX24));
    atomicAdd(s + 2, (unsigned long long)fix(A[j], FIX24));
    atomicAdd(s + 3, (unsigned long long)fix(Bb[j], FIX24));
    atomicAdd(s + 4, (unsigned long long)(long long)X[j]);
    atomicAdd(s + 5, (unsigned long long)(long long)Y[j]);
    atomicAdd(s + 6, (unsigned long long)fix(Z[j], FIX20));
  }
  __syncthreads();
  unsigned long long* dst =
      reinterpret_cast<unsigned long long*>(c.sums + (it % 3) * slot + (long long)b * K * SUMW);
  for (int k = threadIdx.x; k < K; k += 256) {
    if (acc[k * 7] == 0ull) continue;
    for (int w = 0; w < 7; ++w) atomicAdd(dst + (long long)k * SUMW + w, acc[k * 7 + w]);
  }
}

// block-wide exclusive prefix of a 0/1 flag (blockDim.x == 1024); returns the block total
__device__ int block_scan(int flag, int& excl, int* wsum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wsum[wv] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
  for (int q = 0; q < 16; ++q) { before += q < wv ? wsum[q] : 0; total += wsum[q]; }
  excl = before + in_wave;
  return total;
}

// the max_points smallest |lp - lv| (postopt_utils.py:156-168): k-th smallest by a radix select over the bit patterns
// (4 passes of 8-bit digits, like radix_select in eval.hip), ties at the threshold taken lowest pixel index first
__global__ __launch_bounds__(1024) void postopt_vo_select(Ctx c) {
  __shared__ unsigned hist[256];
  __shared__ int s_valid, wsum[16];
  __shared__ unsigned s_prefix, s_eq;
  __shared__ long long s_k;
  __shared__ int s_cut, s_run;
  const int b = blockIdx.y;
  const unsigned* dv = c.dv + (long long)b * c.N;
  int32_t* st = c.state + b * 8;
  for (int i = threadIdx.x; i < 256; i += 1024) hist[i] = 0;
  if (threadIdx.x == 0) s_valid = 0;
  __syncthreads();
  int nv = 0;
  for (long long i = threadIdx.x; i < c.N; i += 1024) {
    const unsigned u = dv[i];
    nv += (int)(u >> 31);
    atomicAdd(&hist[(u >> 24) & 127u], 1u);
  }
  atomicAdd(&s_valid, nv);
  __syncthreads();
  const int nvalid = s_valid;
  if (nvalid < c.max_points) {                         // the mask is the validity alone
    if (threadIdx.x == 0) { st[2] = (int32_t)0xffffffffu; st[3] = 0x7fffffff; st[4] = nvalid; }
    return;
  }
  unsigned prefix = 0, mask = 0;
  long long k = c.max_points - 1;
  unsigned eq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (shift < 24) {
      for (int i = threadIdx.x; i < 256; i += 1024) hist[i] = 0;
      __syncthreads();
      for (long long i = threadIdx.x; i < c.N; i += 1024) {
        const unsigned u = dv[i] & 0x7fffffffu;
        if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      long long kk = k; unsigned d = 0;
      for (; d < 256; ++d) { if (kk < (long long)hist[d]) break; kk -= hist[d]; }
      s_prefix = prefix | (d << shift); s_k = kk; s_eq = hist[d];
    }
    __syncthreads();
    prefix = s_prefix; k = s_k; eq = s_eq; mask |= 255u << shift;
    __syncthreads();
  }
  // the k+1 first (by pixel index) of the `eq` pixels equal to the threshold are in the top k
  const long long take = k + 1;
  int cut = 0x7fffffff;
  if (take < (long long)eq) {
    if (threadIdx.x == 0) { s_run = 0; s_cut = 0x7fffffff; }
    __syncthreads();
    for (long long c0 = 0; c0 < c.N; c0 += 1024) {
      const long long p = c0 + threadIdx.x;
      const int flag = p < c.N && (dv[p] & 0x7fffffffu) == prefix;
      int excl;
      const int tot = block_scan(flag, excl, wsum);
      const int run = s_run;
      if (flag && run + excl + 1 == take) s_cut = (int)p;
      __syncthreads();
      if (threadIdx.x == 0) s_run = run + tot;
      __syncthreads();
      if (s_run >= take) break;
    }
    cut = s_cut;
  }
  if (threadIdx.x == 0) { st[2] = (int32_t)prefix; st[3] = cut; st[4] = nvalid; }
}

__device__ __forceinline__ bool vo_selected(unsigned u, long long p, unsigned T, int cut) {
  const unsigned a = u & 0x7fffffffu;
  return (u >> 31) && (a < T || (a == T && p <= (long long)cut));
}

// per-segment sums for the targets (postopt_utils.py:197-207).  Dynamic LDS: K x 4 int64.
__global__ __launch_bounds__(256) void postopt_segment_stats(Ctx c) {
  extern __shared__ float4 smem[];
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  const int b = blockIdx.y, K = c.K;
  const int32_t* st = c.state + b * 8;
  const unsigned T = (unsigned)st[2];
  const int cut = st[3];
  for (int i = threadIdx.x; i < K * STW; i += 256) acc[i] = 0ull;
  __syncthreads();
  const long long p0 = (long long)blockIdx.x * (256 * PIX) + threadIdx.x;
  for (int j = 0; j < PIX; ++j) {
    const long long p = p0 + j * 256;
    if (p >= c.N) continue;
    const long long o = (long long)b * c.N + p;
    const float lp = logf(c.depth[o]);
    unsigned long long* s = acc + c.raw[o] * STW;
    atomicAdd(s + 0, 1ull);
    atomicAdd(s + 1, (unsigned long long)fix(lp, FIX24));
    if (vo_selected(c.dv[o], p, T, cut)) {
      const float lv = logf(c.vo[o]);
      atomicAdd(s + 2, 1ull);
      atomicAdd(s + 3, (unsigned long long)fix(lv - lp, FIX24));
    }
  }
  __syncthreads();
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(c.stats + (long long)b * K * STW);
  for (int k = threadIdx.x; k < K; k += 256) {
    if (acc[k * STW] == 0ull) continue;
    for (int w = 0; w < STW; ++w) atomicAdd(dst + (long long)k * STW + w, acc[k * STW + w]);
  }
}

// fixed-order block sum of two doubles (blockDim.x == 1024); every thread gets the totals
__device__ __forceinline__ double2 block_sum2(double a, double b, double* sh) {
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh[16 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  double ta = 0.0, tb = 0.0;
  for (int q = 0; q < 16; ++q) { ta += sh[q]; tb += sh[16 + q]; }
  return make_double2(ta, tb);
}

// the K x K system (postopt_utils.py:208-219), one workgroup per image, thread i = segment slot i.
// A = diag(l0 s + l1 m + l2) - l0 W over the non-empty slots (W_ii = 1 included in s); an empty slot is an identity
// row with a zero right-hand side and no coupling.  Jacobi-preconditioned CG in fp64 to a relative residual of 1e-10.
__global__ __launch_bounds__(1024) void postopt_solve(Ctx c) {
  __shared__ float s_cx[KMAX], s_cy[KMAX], s_base[KMAX];
  __shared__ double s_p[KMAX];
  __shared__ double sh[32];
  __shared__ int wsum[16];
  const int b = blockIdx.y, K = c.K, i = threadIdx.x;
  int32_t* st = c.state + b * 8;
  const long long* sl = c.sums + (st[1] % 3) * ((long long)c.B * K * SUMW) + (long long)b * K * SUMW;
  const long long* ss = c.stats + (long long)b * K * STW;
  bool ne = false;
  float base = 0.f, target = 1.f, m = 0.f;
  if (i < K) {
    const long long* s = sl + (long long)i * SUMW;
    ne = s[0] > 0;
    float4 a, q;
    centre_of(s, a, q);
    s_cx[i] = q.x; s_cy[i] = q.y;
    if (ne) {
      const long long* t = ss + (long long)i * STW;
      base = unfix(t[1], FIX24) / (float)t[0];
      if (t[2] > 0) { m = 1.f; target = unfix(t[3], FIX24) / (float)t[2] + base; }
    }
  }
  if (i < K) s_base[i] = base;
  int rank;
  const int nseg = block_scan(ne ? 1 : 0, rank, wsum);
  if (i < K) c.compact[(long long)b * K + i] = ne ? rank : -1;
  if (i == 0) st[5] = nseg;
  __syncthreads();
  const double l0 = c.l0, l1 = c.l1, l2 = c.l2;
  const bool coupled = l0 != 0.0;
  float* Wm = c.wmat + (long long)b * K * K;
  double s = 0.0, cpl = 0.0;
  if (coupled && i < K) {
    // w_ij = exp(-|c_i - c_j| / 20) in fp32 like the reference; column i of the symmetric W is row i
    for (int j = 0; j < K; ++j) {
      float w = 0.f;
      if (ne && sl[(long long)j * SUMW] > 0) {
        const float dx = s_cx[j] - s_cx[i], dy = s_cy[j] - s_cy[i];
        w = expf(-sqrtf(dx * dx + dy * dy) / 20.f);
        s += (double)w;
        cpl += ((double)base - (double)s_base[j]) * (double)w;
      }
      Wm[(long long)j * K + i] = w;
    }
  }
  __syncthreads();     // W complete (the block's own global writes are visible to it after the barrier)
  const double dd = ne ? l0 * s + l1 * (double)m + l2 : 1.0;     // diag(l0 s + l1 m + l2)
  const double diag = ne ? dd - l0 : 1.0;                         // ... - l0 W_ii
  const double rhs = ne ? l2 * (double)base + l1 * (double)m * (double)target + l0 * cpl : 0.0;
  double x = 0.0, r = i < K ? rhs : 0.0;
  double z = r / diag, p = z;
  double2 t = block_sum2(r * z, r * r, sh);
  double rz = t.x;
  const double bnorm = sqrt(t.y);
  const int maxit = 2 * K + 64;
  for (int itc = 0; itc < maxit && bnorm > 0.0; ++itc) {
    s_p[i] = p;
    __syncthreads();
    double q = 0.0;
    if (i < K) {
      double wp = 0.0;
      if (coupled && ne)
        for (int j = 0; j < K; ++j) wp += (double)Wm[(long long)j * K + i] * s_p[j];
      q = ne ? dd * p - l0 * wp : p;
    }
    const double pq = block_sum2(p * q, 0.0, sh).x;
    const double alpha = rz / pq;
    x += alpha * p;
    r -= alpha * q;
    z = r / diag;
    t = block_sum2(r * z, r * r, sh);
    if (sqrt(t.y) <= 1e-10 * bnorm) break;
    const double beta = t.x / rz;
    rz = t.x;
    p = z + beta * p;
  }
  if (i < K) c.shift[(long long)b * K + i] = ne ? (float)x - base : 0.f;
}

// out = exp(log d + x_label - base_label) (postopt_utils.py:220-223)
__global__ __launch_bounds__(256) void postopt_apply(Ctx c) {
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c.nseg && p == 0) c.nseg[b] = c.state[b * 8 + 5];
  if (p >= c.N) return;
  const long long o = (long long)b * c.N + p;
  const int k = c.raw[o];
  c.out[o] = expf(logf(c.depth[o]) + c.shift[(long long)b * c.K + k]);
  if (c.labels) c.labels[o] = c.compact[(long long)b * c.K + k];
}

inline long long align256(long long v) { return (v + 255) / 256 * 256; }

struct Layout {
  long long lab4, dv, raw, sums, cen, stats, shift, compact, wmat, state, total;
};

inline Layout layout(int B, long long N, int K) {
  Layout l;
  long long o = 0;
  l.lab4 = o;    o += align256((long long)B * N * 16);
  l.dv = o;      o += align256((long long)B * N * 4);
  l.raw = o;     o += align256((long long)B * N * 4);
  l.sums = o;    o += align256(3LL * B * K * SUMW * 8);
  l.cen = o;     o += align256(2LL * B * K * 32);
  l.stats = o;   o += align256((long long)B * K * STW * 8);
  l.shift = o;   o += align256((long long)B * K * 4);
  l.compact = o; o += align256((long long)B * K * 4);
  l.wmat = o;    o += align256((long long)B * K * K * 4);
  l.state = o;   o += align256((long long)B * 8 * 4);
  l.total = o;
  return l;
}

inline bool shape_ok(int B, int H, int W, int K) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31) && K >= 1 && K <= KMAX;
}

}  // namespace

extern "C" int64_t fs_postopt_workspace_bytes(int B, int H, int W, int K) {
  if (!shape_ok(B, H, W, K)) return -1;
  return layout(B, (long long)H * W, K).total;
}

extern "C" int fs_postopt(const FsPostOptArgs* a, void* stream) {
  if (!a || !a->image || !a->depth || !a->vo || !a->centres || !a->out || !a->workspace) return FS_EINVAL;
  if (!shape_ok(a->B, a->H, a->W, a->K) || a->iter_num < 1 || a->max_points < 1) return FS_EINVAL;
  if (!(a->lambda2 > 0.0) || !(a->lambda0 >= 0.0) || !(a->lambda1 >= 0.0)) return FS_EINVAL;
  const long long N = (long long)a->H * a->W;
  const Layout l = layout(a->B, N, a->K);
  if (a->workspace_bytes < l.total) return FS_EINVAL;
  char* ws = static_cast<char*>(a->workspace);
  Ctx c;
  c.image = a->image; c.depth = a->depth; c.vo = a->vo; c.ctab = a->centres;
  c.out = a->out; c.labels = a->labels; c.nseg = a->nseg;
  c.lab4 = reinterpret_cast<float4*>(ws + l.lab4);
  c.dv = reinterpret_cast<unsigned*>(ws + l.dv);
  c.raw = reinterpret_cast<int32_t*>(ws + l.raw);
  c.sums = reinterpret_cast<long long*>(ws + l.sums);
  c.cen = reinterpret_cast<float4*>(ws + l.cen);
  c.stats = reinterpret_cast<long long*>(ws + l.stats);
  c.shift = reinterpret_cast<float*>(ws + l.shift);
  c.compact = reinterpret_cast<int32_t*>(ws + l.compact);
  c.wmat = reinterpret_cast<float*>(ws + l.wmat);
  c.state = reinterpret_cast<int32_t*>(ws + l.state);
  for (int ch = 0; ch < 3; ++ch) { c.mean[ch] = a->rgb_mean[ch]; c.std[ch] = a->rgb_std[ch]; }
  c.lw = a->lab_dist_weight; c.dw = a->depth_dist_weight; c.iw = a->image_dist_weight;
  c.l0 = a->lambda0; c.l1 = a->lambda1; c.l2 = a->lambda2;
  c.B = a->B; c.H = a->H; c.W = a->W; c.K = a->K; c.max_points = a->max_points;
  c.N = N;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned pix_blocks = (unsigned)((N + 255) / 256);
  const unsigned tile_blocks = (unsigned)((N + 256 * PIX - 1) / (256 * PIX));
  const size_t lds_assign = (size_t)a->K * (2 * 16 + 7 * 8);
  const size_t lds_stats = (size_t)a->K * STW * 8;
  static bool lds_raised = false;                     // assign at K > 682 needs more than the default 64 KiB
  if (!lds_raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(postopt_assign), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((size_t)KMAX * (2 * 16 + 7 * 8))) != hipSuccess)
      return FS_ELAUNCH;
    lds_raised = true;
  }
  hipLaunchKernelGGL(postopt_prepare, dim3(pix_blocks, a->B), dim3(256), 0, st, c);
  hipLaunchKernelGGL(postopt_centres_init, dim3(1, a->B), dim3(256), 0, st, c);
  for (int it = 0; it < a->iter_num; ++it)
    hipLaunchKernelGGL(postopt_assign, dim3(tile_blocks, a->B), dim3(256), lds_assign, st, c, it);
  hipLaunchKernelGGL(postopt_vo_select, dim3(1, a->B), dim3(1024), 0, st, c);
  hipLaunchKernelGGL(postopt_segment_stats, dim3(tile_blocks, a->B), dim3(256), lds_stats, st, c);
  hipLaunchKernelGGL(postopt_solve, dim3(1, a->B), dim3(1024), 0, st, c);
  hipLaunchKernelGGL(postopt_apply, dim3(pix_blocks, a->B), dim3(256), 0, st, c);
  return fs_launch_status();
}
