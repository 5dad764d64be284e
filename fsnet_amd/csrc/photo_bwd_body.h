// Body of the fused photometric backward, shared by photo_fused.hip (two source frames, pinhole and fisheye) and
// photo_multi.hip / photo_mei_multi.hip (one to four source frames, pinhole / fisheye): the kernels differ in how a
// wave finds its source frame and in the argument struct, which the policy `FR` answers — everything else is this one text.  Included after
// photo_common.h by files that allow fused multiply-adds (FS_PHOTO_CONTRACT_FAST).
#pragma once
#pragma clang fp contract(fast)

namespace {

// The three colour channels of one quantity as a packed pair + a scalar (backward kernel: a wave owns ONE frame there, the
// channels are what is independent): two instructions where three scalar ones stood, no register overhead.
struct C3 { f2 p; float s; };
__device__ __forceinline__ C3 c3(float a, float b, float c) { return C3{f2{a, b}, c}; }
__device__ __forceinline__ C3 c3(float a) { return C3{f2{a, a}, a}; }
__device__ __forceinline__ C3 operator+(C3 a, C3 b) { return C3{a.p + b.p, a.s + b.s}; }
__device__ __forceinline__ C3 operator-(C3 a, C3 b) { return C3{a.p - b.p, a.s - b.s}; }
__device__ __forceinline__ C3 operator*(C3 a, C3 b) { return C3{a.p * b.p, a.s * b.s}; }
__device__ __forceinline__ C3 operator+(C3 a, float b) { return C3{a.p + b, a.s + b}; }
__device__ __forceinline__ C3 operator-(C3 a, float b) { return C3{a.p - b, a.s - b}; }
__device__ __forceinline__ C3 operator*(C3 a, float b) { return C3{a.p * b, a.s * b}; }
__device__ __forceinline__ C3 operator*(float b, C3 a) { return C3{a.p * b, a.s * b}; }
__device__ __forceinline__ C3 operator-(float b, C3 a) { return C3{b - a.p, b - a.s}; }
__device__ __forceinline__ C3 operator-(C3 a) { return C3{-a.p, -a.s}; }
__device__ __forceinline__ C3 hsum3(C3 v) { return C3{f2{hsum3(v.p.x), hsum3(v.p.y)}, hsum3(v.s)}; }
__device__ __forceinline__ C3 rcp3(C3 v) {
  return C3{f2{__builtin_amdgcn_rcpf(v.p.x), __builtin_amdgcn_rcpf(v.p.y)}, __builtin_amdgcn_rcpf(v.s)};
}
__device__ __forceinline__ void put(C3& v, int c, float x) { if (c == 0) v.p.x = x; else if (c == 1) v.p.y = x; else v.s = x; }
__device__ __forceinline__ float get(const C3& v, int c) { return c == 0 ? v.p.x : (c == 1 ? v.p.y : v.s); }
__device__ __forceinline__ float dot3(C3 a, C3 b) { const f2 q = a.p * b.p; return (q.x + q.y) + a.s * b.s; }

// two horizontally adjacent texels in ONE 8-byte load at 4-byte alignment (global memory runs in unaligned access
// mode on gfx9): the gather is bound by the number of vector-memory instructions, not by their bytes
struct __attribute__((packed, aligned(4))) F2u { float a, b; };
__device__ __forceinline__ F2u ldg2(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const F2u*>(reinterpret_cast<const char*>(base) + byte_off);
}

constexpr int BW = 60;     // output columns per wave (lanes 2..61)
constexpr int BRH = 32;    // output rows per wave
constexpr int LDS_C = 40;  // low-res accumulation tile of a wave (scales >= 1): columns / rows
constexpr int LDS_R = 24;

struct BRow {
  C3 t, tt, x, xx, xt;                      // horizontal 3-tap sums (per colour channel)
  C3 rt, rx;                                // raw values
  C3 Jx, Jy;                                // d pred_c / d (ix, iy) with the border-clamp multipliers applied
  float X, Y, Z, D;                         // transformed point (pinhole: Z + eps) and the upsampled depth
  float pm;                                 // patched_mask at the pixel (0 for virtual positions)
  int sel;                                  // selection byte at the pixel (-1 for virtual positions)
};
struct CRow { C3 a, b, c; };                // horizontally box-summed coefficients of one centre row

// FR: the frame-count policy (photo_common.h)
template <bool FISH, class FR, class Args>
__device__ __forceinline__ void photo_bwd_body(const Args& p, int SX, int SY, int nwaves,
                                               float (*s_dd)[LDS_R * LDS_C]) {
  const int nblk = gridDim.x;
  const int lb = ((int)blockIdx.x & 7) * (nblk >> 3) + ((int)blockIdx.x >> 3);
  const int wid = (int)threadIdx.x >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(lb * 4 + wid);
  if (wv >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const int sx = wv % SX;
  int rest = wv / SX;
  const int nf = FR::count(p);
  int f;
  FR::split(rest, nf, f);
  const int s = rest % p.S; rest /= p.S;
  const int sy = rest % SY;
  const int b = rest / SY;
  const int H = p.H, W = p.W;
  const unsigned HW = (unsigned)(H * W);
  const int h = p.dh[s], w = p.dw[s];
  const float* ge = p.geo + (long)b * FR::geo_stride(nf);
  const float* timg = p.img0 + (long)b * 3 * HW;
  const float* src = p.img_src[f] + (long)b * 3 * HW;
  const float* dmap = p.depth[s] + (long)b * h * w;
  const uint8_t* selb = p.sel + ((long)s * p.B + b) * HW;
  float* ddout = p.d_depth[s] + (long)b * h * w;
  float* lds = s_dd[wid];
  const int x0s = sx * BW, ys = sy * BRH;
  const int x = x0s - 2 + lane;
  const int xr = min(max(refl(x, W), 0), W - 1);
  const bool x_real = x >= 0 && x < W;
  const bool last_x = x0s + BW >= W, last_y = ys + BRH >= H;
  const bool col_own = (lane >= 2 && lane < 2 + BW && x < W) || (x == -1) || (x == W && last_x);   // x == -1 only when sx == 0
  const int q_lo = ys == 0 ? -1 : ys, q_hi = last_y ? H : ys + BRH - 1;
  const float k9 = 1.f / 9.f, k81 = 1.f / 81.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const float iwm1 = 1.f / wm1, ihm1 = 1.f / hm1;
  double msum = 0.0;
  for (int k = 0; k < p.B; ++k) msum += p.mask_sum[k];
  const float gscale = (float)((p.gout ? *p.gout : 1.0) / ((double)p.S * (msum + 1e-6)));
  const float wss = gscale * (0.85f / 3.f), wl1 = gscale * (0.15f / 3.f);

  // depth upsample invariants (see the forward kernel)
  const float sh = (H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
  const float sw = (W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
  const float fxu = sw * (float)xr;
  const int dx0 = w > 1 ? min((int)fxu, w - 2) : 0;
  const float dlx = w > 1 ? fxu - (float)dx0 : 0.f;
  const bool unit_scale = (h == H && w == W);
  const int lx_min = __builtin_amdgcn_readlane(dx0, 2);                       // lane 2 holds the strip's first column
  const int ly_min = (int)(sh * (float)min(max(ys - 1, 0), H - 1));
  if (!unit_scale) {
    for (int i = lane; i < LDS_R * LDS_C; i += 64) lds[i] = 0.f;
  }
  const float pxf = (float)xr;
  float ra[3] = {0.f, 0.f, 0.f}, Pm[12];
  if (!FISH) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ra[i] = ge[3 * i] * pxf;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) Pm[k] = ge[18 + f * 12 + k];
  const float* mei = nullptr;
  if constexpr (FISH) mei = p.mei + (long)b * 8;
  float dPacc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) dPacc[k] = 0.f;

  auto ray_of = [&](int yr, float (&r)[3]) {
    if constexpr (FISH) {
      const float* lut = p.lut_ptrs[b];
      const unsigned o = (unsigned)(yr * W + xr) * 4u;
      r[0] = ldg(lut, o); r[1] = ldg(lut + HW, o); r[2] = ldg(lut + 2 * HW, o);
    } else {
      const float pyf = (float)yr;
#pragma unroll
      for (int i = 0; i < 3; ++i) r[i] = (ra[i] + ge[3 * i + 1] * pyf) + ge[3 * i + 2];
    }
  };

  auto step = [&](BRow& r2, const BRow& r1, BRow& r0, CRow& c2, const CRow& c1, CRow& c0, const int it) {
    // ------------------------------------------------------------------ stage A: row y
    const int y = ys - 2 + it;
    const int yr = min(max(refl(y, H), 0), H - 1);
    const bool y_real = y >= 0 && y < H;
    const unsigned ob = (unsigned)(yr * W + xr) * 4u;
    r0.rt = c3(ldg(timg, ob), ldg(timg + HW, ob), ldg(timg + 2 * HW, ob));
    r0.sel = (x_real && y_real) ? (int)selb[(unsigned)(yr * W + xr)] : -1;
    r0.pm = (x_real && y_real) ? (p.patched_mask ? (float)p.patched_mask[(long)b * HW + (unsigned)(yr * W + xr)] : 1.f) : 0.f;
    if (p.motion_mask && x_real && y_real) r0.pm *= 1.f - p.motion_mask[(long)b * HW + (unsigned)(yr * W + xr)];
    {
      const float fyu = sh * (float)yr;
      const int dy0 = h > 1 ? min((int)fyu, h - 2) : 0;
      const float dly = h > 1 ? fyu - (float)dy0 : 0.f;
      // (a one-row map has dly = 0 and reads its row twice; a one-column map has dlx = 0: the same blend as the forward)
      const int dy1 = dy0 + (h > 1 ? 1 : 0);
      float d00, d01, d10, d11;
      if (w > 1) {
        const F2u a = ldg2(dmap, (unsigned)(dy0 * w + dx0) * 4u), c2_ = ldg2(dmap, (unsigned)(dy1 * w + dx0) * 4u);
        d00 = a.a; d01 = a.b; d10 = c2_.a; d11 = c2_.b;
      } else {
        d00 = d01 = ldg(dmap, (unsigned)(dy0 * w) * 4u); d10 = d11 = ldg(dmap, (unsigned)(dy1 * w) * 4u);
      }
      r0.D = (1.f - dly) * ((1.f - dlx) * d00 + dlx * d01) + dly * ((1.f - dlx) * d10 + dlx * d11);
    }
    float ray[3];
    ray_of(yr, ray);
    float ixu, iyu;
    {
      const float cx_ = r0.D * ray[0], cy_ = r0.D * ray[1], cz_ = r0.D * ray[2];
      r0.X = Pm[0] * cx_ + Pm[1] * cy_ + Pm[2] * cz_ + Pm[3];
      r0.Y = Pm[4] * cx_ + Pm[5] * cy_ + Pm[6] * cz_ + Pm[7];
      r0.Z = Pm[8] * cx_ + Pm[9] * cy_ + Pm[10] * cz_ + Pm[11];
      if (FISH) {
        float u, v;
        mei_cam2image(mei, r0.X, r0.Y, r0.Z, u, v);
        const float un = u / (float)max(W - 1, 1) * 2.f - 1.f, vn = v / (float)max(H - 1, 1) * 2.f - 1.f;
        ixu = (un + 1.f) * 0.5f * wm1; iyu = (vn + 1.f) * 0.5f * hm1;
      } else {
        r0.Z += 1e-7f;
        const float iz = __builtin_amdgcn_rcpf(r0.Z);
        const float u = r0.X * iz, v = r0.Y * iz;
        const float un = (u * iwm1 - 0.5f) * 2.f, vn = (v * ihm1 - 0.5f) * 2.f;
        ixu = (un + 1.f) * 0.5f * wm1; iyu = (vn + 1.f) * 0.5f * hm1;
      }
    }
    {
      // border clamp of grid_sample: the coordinate gradient is zero where the sample was clipped
      const float mx = (ixu > 0.f && ixu < wm1) ? 1.f : 0.f, my = (iyu > 0.f && iyu < hm1) ? 1.f : 0.f;
      const float ix = fminf(fmaxf(ixu, 0.f), wm1), iy = fminf(fmaxf(iyu, 0.f), hm1);
      const float fx0 = fminf(floorf(ix), wm1 - 1.f), fy0 = fminf(floorf(iy), hm1 - 1.f);
      const float wx = ix - fx0, wy = iy - fy0;
      const unsigned o0 = (unsigned)((int)fy0 * W + (int)fx0) * 4u, o1 = o0 + (unsigned)W * 4u;
      float rxv[3], jxv[3], jyv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const F2u a = ldg2(src + c * HW, o0), bb = ldg2(src + c * HW, o1);
        const float top = a.a + wx * (a.b - a.a), bot = bb.a + wx * (bb.b - bb.a);
        rxv[c] = top + wy * (bot - top);
        jxv[c] = mx * ((a.b - a.a) * (1.f - wy) + (bb.b - bb.a) * wy);
        jyv[c] = my * (bot - top);
      }
      r0.rx = c3(rxv[0], rxv[1], rxv[2]); r0.Jx = c3(jxv[0], jxv[1], jxv[2]); r0.Jy = c3(jyv[0], jyv[1], jyv[2]);
    }
    r0.t = hsum3(r0.rt);
    r0.tt = hsum3(r0.rt * r0.rt);
    r0.x = hsum3(r0.rx);
    r0.xx = hsum3(r0.rx * r0.rx);
    r0.xt = hsum3(r0.rx * r0.rt);
    // ------------------------------------------------------------------ stage B: window centre = row y - 1 (r1)
    {
      const float wgt = (it >= 2 && r1.sel == nf + f) ? r1.pm * wss : 0.f;
      const C3 sxs = (r2.x + r1.x) + r0.x, sys_ = (r2.t + r1.t) + r0.t;
      const C3 sxx = (r2.xx + r1.xx) + r0.xx, syy = (r2.tt + r1.tt) + r0.tt;
      const C3 sxy = (r2.xt + r1.xt) + r0.xt;
      const C3 mux = sxs * k9, muy = sys_ * k9;
      const C3 sgx = (9.f * sxx - sxs * sxs) * k81, sgy = (9.f * syy - sys_ * sys_) * k81,      // (as the forward)
               sgxy = (9.f * sxy - sxs * sys_) * k81;
      const C3 n1 = 2.f * mux * muy + C1, n2 = 2.f * sgxy + C2;
      const C3 d1 = mux * mux + muy * muy + C1, d2 = sgx + sgy + C2;
      const C3 n = n1 * n2, d = d1 * d2;
      const C3 id = rcp3(d);
      const C3 sv = (1.f - n * id) * 0.5f;
      // d n / d x(q) = a1 + a2 (t(q) - muy),  d d / d x(q) = b1 + b2 (x(q) - mux)   (each tap weight 1/9)
      const C3 a1 = 2.f * muy * n2 * k9, a2 = 2.f * n1 * k9;
      const C3 b1 = 2.f * mux * d2 * k9, b2 = 2.f * d1 * k9;
      const C3 hh = -0.5f * id * id;
      C3 A = hh * ((a1 - a2 * muy) * d - n * (b1 - b2 * mux));
      C3 Bc = -(hh * n * b2);
      C3 Cc = hh * a2 * d;
      const bool on = wgt != 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float svc = get(sv, c);
        const bool ok = on && svc >= 0.f && svc <= 1.f;     // (outside the clamp of the SSIM term: no gradient)
        put(A, c, ok ? wgt * get(A, c) : 0.f);
        put(Bc, c, ok ? wgt * get(Bc, c) : 0.f);
        put(Cc, c, ok ? wgt * get(Cc, c) : 0.f);
      }
      c0.a = hsum3(A);
      c0.b = hsum3(Bc);
      c0.c = hsum3(Cc);
    }
    // ------------------------------------------------------------------ stage C: output row q = y - 2 (r2, centres c2 c1 c0)
    const int qy = y - 2;
    if (it >= 3 && qy >= q_lo && qy <= q_hi) {
      const bool l1_on = r2.sel == nf + f;
      const C3 ga = (c2.a + c1.a) + c0.a, gb = (c2.b + c1.b) + c0.b, gc = (c2.c + c1.c) + c0.c;
      C3 dpred = ga + gb * r2.rx + gc * r2.rt;
      if (l1_on) {
        const C3 df = r2.rx - r2.rt;
        const float w1 = r2.pm * wl1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float dfc = get(df, c);
          put(dpred, c, get(dpred, c) + w1 * (dfc > 0.f ? 1.f : (dfc < 0.f ? -1.f : 0.f)));
        }
      }
      if (!col_own) dpred = c3(0.f);
      const float du = dot3(dpred, r2.Jx);
      const float dv = dot3(dpred, r2.Jy);
      if (du != 0.f || dv != 0.f) {
        float dX, dY, dZ;
        if (FISH) {
          float dq[3];
          mei_cam2image_bwd(mei, r2.X, r2.Y, r2.Z, du, dv, dq);
          dX = dq[0]; dY = dq[1]; dZ = dq[2];
        } else {
          const float iz = __builtin_amdgcn_rcpf(r2.Z);
          dX = du * iz; dY = dv * iz;
          dZ = -(du * r2.X + dv * r2.Y) * iz * iz;
        }
        const int qyr = min(max(refl(qy, H), 0), H - 1);
        float ray[3];
        ray_of(qyr, ray);
        const float pr0 = Pm[0] * ray[0] + Pm[1] * ray[1] + Pm[2] * ray[2];
        const float pr1 = Pm[4] * ray[0] + Pm[5] * ray[1] + Pm[6] * ray[2];
        const float pr2 = Pm[8] * ray[0] + Pm[9] * ray[1] + Pm[10] * ray[2];
        const float dD = dX * pr0 + dY * pr1 + dZ * pr2;
        const float cam[3] = {r2.D * ray[0], r2.D * ray[1], r2.D * ray[2]};
        const float dxyz[3] = {dX, dY, dZ};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) dPacc[i * 4 + j] += dxyz[i] * cam[j];
          dPacc[i * 4 + 3] += dxyz[i];
        }
        // transpose of the bilinear depth upsample
        if (unit_scale) {
          atomicAdd(ddout + (unsigned)(qyr * w + xr), dD);
        } else {
          const float fyu = sh * (float)qyr;
          const int dy0 = h > 1 ? min((int)fyu, h - 2) : 0;
          const float dly = h > 1 ? fyu - (float)dy0 : 0.f;
          const int li = (dy0 - ly_min) * LDS_C + (dx0 - lx_min);
          if (li >= 0 && dx0 >= lx_min && li + LDS_C + 1 < LDS_R * LDS_C && dx0 - lx_min + 1 < LDS_C) {
            atomicAdd(&lds[li], (1.f - dly) * (1.f - dlx) * dD);
            atomicAdd(&lds[li + 1], (1.f - dly) * dlx * dD);
            atomicAdd(&lds[li + LDS_C], dly * (1.f - dlx) * dD);
            atomicAdd(&lds[li + LDS_C + 1], dly * dlx * dD);
          } else {       // (strips of an unexpected aspect: straight to memory)
            const int hh1 = min(dy0 + 1, h - 1), ww1 = min(dx0 + 1, w - 1);
            atomicAdd(ddout + dy0 * w + dx0, (1.f - dly) * (1.f - dlx) * dD);
            atomicAdd(ddout + dy0 * w + ww1, (1.f - dly) * dlx * dD);
            atomicAdd(ddout + hh1 * w + dx0, dly * (1.f - dlx) * dD);
            atomicAdd(ddout + hh1 * w + ww1, dly * dlx * dD);
          }
        }
      }
    }
  };

  const int nsteps = BRH + 4 + (last_y ? 1 : 0);
  BRow A = {}, B = {}, C = {};
  CRow ca = {}, cb = {}, cc = {};
  A.sel = B.sel = C.sel = -1;
  for (int it = 0; it < nsteps; it += 3) {
    step(B, C, A, cb, cc, ca, it);
    if (it + 1 < nsteps) step(C, A, B, cc, ca, cb, it + 1);
    if (it + 2 < nsteps) step(A, B, C, ca, cb, cc, it + 2);
  }
  // ---- per-strip partial of d loss / d P_f (reduced in a fixed order by fs_photo_pose_grad) ----
  {
    const long tile = (long)sy * SX + sx, tiles = (long)SY * SX;
    float* out = p.dP + ((((long)s * p.B + b) * tiles + tile) * nf + f) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float v = wave_sum(dPacc[k]);
      if (lane == 0) out[k] = v;
    }
  }
  if (!unit_scale) {
    for (int i = lane; i < LDS_R * LDS_C; i += 64) {
      const float v = lds[i];
      if (v != 0.f) {
        const int yy = ly_min + i / LDS_C, xx = lx_min + i % LDS_C;
        if (yy < h && xx < w) atomicAdd(ddout + yy * w + xx, v);
      }
    }
  }
}

}  // namespace
