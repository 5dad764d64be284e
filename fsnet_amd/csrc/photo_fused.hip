// Fused photometric forward: warp (backproject -> project -> bilinear grid_sample, border padding) + SSIM/L1
// reprojection loss for both source frames + per-pixel minimum against the identity terms + masked sum, for ALL
// scales, in one launch — the warped images never reach HBM (fs_photo_warp + fs_photo_loss_fwd wrote and re-read
// 8 x [B,3,H,W] floats, and staged the target tile once per scale).
// Replaces (reference): MonoDepth2Decoder._generate_images_pred (monodepth2_decoder.py:61-116; FishEyeDecoder
// :355-411), compute_reprojection_loss (:118-128; SSIM monodepth_utils.py:184-215) and the per-pixel min / masking
// of compute_total_reprojection_loss (:226-272, 292).
// (Structure of the kernel: photo_fwd_body.h.)
// FS_HIPCC_FLAGS: -fno-slp-vectorize
// (SLP packing into v_pk_add/mul_f32 costs register shuffles here and keeps the DPP shifts from folding into the adds)
#include <algorithm>
// photo_common.h's row helpers (hsum3, f2, ldg) under this file's contraction mode: the header switches it on in front of
// them and it stays on from there — last include, so that it reaches nothing but this file's own code
#define FS_PHOTO_CONTRACT_FAST
#include "photo_common.h"

// fused multiply-adds allowed in this file (the library builds with -ffp-contract=off to mirror the unfused ATen
// arithmetic of the staged kernels; here an FMA only removes a rounding and a third of the VALU instructions)
#pragma clang fp contract(fast)
// the channel triple C3, the 8-byte tap pair load ldg2 and the whole backward body: shared with photo_multi.hip
#include "photo_bwd_body.h"

// the forward kernel's body (FW, FRH, Row and the row step): shared with photo_multi.hip
#include "photo_fwd_body.h"

namespace {

// one pair, both frames there: no pair loop and no LDS slot for the running minimum (photo_fwd_body.h)
template <bool WRITE_PRED, bool FISH>
__global__ __launch_bounds__(256) void photo_fused_fwd_kernel(const FsPhotoArgs p, int SX, int SY, int nwaves) {
  photo_fwd_body<WRITE_PRED, FISH, TwoFrames>(p, SX, SY, nwaves, nullptr, nullptr);
}


// =============================================================================================================
// Fused backward: d loss / d depth_s and the per-strip partials of d loss / d P_f, recomputing the warp instead
// of reading the eight warped images back (fs_photo_loss_bwd staged pred + target tiles per scale through LDS).
// A wave owns (batch element, scale, source frame, strip of 60 columns x 32 rows) and walks the rows once with two
// register rings, three stages per step at row y:
//   A  warp row y (both the values and the sampler Jacobian d pred / d (ix, iy)), horizontal window sums
//   B  window centre y-1: SSIM-derivative coefficients A + B x(q) + C t(q) for this frame where the per-pixel minimum
//      selected it (sel == 2 + f), horizontally box-summed (the transpose of the window gather)
//   C  output row y-2: vertical box sum of the coefficient rows -> d loss / d pred, + the L1 term, through the sampler
//      Jacobian, the projection and the depth upsample.
// Reflection padding: halo lanes / rows hold the reflected pixel; the virtual positions x = -1, W and y = -1, H
// (which receive window contributions of the border centres) push their gradient through the reflected pixel's
// chain — the chain is linear in d pred, so that equals folding them onto the reflected pixel.
// =============================================================================================================
// (BW, BRH, the low-res LDS tile, the row structs and the kernel's body: photo_bwd_body.h, shared with photo_multi.hip)

template <bool FISH>
__global__ __launch_bounds__(256) void photo_fused_bwd_kernel(const FsPhotoArgs p, int SX, int SY, int nwaves) {
  __shared__ float s_dd[4][LDS_R * LDS_C];
  photo_bwd_body<FISH, TwoFrames>(p, SX, SY, nwaves, s_dd);
}

}  // namespace

extern "C" int fs_photo_fused_fwd(const FsPhotoArgs* a, void* stream) {
  if (!photo_args_ok(a, 2) || (!a->ident && !a->motion_mask) || !a->sel || !a->loss_sums) return FS_EINVAL;
  if (!photo_fisheye_ok(a) || !photo_planes_32bit(a)) return FS_EINVAL;
  if ((a->pred != nullptr) != (a->ov != nullptr)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s]) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + FW - 1) / FW, SY = (a->H + FRH - 1) / FRH;
  const long nwaves = (long)a->B * a->S * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x7fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  const bool fish = a->lut_ptrs != nullptr;
  if (a->pred) {
    if (fish) hipLaunchKernelGGL((photo_fused_fwd_kernel<true, true>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
    else hipLaunchKernelGGL((photo_fused_fwd_kernel<true, false>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  } else {
    if (fish) hipLaunchKernelGGL((photo_fused_fwd_kernel<false, true>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
    else hipLaunchKernelGGL((photo_fused_fwd_kernel<false, false>), grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  }
  return fs_launch_status();
}

extern "C" int64_t fs_photo_fused_bwd_tiles(int H, int W) {
  if (H < 2 || W < 2) return -1;
  return (int64_t)((W + BW - 1) / BW) * ((H + BRH - 1) / BRH);
}

extern "C" int fs_photo_fused_bwd(const FsPhotoArgs* a, void* stream) {
  if (!photo_args_ok(a, 2) || !a->sel || !a->dP || !a->mask_sum) return FS_EINVAL;
  if (!photo_fisheye_ok(a) || !photo_planes_32bit(a)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || !a->d_depth[s]) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + BW - 1) / BW, SY = (a->H + BRH - 1) / BRH;
  const long nwaves = (long)a->B * a->S * 2 * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x7fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  if (a->lut_ptrs) hipLaunchKernelGGL(photo_fused_bwd_kernel<true>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  else hipLaunchKernelGGL(photo_fused_bwd_kernel<false>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}
