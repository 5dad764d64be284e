// Photometric loss chain over N = 1..4 temporal source frames (train_cfg.frame_ids = [0, a, ...], pinhole camera): the
// kernels of photo_fused.hip with a frame count.  frame_ids = [0, a, b] keeps running on those; this file is the path of
// every other count (and takes N = 2 as well, which its tests hold against the two-source path).
// Replaces (reference): MonoDepth2Decoder._generate_images_pred, compute_reprojection_loss and the per-pixel minimum of
// compute_total_reprojection_loss (monodepth2_decoder.py:61-128, 205-292) for any length of frame_ids.
//
// Forward: photo_fwd_body.h, the body photo_fused_fwd_kernel runs, walking the strip once per frame pair with the running
// minimum parked in LDS between the walks.
// Backward: photo_bwd_body.h, the body photo_fused_bwd_kernel runs, with the frame index taken modulo N.
// Setup, identity planes and pose gradient (fs_photo_multi_setup / _identity / _pose_grad) are the kernels of
// photometric.hip, built unfused there.
// FS_HIPCC_FLAGS: -fno-slp-vectorize
// (as in photo_fused.hip)
#include <algorithm>
#define FS_PHOTO_CONTRACT_FAST
#include "photo_common.h"
#pragma clang fp contract(fast)
#include "photo_bwd_body.h"
#include "photo_fwd_body.h"

namespace {

template <bool WRITE_PRED>
__global__ __launch_bounds__(256) void photo_multi_fwd_kernel(const FsPhotoMultiArgs p, int SX, int SY, int nwaves) {
  // the running minimum of the strip's pixels between two pair walks: slot [row][lane], owned by the lane
  __shared__ float s_best[4][FRH][64];
  __shared__ uint8_t s_bi[4][FRH][64];
  const int wid = (int)threadIdx.x >> 6;
  photo_fwd_body<WRITE_PRED, false, NFrames>(p, SX, SY, nwaves, s_best[wid], s_bi[wid]);
}

__global__ __launch_bounds__(256) void photo_multi_bwd_kernel(const FsPhotoMultiArgs p, int SX, int SY, int nwaves) {
  __shared__ float s_dd[4][LDS_R * LDS_C];
  photo_bwd_body<false, NFrames>(p, SX, SY, nwaves, s_dd);
}

bool valid(const FsPhotoMultiArgs* a) {
  return a && a->nsrc >= 1 && a->nsrc <= MAXF && photo_args_ok(a, a->nsrc) && photo_planes_32bit(a);
}

}  // namespace

extern "C" int fs_photo_multi_fwd(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || (!a->ident && !a->motion_mask) || !a->sel || !a->loss_sums) return FS_EINVAL;
  if ((a->pred != nullptr) != (a->ov != nullptr)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + FW - 1) / FW, SY = (a->H + FRH - 1) / FRH;
  const long nwaves = (long)a->B * a->S * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  if (a->pred) hipLaunchKernelGGL(photo_multi_fwd_kernel<true>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  else hipLaunchKernelGGL(photo_multi_fwd_kernel<false>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int64_t fs_photo_multi_bwd_tiles(int H, int W) {
  if (H < 2 || W < 2) return -1;
  return (int64_t)((W + BW - 1) / BW) * ((H + BRH - 1) / BRH);
}

extern "C" int fs_photo_multi_bwd(const FsPhotoMultiArgs* a, void* stream) {
  if (!valid(a) || !a->sel || !a->dP || !a->mask_sum) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || !a->d_depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + BW - 1) / BW, SY = (a->H + BRH - 1) / BRH;
  const long nwaves = (long)a->B * a->S * a->nsrc * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  hipLaunchKernelGGL(photo_multi_bwd_kernel, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int fs_photo_multi_strip(int which, int32_t* cols, int32_t* rows) {
  if (!cols || !rows || which < 0 || which > 2) return FS_EINVAL;
  *cols = which == 0 ? ID_W : (which == 1 ? FW : BW);
  *rows = which == 0 ? ID_RS : (which == 1 ? FRH : BRH);
  return 0;
}
