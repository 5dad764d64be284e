// Photometric loss chain over N = 1..4 temporal source frames on the fisheye / Mei ray tables (FishEyeDecoder with
// train_cfg.frame_ids = [0, a, ...]): the kernels of photo_multi.hip with the ray-table geometry of photo_fused.hip's
// fisheye instantiation.  frame_ids = [0, a, b] keeps running on photo_fused.hip; this file is the path of every other
// count (and takes N = 2 as well, which its tests hold against the two-source path).
// Replaces (reference): FishEyeDecoder._generate_images_pred (monodepth2_decoder.py:355-413) followed by
// compute_reprojection_loss and the per-pixel minimum of compute_total_reprojection_loss (:118-128, 205-292) for any
// length of frame_ids.
//
// Forward: photo_fwd_body.h with FISH = true and the policy NFramesMei (photo_common.h): a strip is walked once per frame
// pair, the running minimum parked in LDS between the walks; the ray-table projection addresses the pair's geo entries.
// Backward: photo_bwd_body.h with FISH = true, the frame index taken modulo N.
// Setup: fs_photo_mei_multi_setup (photometric.hip, K = identity).  Identity planes, tile count, strip sizes and pose
// gradient are those of the pinhole chain as they are (fs_photo_multi_identity / _bwd_tiles / _strip / _pose_grad): none
// of them has any geometry, and with K = identity the pose gradient is dT itself.
// (A file of its own, not three more kernels in photo_multi.hip: tests/test_photo64n_cpu.py holds that file to its three.)
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
__global__ __launch_bounds__(256) void photo_mei_multi_fwd_kernel(const FsPhotoMeiMultiArgs p, int SX, int SY, int nwaves) {
  // the running minimum of the strip's pixels between two pair walks: slot [row][lane], owned by the lane
  __shared__ float s_best[4][FRH][64];
  __shared__ uint8_t s_bi[4][FRH][64];
  const int wid = (int)threadIdx.x >> 6;
  photo_fwd_body<WRITE_PRED, true, NFramesMei>(p, SX, SY, nwaves, s_best[wid], s_bi[wid]);
}

__global__ __launch_bounds__(256) void photo_mei_multi_bwd_kernel(const FsPhotoMeiMultiArgs p, int SX, int SY, int nwaves) {
  __shared__ float s_dd[4][LDS_R * LDS_C];
  photo_bwd_body<true, NFramesMei>(p, SX, SY, nwaves, s_dd);
}

// what fs_photo_multi_* refuse, and the ray tables or their parameters missing
bool valid(const FsPhotoMeiMultiArgs* a) {
  return a && a->nsrc >= 1 && a->nsrc <= MAXF && photo_args_ok(a, a->nsrc) && photo_planes_32bit(a) && a->lut_ptrs && a->mei;
}

}  // namespace

extern "C" int fs_photo_mei_multi_fwd(const FsPhotoMeiMultiArgs* a, void* stream) {
  if (!valid(a) || (!a->ident && !a->motion_mask) || !a->sel || !a->loss_sums) return FS_EINVAL;
  if ((a->pred != nullptr) != (a->ov != nullptr)) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + FW - 1) / FW, SY = (a->H + FRH - 1) / FRH;
  const long nwaves = (long)a->B * a->S * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  if (a->pred) hipLaunchKernelGGL(photo_mei_multi_fwd_kernel<true>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  else hipLaunchKernelGGL(photo_mei_multi_fwd_kernel<false>, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}

extern "C" int fs_photo_mei_multi_bwd(const FsPhotoMeiMultiArgs* a, void* stream) {
  if (!valid(a) || !a->sel || !a->dP || !a->mask_sum) return FS_EINVAL;
  for (int s = 0; s < a->S; ++s) if (!a->depth[s] || !a->d_depth[s] || a->dh[s] < 1 || a->dw[s] < 1) return FS_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int SX = (a->W + BW - 1) / BW, SY = (a->H + BRH - 1) / BRH;
  const long nwaves = (long)a->B * a->S * a->nsrc * SY * SX;
  const long nblk = photo_blocks(nwaves, 8);
  if (nblk > 0x1fffffffL) return FS_EINVAL;
  const dim3 grid((unsigned)nblk), blk(256);
  hipLaunchKernelGGL(photo_mei_multi_bwd_kernel, grid, blk, 0, st, *a, SX, SY, (int)nwaves);
  return fs_launch_status();
}
