"""Kitti360FisheyeEvaluator with the reference's module path, class name and methods
(monodepth/evaluation/kitti360_fisheye_eval.py:1-145), on the device:

  - `_precompute` reads the split and the image sizes on the host, then reads the velodyne scans one group of
    `group_size` frames at a time and projects each group through the Mei model in one fs_lidar_mei_depth call, so at
    most `group_size` scans are held in host memory (the reference: per-point f64 numpy
    and a scatter per frame, :97-145).  The last point in scan order wins a pixel, as numpy's fancy assignment decides
    it; the reference's duplicate search (:83-91) runs sub2ind on untruncated float coordinates and finds no duplicate
    in practice, so it is not restated.  Points whose truncated pixel index falls outside the image are dropped (the
    reference would fail or wrap the index; with KITTI-360's mirror parameter none does).
  - `_single_loss` is fs_depth_eval_masked: 0.3 < gt < 60 (float32 comparisons) and the close mask, no crop, then the
    KITTI median scaling, clamp and errors (:43-72).  No valid pixel: ValueError, like the reference.

Deliberate deviation: a cached `gt_saved_file` also loads its `close_masks` (the reference loads only `data` and then
fails in single_call on the missing attribute).  The file format is the reference's: `data` float32 [N, H, W] and
`close_masks` bool [N, H, W] written by np.savez_compressed.

`gt_depths=` / `close_masks=` / `device=` are conveniences of this package (as on KittiEigenEvaluator): ground truth
given directly; close_masks default to all-true."""
import os

import numpy as np
import torch

from fsnet_amd.hip import ops
from fsnet_amd.monodepth.data.datasets.fisheye_dataset import (extract_P_from_fisheye_calib,
                                                               read_cam2velo_from_sequence, read_fisheycalib)
from fsnet_amd.monodepth.data.datasets.fisheye_dataset import read_extrinsic_from_sequence as read_fisheye_extrinsic
from .kitti_unsupervised_eval import Kitti360LidarExport, KittiEigenEvaluator, stack_maps

GT_LO, GT_HI = 0.3, 60.0     # kitti360_fisheye_eval.py:47


class Kitti360FisheyeEvaluator(Kitti360LidarExport, KittiEigenEvaluator):
    def __init__(self, data_path=None, split_file=None, gt_saved_file=None, is_evaluate_absolute=False, gt_depths=None,
                 close_masks=None, device=None, group_size=8):
        self.is_evaluate_absolute = is_evaluate_absolute
        self.device = device
        self.group_size = int(group_size)
        self._gt_dev = {}
        self._mask_dev = {}
        if gt_depths is not None:
            self.gt_depths = gt_depths
            self.close_masks = close_masks if close_masks is not None else [
                np.ones(np.shape(g)[:2], dtype=bool) for g in gt_depths]
        elif gt_saved_file is not None and os.path.isfile(gt_saved_file):
            f = np.load(gt_saved_file, fix_imports=True, encoding='latin1', allow_pickle=True)
            self.gt_depths, self.close_masks = f["data"], f["close_masks"]
        else:
            if data_path is None or split_file is None:
                raise ValueError("Kitti360FisheyeEvaluator: no cached ground truth (gt_saved_file=%r) and no data_path "
                                 "/ split_file to export it from" % (gt_saved_file,))
            print("Start exporting ground truth depths specified by %s to %s" % (split_file, gt_saved_file))
            self._precompute(data_path, split_file, gt_saved_file)

    def _load_calib(self, calib_dir):
        """reference :16-36 (without the host projector: the projection is fs_lidar_mei_depth)"""
        left_calib = read_fisheycalib(os.path.join(calib_dir, "image_02.yaml"))
        right_calib = read_fisheycalib(os.path.join(calib_dir, "image_03.yaml"))
        self.cam_calib = dict(left_calib=left_calib, right_calib=right_calib,
                              T_image2pose=read_fisheye_extrinsic(os.path.join(calib_dir, "calib_cam_to_pose.txt")),
                              P0=extract_P_from_fisheye_calib(left_calib), P1=extract_P_from_fisheye_calib(right_calib),
                              T_cam2velo=read_cam2velo_from_sequence(os.path.join(calib_dir, "calib_cam_to_velo.txt")))

    def velo_to_camera(self):
        """T_velo2cam02, composed exactly as the reference does (:106-108)"""
        T_cam002pose = self.cam_calib['T_image2pose']['T_image0']
        T_cam022pose = self.cam_calib['T_image2pose']['T_image2']
        return np.linalg.inv(T_cam022pose) @ T_cam002pose @ np.linalg.inv(self.cam_calib['T_cam2velo'])

    def mei_row(self):
        """gamma1, gamma2, u0, v0, k1, k2, xi of the left camera: the values _cam2image reads (P0 and left_calib)"""
        P, c = self.cam_calib['P0'], self.cam_calib['left_calib']
        return np.array([P[0, 0], P[1, 1], P[0, 2], P[1, 2], c["distortion_parameters"]["k1"],
                         c["distortion_parameters"]["k2"], c["mirror_parameters"]["xi"]], dtype=np.float64)

    def _precompute(self, data_path, split_file, gt_saved_file):
        self._load_calib(os.path.join(data_path, 'calibration'))
        maps = self._export_lidar(data_path, split_file, 'image_02', 'data_rgb', ops.LidarMeiDepth,
                                  self.velo_to_camera(), self.mei_row())
        gt_depths = [depth for depth, _ in maps]
        masks = [close.astype(bool) for _, close in maps]
        if gt_saved_file is not None:
            np.savez_compressed(gt_saved_file, data=stack_maps(gt_depths), close_masks=stack_maps(masks))
        self.gt_depths = gt_depths
        self.close_masks = masks

    def _mask(self, index, device):
        m = self._mask_dev.get(index)
        if m is None or m.device != device:
            m = torch.as_tensor(np.asarray(self.close_masks[index], dtype=np.uint8)).to(device)
            if len(self._mask_dev) < 4096:
                self._mask_dev[index] = m
        return m

    def _errors(self, depth_0, gt, close_mask):
        dev = self._device_for(depth_0)
        pred = torch.as_tensor(depth_0, dtype=torch.float32).to(dev)
        gt = torch.as_tensor(gt, dtype=torch.float32).to(dev)
        mask = torch.as_tensor(np.asarray(close_mask, dtype=np.uint8) if not isinstance(close_mask, torch.Tensor)
                               else close_mask).to(dev)
        return ops.depth_eval_masked(pred[None], gt[None], mask[None], lo=GT_LO, hi=GT_HI, crop=False)[0]

    def _single_loss(self, depth_0, gt_depth, close_mask):
        """depth_0: predicted depth [h, w] (device tensor, or numpy as in the reference); gt_depth / close_mask: [H, W]"""
        out = self._errors(depth_0, gt_depth, close_mask).cpu().numpy()
        if out[15] == 0:
            raise ValueError
        return dict(ratio=np.float32(out[0]), error=tuple(out[1:8]), abs_error=tuple(out[8:15]))

    def single_call(self, depth_0, index):
        dev = self._device_for(depth_0)
        return self._single_loss(depth_0, self._gt(index, dev), self._mask(index, dev))

    def device_errors(self, depth_0, index):
        """f64 [16] on the device: ratio, err[7], abs_err[7], n_valid of the fisheye metric (the evaluation hooks)"""
        return self._errors(depth_0, self._gt(index, depth_0.device), self._mask(index, depth_0.device))

