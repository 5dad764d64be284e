"""KittiEigenEvaluator with the reference's constructor and methods (monodepth/evaluation/
kitti_unsupervised_eval.py:11-127).  `_single_loss` runs on the device: resize to the ground truth's size, valid mask
+ Garg crop, median scaling, clamp and the seven depth errors are one HIP launch per image (fs_depth_eval), so a
validation pass does not copy depth maps to the host.  KittiEigenEvaluator exports its ground truth on the host
(`_precompute`, :27-45, generate_depth_map) or, with export_on_device, through fs_lidar_pinhole_depth; called with a
folder of saved predictions it scores those (:102-161).  Kitti360Evaluator (:164-212) exports it on the device, with the loop
(Kitti360LidarExport) that Kitti360FisheyeEvaluator's export runs too.  Every device export here and the nuScenes
evaluator's walk its frames with size_runs and keep their op with lidar_op."""
import os
from itertools import groupby

import numpy as np
import torch

from fsnet_amd.hip import ops


def stack_maps(maps):
    """maps of one size as one array [N, H, W]; of several sizes (the Eigen split mixes recording dates whose rectified
    image sizes differ: 375x1242, 370x1224, 376x1241 ...) as an object array, which a ragged list only becomes when
    asked (the reference's np.array(gts) relied on an older NumPy doing that implicitly; NumPy >= 1.24 raises).  The
    evaluators load their caches with allow_pickle=True."""
    if len({m.shape for m in maps}) <= 1:
        return np.array(maps)
    arr = np.empty(len(maps), dtype=object)
    for k, m in enumerate(maps):
        arr[k] = m
    return arr


def size_runs(records, key, group_size):
    """Yields `records` in order as lists: runs of consecutive records of equal key(record), at most `group_size`
    long — what one call of a LiDAR op takes (one H, W per call), and what is held in host memory at a time."""
    for _, run in groupby(records, key):
        run = list(run)
        for start in range(0, len(run), group_size):
            yield run[start:start + group_size]


def lidar_op(op, op_cls, shape, device):
    """`op` while it is an `op_cls` whose maps have `shape` — (G, H, W), or (G, C, H, W) — else a new
    op_cls(*shape, device): an op's buffers are kept from group to group while the shape holds."""
    if type(op) is not op_cls or tuple(op.depth.shape) != tuple(shape):
        op = op_cls(*shape, device)
    return op


class KittiEigenEvaluator(object):
    def __init__(self, data_path=None, split_file=None, gt_saved_file=None, is_evaluate_absolute=False, gt_depths=None,
                 device=None, export_on_device=False, group_size=8):
        """export_on_device (an addition, default off): a missing ground-truth cache is exported by
        fs_lidar_pinhole_depth, `group_size` scans per call (_precompute_on_device), instead of generate_depth_map
        per scan on the host.  Same maps, same cache."""
        self.is_evaluate_absolute = is_evaluate_absolute
        self.device = device
        self.export_on_device = bool(export_on_device)
        self.group_size = int(group_size)
        if gt_depths is not None:
            self.gt_depths = gt_depths
        elif gt_saved_file is not None and os.path.isfile(gt_saved_file):
            self.gt_depths = np.load(gt_saved_file, fix_imports=True, encoding='latin1', allow_pickle=True)["data"]
        else:
            if data_path is None or split_file is None:
                raise ValueError("KittiEigenEvaluator: no cached ground truth (gt_saved_file=%r) and no data_path / "
                                 "split_file to export it from" % (gt_saved_file,))
            print("Start exporting ground truth depths specified by %s to %s" % (split_file, gt_saved_file))
            if self.export_on_device:
                self._precompute_on_device(data_path, split_file, gt_saved_file)
            else:
                self._precompute(data_path, split_file, gt_saved_file)
        self._gt_dev = {}

    def _precompute(self, data_path, split_file, gt_saved_file):
        """ground truth of a split from the raw velodyne scans, cached as <gt_saved_file> (reference :27-46)"""
        from fsnet_amd.monodepth.networks.utils.monodepth_utils import generate_depth_map
        gts = []
        with open(split_file, "r") as f:
            for line in f:
                if not line.strip():
                    continue
                folder, frame_id, _ = line.split()
                scan = os.path.join(data_path, folder, "velodyne_points/data", "{:010d}.bin".format(int(frame_id)))
                gts.append(generate_depth_map(os.path.join(data_path, folder.split("/")[0]), scan, 2, True).astype(np.float32))
        if gt_saved_file is not None:
            np.savez_compressed(gt_saved_file, data=stack_maps(gts))
        self.gt_depths = gts

    def _precompute_on_device(self, data_path, split_file, gt_saved_file):
        """_precompute with the projection on the device: per recording date P_velo2im and (H, W) as
        generate_depth_map composes them (kitti_velo_to_image, f64 on the host); each group of size_runs is one
        fs_lidar_pinhole_depth call, each frame with its own matrix.  At most `group_size` scans are held in host
        memory.  The maps equal generate_depth_map(..., 2, True).astype(float32) bit for bit."""
        from fsnet_amd.monodepth.data.datasets.utils import read_pc_from_bin
        from fsnet_amd.monodepth.networks.utils.monodepth_utils import kitti_velo_to_image
        calib, frames = {}, []              # frames: (scan path, P [3, 4], h, w)
        with open(split_file, "r") as f:
            for line in f:
                if not line.strip():
                    continue
                folder, frame_id, _ = line.split()
                date = folder.split("/")[0]
                if date not in calib:
                    calib[date] = kitti_velo_to_image(os.path.join(data_path, date), 2)
                P, (h, w) = calib[date]
                frames.append((os.path.join(data_path, folder, "velodyne_points/data",
                                            "{:010d}.bin".format(int(frame_id))), P, int(h), int(w)))
        dev = self._device_for()
        gts, op = [], None
        for group in size_runs(frames, lambda fr: fr[2:], self.group_size):
            op = lidar_op(op, ops.LidarPinholeDepth, (len(group),) + group[0][2:], dev)
            op.stage([read_pc_from_bin(fr[0]) for fr in group], np.stack([fr[1] for fr in group]))
            gts.extend(op.run().cpu().numpy())
        if gt_saved_file is not None:
            np.savez_compressed(gt_saved_file, data=stack_maps(gts))
        self.gt_depths = gts

    def _device_for(self, depth_0=None):
        """the device of the prediction, else the configured one, else the current one"""
        if isinstance(depth_0, torch.Tensor) and depth_0.is_cuda:
            return depth_0.device
        return self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def _gt(self, index, device):
        g = self._gt_dev.get(index)
        if g is None or g.device != device:
            g = torch.as_tensor(np.asarray(self.gt_depths[index], dtype=np.float32)).to(device)
            if len(self._gt_dev) < 4096:
                self._gt_dev[index] = g
        return g

    def _depth_eval(self, pred, gt):
        """pred [B, h, w], gt [B, H, W] on the device -> f64 [B, 16]: ratio, err[7], abs_err[7], n_valid
        (fs_depth_eval).  An evaluator with another metric of these two arguments overrides this alone."""
        return ops.depth_eval(pred, gt)

    def _single_loss(self, depth_0, gt_depth):
        """depth_0: predicted depth [h, w] (device tensor, or numpy as in the reference); gt_depth: [H, W]."""
        dev = self._device_for(depth_0)
        pred = torch.as_tensor(depth_0, dtype=torch.float32).to(dev)
        gt = torch.as_tensor(gt_depth, dtype=torch.float32).to(dev)
        out = self._depth_eval(pred[None], gt[None])[0].cpu().numpy()
        if out[15] == 0:
            raise ValueError
        return dict(ratio=np.float32(out[0]), error=tuple(out[1:8]), abs_error=tuple(out[8:15]))

    def single_call(self, depth_0, index):
        return self._single_loss(depth_0, self._gt(index, self._device_for(depth_0)))

    def device_errors(self, depth_0, index):
        """f64 [16] on the device: ratio, err[7], abs_err[7], n_valid of frame `index` (_depth_eval) — what the
        evaluation hooks collect; each evaluator supplies its own metric here"""
        return self._depth_eval(depth_0[None], self._gt(index, depth_0.device)[None])[0]

    def log(self, writer, mean_errors, mean_abs_errors, global_step=0, epoch_num=0, is_print=True):
        log_str = f"Epoch {epoch_num}"
        log_str += "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
        log_str += "\n" + ("&{: 8.3f}  " * 7).format(*np.asarray(mean_errors).tolist()) + "\\\\"
        log_str += f"\nEpoch {epoch_num}| Abs Error without Scaled"
        log_str += "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
        log_str += "\n" + ("&{: 8.3f}  " * 7).format(*np.asarray(mean_abs_errors).tolist()) + "\\\\"
        if writer is not None:
            writer.add_text("evaluation logs", log_str.replace(' ', '&nbsp;').replace('\n', '  \n'), global_step=epoch_num)
        if is_print:
            print(log_str)
        return log_str


    def __call__(self, result_path, writer=None, global_step=0, epoch_num=0):
        """The Eigen metric over a folder of saved predictions, 16-bit PNGs of depth * 256 in the order of the ground
        truth (reference :102-161; KittiEvaluationHook(save_depth_dir=...) writes such a folder).  Per file: read_depth,
        then fs_depth_eval against the cached ground truth, as for a live prediction.  Prints the reference's log with
        the mean and standard deviation of the median ratios; returns what the hooks return (the reference returns
        None), or None when the file count differs from the ground truth's."""
        from fsnet_amd.monodepth.data.datasets.utils import read_depth
        filelist = sorted(os.listdir(result_path))
        if len(filelist) != len(self.gt_depths):
            print(f"The length of pred_depths is {len(filelist)} while the length of gt_depths is {len(self.gt_depths)}")
            print("Drop evaluation")
            return None
        dev = self._device_for()
        rows = [self.device_errors(torch.from_numpy(read_depth(os.path.join(result_path, name))).to(dev), i)
                for i, name in enumerate(filelist)]
        res = torch.stack(rows).cpu().numpy()
        if (res[:, 15] == 0).any():
            raise ValueError
        mean_errors, mean_abs_errors, scales = res[:, 1:8].mean(0), res[:, 8:15].mean(0), res[:, 0]
        log_str = f"Epoch {epoch_num} | Scaled Error | {scales.mean()}, {scales.std()}"
        log_str += "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
        log_str += "\n" + ("&{: 8.3f}  " * 7).format(*mean_errors.tolist()) + "\\\\"
        log_str += f"\nEpoch {epoch_num} | Abs Error without Scaled"
        log_str += "\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
        log_str += "\n" + ("&{: 8.3f}  " * 7).format(*mean_abs_errors.tolist()) + "\\\\"
        if writer is not None:
            writer.add_text("evaluation logs", log_str.replace(' ', '&nbsp;').replace('\n', '  \n'), global_step=epoch_num)
        print(log_str)
        return dict(mean_errors=mean_errors, mean_abs_errors=mean_abs_errors, ratios=scales)


class Kitti360LidarExport(object):
    """The ground-truth export loop of the KITTI-360 evaluators, which set `group_size`: at most that many scans are
    held in host memory and projected per call of a LiDAR op."""

    def _export_lidar(self, data_path, split_file, camera, image_subdir, op_cls, *frame_args):
        """Reads the comma-separated split and, for its size, each frame of `camera`/`image_subdir`; per group of
        size_runs reads the scans, stages them and `frame_args` (the same for every frame) in an
        `op_cls(G, H, W, device)` (lidar_op) and runs it.  Returns, per frame, the tuple of host arrays the op puts
        out."""
        from PIL import Image
        from fsnet_amd.monodepth.data.datasets.utils import read_pc_from_bin
        img_dir = os.path.join(data_path, 'data_2d_raw')
        pc_dir = os.path.join(data_path, 'data_3d_raw')
        frames = []                       # (scan path, h, w): the scans are read one group at a time below
        with open(split_file, 'r') as f:
            for line in f.readlines():
                sequence_name, _, img_index, _, _ = line.strip().split(',')
                frame_id = int(img_index)
                with Image.open(os.path.join(img_dir, sequence_name, camera, image_subdir,
                                             "{:010d}.png".format(frame_id))) as im:
                    w, h = im.size
                frames.append((os.path.join(pc_dir, sequence_name, "velodyne_points/data",
                                            "{:010d}.bin".format(frame_id)), h, w))
        dev = self._device_for()
        maps, op = [], None
        for group in size_runs(frames, lambda fr: fr[1:], self.group_size):
            op = lidar_op(op, op_cls, (len(group),) + group[0][1:], dev)
            op.stage([read_pc_from_bin(fr[0]) for fr in group], *[np.stack([a] * len(group)) for a in frame_args])
            out = op.run()
            maps.extend(zip(*[o.cpu().numpy() for o in (out if isinstance(out, tuple) else (out,))]))
        return maps


class Kitti360Evaluator(Kitti360LidarExport, KittiEigenEvaluator):
    """KITTI-360 perspective evaluation (reference :164-212): the Eigen metric of the parent, unchanged, on ground truth
    exported from the raw velodyne scans through image_00's rectified pinhole camera.  `_precompute` reads the split and
    the image sizes on the host, composes P_velo2img in f64 as the reference does, and projects `group_size` scans per
    fs_lidar_pinhole_depth call (the reference: project_depth_map per frame, a Python loop over every duplicate index;
    the host form is monodepth_utils.project_depth_map).  At most `group_size` scans are held in host memory.  The cache
    is the reference's: `data` float32 [N, H, W] written by np.savez_compressed, an object array when sizes differ."""

    def __init__(self, data_path=None, split_file=None, gt_saved_file=None, is_evaluate_absolute=False, gt_depths=None,
                 device=None, group_size=8):
        super().__init__(data_path, split_file, gt_saved_file, is_evaluate_absolute, gt_depths, device,
                         group_size=group_size)

    def _load_calib(self, calib_dir):
        from fsnet_amd.monodepth.data.datasets.kitti360_dataset import read_P01_from_sequence, read_T_from_sequence
        P0, _, R0, _ = read_P01_from_sequence(os.path.join(calib_dir, "perspective.txt"))
        self.cam_calib = dict(P0=P0, R0=R0,
                              T_cam2velo=read_T_from_sequence(os.path.join(calib_dir, "calib_cam_to_velo.txt")))

    def velo_to_image(self):
        """P_velo2img [3, 4] f64, composed exactly as the reference does (:190)"""
        return self.cam_calib['P0'] @ self.cam_calib['R0'] @ np.linalg.inv(self.cam_calib['T_cam2velo'])

    def _precompute(self, data_path, split_file, gt_saved_file):
        self._load_calib(os.path.join(data_path, 'calibration'))
        gts = [depth for depth, in self._export_lidar(data_path, split_file, 'image_00', 'data_rect',
                                                      ops.LidarPinholeDepth, self.velo_to_image())]
        if gt_saved_file is not None:
            np.savez_compressed(gt_saved_file, data=stack_maps(gts))
        self.gt_depths = gts
