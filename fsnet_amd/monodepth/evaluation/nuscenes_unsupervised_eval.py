"""NuscenesEvaluator with the reference's constructor and methods (monodepth/evaluation/
nuscenes_unsupervised_eval.py:17-320), without the nuScenes devkit and pyquaternion at run time: the tables are JSON
(vision_base.data.datasets.nuscenes_utils.NuScenes), the sweeps are float32 files, and the devkit's three helpers the
reference calls — LidarPointCloud.from_file / remove_close / transform, transform_matrix and Quaternion.rotation_matrix —
are restated here in numpy.

`_precompute` exports one LiDAR sweep per sample through its six cameras as 16-bit PNGs, <gt_saved_dir>/<CAM>/<name>.png.
It lists every sample's six jobs first (file name, size, matrix: metadata only), then walks them in groups of up to
`group_size` consecutive samples whose cameras' sizes agree (size_runs) and reads a group's sweeps inside the group.
With a GPU the projection, the last-writer scatter, the duplicate pass and the uint16 cast are fs_lidar_nusc_depth_u16,
one call per group; without one it is nusc_depth_u16 below, the kernel's operation order in numpy.  Both write the same
files.  generate_depth_map keeps the reference's signature and f64 result.

Scoring (`_single_loss`, `single_call`, `device_errors`, `__call__`) is fs_depth_eval_masked: 1e-3 < gt < 80, the median
ratio, the clamp and the seven errors of the KITTI evaluator, inside the reference's crop — which here starts at
0.03594771 of the height as of the width (the KITTI evaluators' Garg crop starts at 0.40810811 H) and so travels as the
kernel's mask.

Deviation: a depth of 256 m or more wraps in the reference's uint16 cast and saturates at 65535 here (kernel and host
mirror alike); the sensor does not reach that range."""
import os
import warnings
from functools import reduce

import numpy as np
import torch

from fsnet_amd.hip import ops
from fsnet_amd.monodepth.data.datasets.utils import read_png16, write_png16
from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import KittiEigenEvaluator, lidar_op, size_runs
from fsnet_amd.monodepth.networks.utils.monodepth_utils import scatter_depth
from fsnet_amd.vision_base.data.datasets.nuscenes_utils import NuScenes

CAMS = ['CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_RIGHT', 'CAM_BACK', 'CAM_BACK_LEFT', 'CAM_FRONT_LEFT']


def quaternion_rotation_matrix(q):
    """(w, x, y, z) -> [3, 3] f64 as pyquaternion's Quaternion(q).rotation_matrix makes it: normalised unless
    |1 - |q|^2| < 1e-14, then the lower-right block of Q(q) @ Qbar(q)^T"""
    q = np.array(q, dtype=np.float64)
    ss = np.dot(q, q)
    if not abs(1.0 - ss) < 1e-14:
        n = np.sqrt(ss)
        if n > 0:
            q = q / n
    w, x, y, z = q
    Q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Qbar = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(Q, Qbar.conj().transpose())[1:][:, 1:]


def transform_matrix(translation, rotation, inverse=False):
    """the devkit's geometry_utils.transform_matrix; rotation: quaternion (w, x, y, z)"""
    R = quaternion_rotation_matrix(rotation)
    tm = np.eye(4)
    if inverse:
        rot_inv = R.T
        tm[:3, :3] = rot_inv
        tm[:3, 3] = rot_inv.dot(np.transpose(-np.array(translation)))
    else:
        tm[:3, :3] = R
        tm[:3, 3] = np.transpose(np.array(translation))
    return tm


def read_lidar_points(path):
    """a .pcd.bin sweep as the devkit's LidarPointCloud holds it: float32 [4, n] (x, y, z, intensity of the 5 stored)"""
    return np.fromfile(path, dtype=np.float32).reshape((-1, 5))[:, :4].T


def remove_close(points, radius):
    """drop the points with |x| < radius and |y| < radius (the devkit's PointCloud.remove_close)"""
    close = np.logical_and(np.abs(points[0, :]) < radius, np.abs(points[1, :]) < radius)
    return points[:, np.logical_not(close)]


def get_lidar_data(nusc, sample_rec, nsweeps, min_distance):
    """at most nsweeps of lidar in the ego frame of the sample, f64 [5, N] (x, y, z, intensity, dt) (reference :17-70).
    The transformed points pass through the devkit's float32 storage."""
    points = np.zeros((5, 0))
    ref_sd_rec = nusc.get('sample_data', sample_rec['data']['LIDAR_TOP'])
    ref_pose_rec = nusc.get('ego_pose', ref_sd_rec['ego_pose_token'])
    ref_time = 1e-6 * ref_sd_rec['timestamp']
    car_from_global = transform_matrix(ref_pose_rec['translation'], ref_pose_rec['rotation'], inverse=True)
    current_sd_rec = ref_sd_rec
    for _ in range(nsweeps):
        pc = remove_close(read_lidar_points(os.path.join(nusc.dataroot, current_sd_rec['filename'])), min_distance)
        current_pose_rec = nusc.get('ego_pose', current_sd_rec['ego_pose_token'])
        global_from_car = transform_matrix(current_pose_rec['translation'], current_pose_rec['rotation'], inverse=False)
        current_cs_rec = nusc.get('calibrated_sensor', current_sd_rec['calibrated_sensor_token'])
        car_from_current = transform_matrix(current_cs_rec['translation'], current_cs_rec['rotation'], inverse=False)
        trans_matrix = reduce(np.dot, [car_from_global, global_from_car, car_from_current])
        pc = pc.copy()
        pc[:3, :] = trans_matrix.dot(np.vstack((pc[:3, :], np.ones(pc.shape[1]))))[:3, :]     # stored as float32
        time_lag = ref_time - 1e-6 * current_sd_rec['timestamp']
        times = time_lag * np.ones((1, pc.shape[1]))
        points = np.concatenate((points, np.concatenate((pc, times), 0)), 1)
        if current_sd_rec['prev'] == '':
            break
        current_sd_rec = nusc.get('sample_data', current_sd_rec['prev'])
    return points


MAX_POINTS = 81920        # rows of the padded sweep (reference :140-141)


def pad_or_trim_to_np(x, shape, pad_val=0):
    """a 2-D array cut or filled with pad_val, at the end of each axis, to `shape` (reference :72-77)"""
    x = np.asarray(x)
    rows, cols = int(shape[0]), int(shape[1])
    out = np.full((rows, cols), pad_val, dtype=x.dtype)
    r, c = min(rows, x.shape[0]), min(cols, x.shape[1])
    out[:r, :c] = x[:r, :c]
    return out


def get_samples(nusc):
    """every sample record, by scene and then by time (reference :128-134)"""
    return sorted(nusc.sample, key=lambda rec: (rec['scene_token'], rec['timestamp']))


def get_lidar(nusc, rec):
    """(float32 [81920, 5] padded sweep, float32 [81920] mask: 1 on the rows that hold a point) of one sample's key
    sweep, the points nearer than 2.2 m removed (reference :136-143)"""
    points = get_lidar_data(nusc, rec, nsweeps=1, min_distance=2.2).T
    padded = pad_or_trim_to_np(points, [MAX_POINTS, 5]).astype(np.float32)
    return padded, (np.arange(MAX_POINTS) < points.shape[0]).astype(np.float32)


def camera_extrinsics(sens):
    """T [4, 4] camera -> ego of a calibrated_sensor record (reference :189-195)"""
    T = np.eye(4)
    T[0:3, 0:3] = np.array(quaternion_rotation_matrix(sens['rotation']))
    T[0:3, 3] = np.array(sens['translation'])
    return T


def projection_matrix(extrinsics, intrinsics):
    """[4, 4] f64 homo_intrinsics @ inv(extrinsics), composed as the reference does (:91-95)"""
    homo_intrinsics = np.eye(4)
    homo_intrinsics[0:3, 0:3] = intrinsics
    return np.dot(homo_intrinsics, np.linalg.inv(extrinsics))


def generate_depth_map(velo, extrinsics, intrinsics, cam=2, im_shape=[900, 1600]):
    """sweep [N, >=3] in the ego frame -> sparse depth image of one camera ([H, W] f64, 0 = no return), the
    reference's function (:85-126) with its matrix products; the scatter and the duplicate pass are the KITTI
    export's (monodepth_utils.scatter_depth)."""
    N = velo.shape[0]
    homo_velo = np.ones([N, 4])
    homo_velo[:, 0:3] = velo[:, 0:3]
    pts = np.dot(projection_matrix(extrinsics, intrinsics), homo_velo.T).T
    pts = pts[pts[:, 2] > 0]
    pts[:, :2] = pts[:, :2] / (pts[:, 2][..., np.newaxis])
    pts[:, 0] = np.round(pts[:, 0]) - 1                   # (- 1: the KITTI matlab convention)
    pts[:, 1] = np.round(pts[:, 1]) - 1
    return scatter_depth(pts, im_shape)


def nusc_depth_u16(velo, M, im_shape):
    """The explicit-order mirror of fs_lidar_nusc_depth_u16 for one camera: velo float32 [N, >=3], M f64 [3, 4] (rows
    0..2 of projection_matrix) -> uint16 [H, W].  p_k = m_k0 x + m_k1 y + m_k2 z + m_k3 in f64, added in that order;
    p2 > 0; col / row = rint(p / p2) - 1; q = min(trunc(p2 * 256), 65535) per point; last writer, then the first
    pixel of every duplicate group takes the group's minimum q."""
    H, W = int(im_shape[0]), int(im_shape[1])
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    v = np.asarray(velo)
    x, y, z = (v[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all='ignore'):
        p = [M[k, 0] * x + M[k, 1] * y + M[k, 2] * z + M[k, 3] for k in range(3)]
        keep = p[2] > 0
        p0, p1, p2 = p[0][keep], p[1][keep], p[2][keep]
        col, row = np.rint(p0 / p2) - 1.0, np.rint(p1 / p2) - 1.0
        q = np.minimum(np.trunc(p2 * 256.0), 65535.0)
    pts = np.stack([col, row, q], axis=1)
    return scatter_depth(pts, [H, W]).astype(np.uint16)


class NuscenesEvaluator(KittiEigenEvaluator):
    def __init__(self, data_path, split_file, gt_saved_dir, nuscenes_version='v1.0-trainval',
                 is_evaluate_absolute=False, is_force_recompute=False, channels=CAMS, device=None,
                 export_on_device=None, group_size=4, gt_cache_bytes=2 << 30):
        """device, export_on_device, group_size and gt_cache_bytes are additions.  export_on_device: None = on the
        device when one is there; group_size samples x six cameras go into one fs_lidar_nusc_depth_u16 call;
        gt_cache_bytes: how much decoded ground truth (5.76 MB per 900 x 1600 map) is kept on the device between
        calls — files beyond it are decoded and uploaded each time they are scored."""
        self.is_evaluate_absolute = is_evaluate_absolute
        self.split_file = split_file
        self.device = device
        self.export_on_device = torch.cuda.is_available() if export_on_device is None else bool(export_on_device)
        self.group_size = int(group_size)
        with open(split_file, 'r') as f:
            self.token_list = [line.strip().split(',')[0] for line in f.readlines()]
        if (not os.path.isdir(gt_saved_dir)) or is_force_recompute:
            print(f"Start exporting ground truth depths specified by {nuscenes_version} to {gt_saved_dir}")
            self._precompute(data_path, gt_saved_dir, nuscenes_version)
        self.channels = channels
        self.gt_saved_dir = gt_saved_dir
        self._gt_dev, self._gt_bytes, self.gt_cache_bytes = {}, 0, int(gt_cache_bytes)

    # ---- ground-truth export -------------------------------------------------------------------------------------
    def _export_jobs(self, nusc, rec, gt_saved_dir):
        """per camera of one sample: (png path, (H, W), M [3, 4])"""
        jobs = []
        for cam in CAMS:
            samp = nusc.get('sample_data', rec['data'][cam])
            filename = samp['filename']
            depth_name = filename.replace('samples', gt_saved_dir).replace('.jpg', '.png')
            sens = nusc.get('calibrated_sensor', samp['calibrated_sensor_token'])
            P = projection_matrix(camera_extrinsics(sens), np.array(sens['camera_intrinsic']))
            jobs.append((depth_name, (int(samp['height']), int(samp['width'])), P[:3]))
        return jobs

    def _precompute(self, data_path, gt_saved_dir, nuscenes_version):
        nusc = NuScenes(version=nuscenes_version, dataroot=data_path, verbose=True)
        for cam in CAMS:
            os.makedirs(os.path.join(gt_saved_dir, cam), exist_ok=True)
        samples = []                       # (sample record, jobs): metadata only; a group's sweeps are read below
        for token in self.token_list:
            rec = nusc.get('sample', token)
            samples.append((rec, self._export_jobs(nusc, rec, gt_saved_dir)))
        for group in size_runs(samples, lambda s: [j[1] for j in s[1]], self.group_size):
            sweeps = []                    # float32 [n, 4] each
            for rec, _ in group:
                lidar_data, lidar_mask = get_lidar(nusc, rec)
                sweeps.append(np.ascontiguousarray(lidar_data[lidar_mask == 1, :4]))
            for (_, jobs), planes in zip(group, self._project(sweeps, [s[1] for s in group])):
                for (depth_name, _, _), plane in zip(jobs, planes):
                    write_png16(depth_name, plane)

    def _project(self, sweeps, jobs):
        """-> per sample, per camera, the uint16 plane [H, W].  On the device when export_on_device and the cameras
        of a sample share one size (fs_lidar_nusc_depth_u16 takes one H, W per call); the host mirror otherwise."""
        sizes = {j[1] for sample in jobs for j in sample}
        if self.export_on_device and len(sizes) != 1:
            print("NuscenesEvaluator: cameras of %d sizes in one group (%s): this group is exported on the host" % (
                len(sizes), sorted(sizes)))
        if not self.export_on_device or len(sizes) != 1:
            return [[nusc_depth_u16(s, j[2], j[1]) for j in sample] for s, sample in zip(sweeps, jobs)]
        (H, W), = sizes
        op = self._op = lidar_op(getattr(self, '_op', None), ops.LidarNuscDepth, (len(sweeps), len(CAMS), H, W),
                                 self._device_for())
        op.stage(sweeps, np.stack([np.stack([j[2] for j in sample]) for sample in jobs]))
        return op.run().cpu().numpy()

    # ---- scoring -------------------------------------------------------------------------------------------------
    METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")

    def log(self, writer, channel, mean_errors, mean_abs_errors, global_step=0, epoch_num=0, is_print=True):
        """the reference's two tables of one channel (:203-216), median-scaled and unscaled, as one string: printed,
        and added to the writer under "Evaluation logs/<channel>" at step epoch_num"""
        head = "  " + "".join("{:>8} | ".format(m) for m in self.METRICS)
        blocks = []
        for title, values in (("", mean_errors), (" | Abs Error without Scaled", mean_abs_errors)):
            row = "".join("&{: 8.3f}  ".format(v) for v in np.asarray(values).tolist()) + "\\\\"
            blocks.append("Epoch %s for channel %s%s\n%s\n%s" % (epoch_num, channel, title, head, row))
        log_str = "\n".join(blocks)
        if writer is not None:
            writer.add_text("Evaluation logs/%s" % channel, log_str.replace(' ', '&nbsp;').replace('\n', '  \n'),
                            global_step=epoch_num)
        if is_print:
            print(log_str)
        return log_str

    def _gt_path(self, filename):
        return filename.replace('samples', self.gt_saved_dir).replace('.jpg', '.png')

    def _gt(self, path, device):
        """the ground truth of one file on `device`: read_png16 / 256 as float32 (read_depth), uploaded once while the
        maps kept so far stay under gt_cache_bytes"""
        g = self._gt_dev.get(path)
        if g is None or g.device != device:
            g = torch.from_numpy(np.array(read_png16(path).astype(np.float64) / 256.0, dtype=np.float32)).to(device)
            size = g.numel() * g.element_size()
            if path not in self._gt_dev and self._gt_bytes + size <= self.gt_cache_bytes:
                self._gt_dev[path] = g
                self._gt_bytes += size
        return g

    def _crop_mask(self, B, H, W, device):
        """uint8 [B, H, W]: the reference's crop (:223-227), rows and columns both from 0.03594771 — not the Garg crop
        of the KITTI evaluators, whose rows start at 0.40810811 H"""
        masks = self.__dict__.setdefault('_crop_masks', {})
        key = (H, W, str(device))
        if key not in masks:
            crop = np.array([0.03594771 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)
            m = torch.zeros(H, W, dtype=torch.uint8)
            m[crop[0]:crop[1], crop[2]:crop[3]] = 1
            masks[key] = m.to(device)
        return masks[key][None].expand(B, H, W).contiguous()

    def _depth_eval(self, pred, gt):
        """pred [B, h, w], gt [B, H, W] on the device -> f64 [B, 16] (fs_depth_eval_masked: 1e-3 < gt < 80, the crop
        as its mask, then the resize, median ratio, clamp and seven errors of fs_depth_eval)"""
        B, H, W = gt.shape
        return ops.depth_eval_masked(pred, gt, self._crop_mask(B, H, W, gt.device), lo=1e-3, hi=80.0, crop=False)

    def single_call(self, depth_0, filename):
        return self._single_loss(depth_0, self._gt(self._gt_path(filename), self._device_for(depth_0)))

    def device_errors(self, depth_0, filename):
        """f64 [16] on the device: ratio, err[7], abs_err[7], n_valid of the file"""
        return self._depth_eval(depth_0[None], self._gt(self._gt_path(filename), depth_0.device)[None])[0]

    def __call__(self, result_path, writer=None, global_step=0, epoch_num=0, batch_size=16):
        """Scores <result_path>/predict_depth/<CAM>/*.png against <gt_saved_dir>/<CAM>/ (reference :257-320), each
        camera's folder in device batches of `batch_size` files of one size.  Files without a usable point are
        skipped with the reference's warning.  Returns what the hooks return (the reference returns None)."""
        dev = self._device_for()
        per_cam, all_mean_errors, all_mean_errors_abs = {}, [], []
        for cam in self.channels:
            predict_dir = os.path.join(result_path, 'predict_depth', cam)
            filelist = os.listdir(predict_dir)
            gt_dir = os.path.join(self.gt_saved_dir, cam)
            print(f'Evaminating images at {predict_dir} against {gt_dir}')
            rows, batch = [], []

            def flush():
                if batch:
                    rows.append(self._depth_eval(torch.stack([b[0] for b in batch]), torch.stack([b[1] for b in batch])))
                    del batch[:]

            for image_file in filelist:
                gt = self._gt(os.path.join(gt_dir, image_file), dev)
                pred = torch.from_numpy(np.array(read_png16(os.path.join(predict_dir, image_file)).astype(np.float64)
                                                 / 256.0, dtype=np.float32)).to(dev)
                if batch and (batch[0][0].shape != pred.shape or batch[0][1].shape != gt.shape):
                    flush()
                batch.append((pred, gt))
                if len(batch) == batch_size:
                    flush()
            flush()
            res = torch.cat(rows).cpu().numpy() if rows else np.zeros((0, 16))
            for image_file, row in zip(filelist, res):
                if row[15] == 0:
                    sample_token = image_file.split('.')[0]
                    warnings.warn(f"image at sample {sample_token} from camera {cam} as no usable points")
            res = res[res[:, 15] != 0]
            print(res[:, 1:8].shape, cam)
            mean_errors, mean_abs_errors = res[:, 1:8].mean(0), res[:, 8:15].mean(0)
            self.log(writer, cam, mean_errors, mean_abs_errors, global_step=global_step, epoch_num=epoch_num)
            per_cam[cam] = dict(mean_errors=mean_errors, mean_abs_errors=mean_abs_errors, ratios=res[:, 0])
            all_mean_errors.append(mean_errors)
            all_mean_errors_abs.append(mean_abs_errors)
        all_mean_errors = np.array(all_mean_errors).mean(0)
        all_mean_errors_abs = np.array(all_mean_errors_abs).mean(0)
        self.log(writer, 'all mean', all_mean_errors, all_mean_errors_abs, global_step=global_step, epoch_num=epoch_num)
        return dict(mean_errors=all_mean_errors, mean_abs_errors=all_mean_errors_abs, per_camera=per_cam)

