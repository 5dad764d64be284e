"""KittiEvaluationHook with the reference's constructor and call signature
(monodepth/pipeline_hooks/evaluation_hooks/base_evaluation_hooks.py:19-67): eval-mode forward over the validation set,
crop to the effective size, inverse-depth resize to the original image size, per-image errors, mean + log.
Everything between the network output and the 15 numbers per image stays on the device (fs_resize_linear with
invert, then the evaluator's device_errors: fs_depth_eval for KITTI, fs_depth_eval_masked for the KITTI-360 fisheye
evaluator); only those numbers are copied back.  Samples of the mirrored augmentation classes (raw frames plus a
device plan, e.g. KITTI360FisheyeDataset with its validation Resize) are collated and resized by DeviceAugment.  KittiEvaluationHook_postopt (:69-127) refines the
prediction with sparse visual-odometry depth first (ops.post_optimize, one call per batch on the device).  Both hooks
take an optional `save_depth_dir` and then also write every frame's prediction as a 16-bit PNG (_save_depth).
FastNuscEvaluationHook (:141-202) and PostOptFastNuscEvaluationHook (:204-288) are the nuScenes passes: depth (not
inverse depth) resized, scored per file name by NuscenesEvaluator, means per camera and over the cameras."""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from fsnet_amd.hip import ops
from fsnet_amd.monodepth.data.datasets.utils import write_png16
from fsnet_amd.monodepth.networks.utils import postopt_utils as PU
from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, DeviceAugment
from fsnet_amd.vision_base.data.datasets.dataset_utils import collate_fn
from fsnet_amd.vision_base.utils.builder import build


def _collate(samples):
    """collate_fn, or DeviceAugment.collate for samples of the mirrored augmentation classes (a validation Resize
    plan: the frames it names are resized on the device by _materialize)"""
    if PLAN not in samples[0]:
        return collate_fn(samples)
    keys = (samples[0][PLAN].get("resize") or {}).get("keys", [('image', 0)])
    idxs = [k[1] for k in keys if isinstance(k, tuple) and k[0] == 'image']
    batch = DeviceAugment(idxs).collate(samples)
    batch[PLAN]["frame_idxs"] = idxs
    return batch


def _materialize(batched_data):
    if PLAN in batched_data:
        return DeviceAugment(batched_data[PLAN]["frame_idxs"]).materialize(batched_data)
    return batched_data


def _original_hw(batched_data, i):
    """the size of the image before the validation Resize: ('original_image', 0) as in the reference, or the
    ('image_resize', 'original_shape') the Resize records (a validation chain without a Copy, such as
    configs/kitti360_fisheye_example's, carries no original image)"""
    if ('original_image', 0) in batched_data:
        return tuple(int(v) for v in batched_data[('original_image', 0)][i].shape[:2])
    return tuple(int(v) for v in batched_data[('image_resize', 'original_shape')][i])


class KittiEvaluationHook(object):
    def __init__(self, test_run_hook_cfg, dataset_eval_cfg=None, save_depth_dir=None, **kwargs):
        self.test_hook = build(**test_run_hook_cfg)
        self.dataset_eval_func = None if dataset_eval_cfg is None else build(**dataset_eval_cfg)
        self.save_depth_dir = save_depth_dir
        for key in kwargs:
            setattr(self, key, kwargs[key])

    def _save_depth(self, depth_0, frame_index):
        """with save_depth_dir (an addition; None = nothing is written): the full-resolution prediction as
        <save_depth_dir>/<frame_index:010d>.png, uint16(depth * 256) — what KittiEigenEvaluator.__call__ and
        kitti_supervised_eval read.  Quantised on the device (fs_depth_quantize_u16), copied back as two bytes per pixel."""
        if self.save_depth_dir is None:
            return
        os.makedirs(self.save_depth_dir, exist_ok=True)
        write_png16(os.path.join(self.save_depth_dir, "%010d.png" % frame_index),
                    ops.depth_quantize_u16(depth_0).cpu().numpy())

    @torch.no_grad()
    def __call__(self, meta_arch, dataset_val, writer=None, global_step=0, epoch_num=0):
        meta_arch.eval()
        batch_size = getattr(self, 'batch_size', 1)
        num_workers = getattr(self, 'num_workers', 4)
        dataloader = DataLoader(dataset_val, batch_size, shuffle=False, num_workers=num_workers, collate_fn=_collate)
        rows = []
        frame_index = 0
        for batched_data in dataloader:
            batched_data = _materialize(batched_data)
            output_dict = self.test_hook(batched_data, meta_arch, global_step, epoch_num)
            depth_b = output_dict['depth']
            for i in range(depth_b.shape[0]):
                depth = depth_b[i, 0]
                h_eff, w_eff = (int(v) for v in batched_data[('image_resize', 'effective_size')][i])
                depth = depth[0:h_eff, 0:w_eff].float().contiguous()
                h, w = _original_hw(batched_data, i)
                depth_0 = ops.resize_linear(depth, h, w, invert=True)          # 1 / cv2.resize(1 / depth, (w, h))
                rows.append(self.dataset_eval_func.device_errors(depth_0, frame_index))
                self._save_depth(depth_0, frame_index)
                frame_index += 1
        res = torch.stack(rows).cpu().numpy()
        if (res[:, 15] == 0).any():
            raise ValueError
        mean_errors, mean_abs_errors = res[:, 1:8].mean(0), res[:, 8:15].mean(0)
        self.dataset_eval_func.log(writer, mean_errors, mean_abs_errors, global_step=global_step, epoch_num=epoch_num)
        meta_arch.train()
        return dict(mean_errors=mean_errors, mean_abs_errors=mean_abs_errors, ratios=res[:, 0])


class KittiEvaluationHook_postopt(KittiEvaluationHook):
    """KittiEvaluationHook with the sparse-VO post-optimisation in front of the metrics (reference :69-127):
    post_opt_cfg (dict or EasyDict) overrides lab_dist_weight, depth_dist_weight, image_dist_weight, h_seg, w_seg,
    iter_num, lambda0, lambda1, lambda2 (hook defaults 1, 1, 1, 10, 18, 3, 0.54/180, 1, 0.4) and, as an addition,
    max_points (800); vo_path is the folder of the VO depth PNGs (read_sparse_vo).  Each batch is refined in one
    ops.post_optimize call, then evaluated like KittiEvaluationHook.

    Deliberate deviations from the reference:
      - the image is cropped to the effective size together with the depth (the reference pairs the full-size image
        with the cropped depth, which fails whenever the two differ, and its bare except hides the failure);
      - sample i uses its own image (the reference uses image[0] for every sample; the same at batch_size 1);
      - a batch that carries ('vo_depth', 0) is refined with it (the reference reads it and then skips refinement);
        it must have the effective size, else ValueError;
      - no bare except: a frame whose VO file is missing is evaluated unrefined and counted in n_unrefined; any other
        error propagates."""
    PARAM_DEFAULTS = dict(lab_dist_weight=1, depth_dist_weight=1, image_dist_weight=1, h_seg=10, w_seg=18, iter_num=3,
                          lambda0=0.54 / (10 * 18), lambda1=1.0, lambda2=0.4, max_points=800)

    def _post_opt_params(self):
        cfg = getattr(self, 'post_opt_cfg', None) or dict()
        params = dict(self.PARAM_DEFAULTS)
        for key in params:
            if key in cfg:
                params[key] = cfg[key]
        return params, cfg.get('vo_path', None)

    def _vo_of(self, batched_data, dataset_val, i, frame_index, h, w, vo_path, device):
        if ('vo_depth', 0) in batched_data:
            vo = batched_data[('vo_depth', 0)][i]
            vo = vo if isinstance(vo, torch.Tensor) else torch.as_tensor(np.asarray(vo))
            if tuple(vo.shape) != (h, w):
                raise ValueError("('vo_depth', 0) of sample %d is %s, the effective size is %s" % (
                    i, tuple(vo.shape), (h, w)))
        else:
            try:
                vo = torch.from_numpy(PU.read_sparse_vo(dataset_val, frame_index, h, w, vo_folder=vo_path))
            except FileNotFoundError:
                return None
        return vo.to(device, torch.float32)

    @torch.no_grad()
    def __call__(self, meta_arch, dataset_val, writer=None, global_step=0, epoch_num=0):
        meta_arch.eval()
        params, vo_path = self._post_opt_params()
        batch_size = getattr(self, 'batch_size', 1)
        num_workers = getattr(self, 'num_workers', 4)
        dataloader = DataLoader(dataset_val, batch_size, shuffle=False, num_workers=num_workers, collate_fn=_collate)
        rows = []
        frame_index = 0
        n_refined = n_unrefined = 0
        for batched_data in dataloader:
            batched_data = _materialize(batched_data)
            output_dict = self.test_hook(batched_data, meta_arch, global_step, epoch_num)
            depth_b = output_dict['depth']
            image_b = batched_data[('image', 0)]
            B = depth_b.shape[0]
            crops, groups = [], {}
            for i in range(B):
                h_eff, w_eff = (int(v) for v in batched_data[('image_resize', 'effective_size')][i])
                depth = depth_b[i, 0, 0:h_eff, 0:w_eff].float()
                vo = self._vo_of(batched_data, dataset_val, i, frame_index + i, h_eff, w_eff, vo_path, depth.device)
                crops.append(depth.contiguous())
                if vo is None:
                    n_unrefined += 1
                    continue
                image = torch.as_tensor(image_b[i])[:, 0:h_eff, 0:w_eff].to(depth.device, torch.float32)
                groups.setdefault((h_eff, w_eff), []).append((i, image, depth, vo))
            for items in groups.values():       # one call per batch (per effective size, which a batch shares)
                refined = ops.post_optimize(torch.stack([t[1] for t in items]), torch.stack([t[2] for t in items]),
                                            torch.stack([t[3] for t in items]), rgb_mean=PU.IMAGENET_MEAN,
                                            rgb_std=PU.IMAGENET_STD, **params)
                for j, t in enumerate(items):
                    crops[t[0]] = refined[j]
                n_refined += len(items)
            for i in range(B):
                h, w = _original_hw(batched_data, i)
                depth_0 = ops.resize_linear(crops[i], h, w, invert=True)          # 1 / cv2.resize(1 / depth, (w, h))
                rows.append(self.dataset_eval_func.device_errors(depth_0, frame_index))
                self._save_depth(depth_0, frame_index)
                frame_index += 1
        res = torch.stack(rows).cpu().numpy()
        if (res[:, 15] == 0).any():
            raise ValueError
        mean_errors, mean_abs_errors = res[:, 1:8].mean(0), res[:, 8:15].mean(0)
        self.dataset_eval_func.log(writer, mean_errors, mean_abs_errors, global_step=global_step, epoch_num=epoch_num)
        meta_arch.train()
        return dict(mean_errors=mean_errors, mean_abs_errors=mean_abs_errors, ratios=res[:, 0],
                    errors=res[:, 1:8], abs_errors=res[:, 8:15], n_refined=n_refined, n_unrefined=n_unrefined)


class FastNuscEvaluationHook(object):
    """The nuScenes validation pass (reference :141-202): per sample the prediction is cropped to the effective size
    and resized to the original image size — depth, not inverse depth, as the reference does here
    (fs_resize_linear, invert off) — then scored against the ground-truth PNG its ('filename', 0) names
    (NuscenesEvaluator.device_errors: fs_depth_eval_masked with the nuScenes crop as its mask).  Samples without a usable point are skipped with the
    reference's warning.  Means per camera in first-seen order, then the mean of the camera means; `log` per camera
    and for 'all mean'.  Only the 16 numbers per sample are copied back, once, after the last batch.

    save_depth_dir (an addition, default None = nothing is written): every prediction as
    <save_depth_dir>/predict_depth/<CAM>/<name>.png, uint16(depth * 256) — the folder NuscenesEvaluator.__call__
    scores when called with save_depth_dir."""

    def __init__(self, test_run_hook_cfg, dataset_eval_cfg=None, save_depth_dir=None, **kwargs):
        self.test_hook = build(**test_run_hook_cfg)
        self.dataset_eval_func = None if dataset_eval_cfg is None else build(**dataset_eval_cfg)
        self.save_depth_dir = save_depth_dir
        for key in kwargs:
            setattr(self, key, kwargs[key])

    def _save_depth(self, depth_0, camera_type, filename):
        if self.save_depth_dir is None:
            return
        d = os.path.join(self.save_depth_dir, 'predict_depth', camera_type)
        os.makedirs(d, exist_ok=True)
        name = os.path.splitext(os.path.basename(filename))[0] + '.png'
        write_png16(os.path.join(d, name), ops.depth_quantize_u16(depth_0).cpu().numpy())

    def _crops(self, batched_data, output_dict):
        """the predictions of a batch cropped to their effective sizes: device fp32 [h_eff, w_eff] each"""
        depth_b = output_dict['depth']
        crops = []
        for i in range(depth_b.shape[0]):
            h_eff, w_eff = (int(v) for v in batched_data[('image_resize', 'effective_size')][i])
            crops.append(depth_b[i, 0, 0:h_eff, 0:w_eff].float().contiguous())
        return crops

    @torch.no_grad()
    def __call__(self, meta_arch, dataset_val, writer=None, global_step=0, epoch_num=0):
        meta_arch.eval()
        batch_size = getattr(self, 'batch_size', 16)
        num_workers = getattr(self, 'num_workers', 4)
        dataloader = DataLoader(dataset_val, batch_size, shuffle=False, num_workers=num_workers, collate_fn=_collate)
        cams, names, rows = [], [], []
        for batched_data in dataloader:
            batched_data = _materialize(batched_data)
            output_dict = self.test_hook(batched_data, meta_arch, global_step, epoch_num)
            for i, depth in enumerate(self._crops(batched_data, output_dict)):
                h, w = _original_hw(batched_data, i)
                depth_0 = ops.resize_linear(depth, h, w, invert=False)          # cv2.resize(depth, (w, h))
                camera_type = batched_data['camera_type'][i]
                filename = batched_data[('filename', 0)][i]
                self._save_depth(depth_0, camera_type, filename)
                if self.dataset_eval_func is not None:
                    cams.append(camera_type)
                    names.append(filename)
                    rows.append(self.dataset_eval_func.device_errors(depth_0, filename))
        meta_arch.train()
        if self.dataset_eval_func is None:
            return None
        res = torch.stack(rows).cpu().numpy() if rows else np.zeros((0, 16))
        errors, abs_errors = dict(), dict()
        for cam, filename, row in zip(cams, names, res):
            errors.setdefault(cam, [])
            abs_errors.setdefault(cam, [])
            if row[15] == 0:
                import warnings
                warnings.warn(f"image at sample {filename}  has no usable points")
                continue
            errors[cam].append(row[1:8])
            abs_errors[cam].append(row[8:15])
        per_cam, all_mean_errors, all_mean_errors_abs = dict(), [], []
        for cam in errors:
            mean_errors = np.array(errors[cam]).mean(0)
            mean_abs_errors = np.array(abs_errors[cam]).mean(0)
            self.dataset_eval_func.log(writer, cam, mean_errors, mean_abs_errors, global_step=global_step,
                                       epoch_num=epoch_num)
            per_cam[cam] = dict(mean_errors=mean_errors, mean_abs_errors=mean_abs_errors)
            all_mean_errors.append(mean_errors)
            all_mean_errors_abs.append(mean_abs_errors)
        all_mean_errors = np.array(all_mean_errors).mean(0)
        all_mean_errors_abs = np.array(all_mean_errors_abs).mean(0)
        self.dataset_eval_func.log(writer, 'all mean', all_mean_errors, all_mean_errors_abs, global_step=global_step,
                                   epoch_num=epoch_num)
        return dict(mean_errors=all_mean_errors, mean_abs_errors=all_mean_errors_abs, per_camera=per_cam)


class PostOptFastNuscEvaluationHook(FastNuscEvaluationHook):
    """FastNuscEvaluationHook with the sparse-VO post-optimisation in front of the resize (reference :204-288): each
    batch is refined in one ops.post_optimize call from its ('vo_depth', 0), which the dataset reads when it is given
    a vo_path.  post_opt_cfg overrides the parameters as for KittiEvaluationHook_postopt, whose deviations hold here
    too: the image is cropped to the effective size with the depth, ('vo_depth', 0) must have that size (ValueError),
    and a batch without ('vo_depth', 0) is scored unrefined (the reference raises KeyError)."""
    PARAM_DEFAULTS = KittiEvaluationHook_postopt.PARAM_DEFAULTS

    def _post_opt_params(self):
        cfg = getattr(self, 'post_opt_cfg', None) or dict()
        params = dict(self.PARAM_DEFAULTS)
        for key in params:
            if key in cfg:
                params[key] = cfg[key]
        return params

    def _crops(self, batched_data, output_dict):
        crops = super()._crops(batched_data, output_dict)
        if ('vo_depth', 0) not in batched_data:
            return crops
        groups = {}
        for i, depth in enumerate(crops):
            vo = batched_data[('vo_depth', 0)][i]
            vo = vo if isinstance(vo, torch.Tensor) else torch.as_tensor(np.asarray(vo))
            if tuple(vo.shape) != tuple(depth.shape):
                raise ValueError("('vo_depth', 0) of sample %d is %s, the effective size is %s" % (
                    i, tuple(vo.shape), tuple(depth.shape)))
            h_eff, w_eff = depth.shape
            image = torch.as_tensor(batched_data[('image', 0)][i])[:, 0:h_eff, 0:w_eff].to(depth.device, torch.float32)
            groups.setdefault((h_eff, w_eff), []).append((i, image, depth, vo.to(depth.device, torch.float32)))
        for items in groups.values():           # one call per batch (per effective size, which a batch shares)
            refined = ops.post_optimize(torch.stack([t[1] for t in items]), torch.stack([t[2] for t in items]),
                                        torch.stack([t[3] for t in items]), rgb_mean=PU.IMAGENET_MEAN,
                                        rgb_std=PU.IMAGENET_STD, **self._post_opt_params())
            for j, t in enumerate(items):
                crops[t[0]] = refined[j].contiguous()
        return crops
