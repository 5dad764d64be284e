"""Sparse-VO depth post-optimisation with the reference's names (monodepth/networks/utils/postopt_utils.py:8-11,
27-53, 94-102, 170-226).  post_optimization runs on the device through ops.post_optimize (csrc/postopt.hip): one
fixed launch sequence, no host round trip.  The reference's SLIC / select_best_vo_points are folded into that call."""
import os

import numpy as np
import torch

from fsnet_amd.hip import ops
from fsnet_amd.monodepth.data.datasets.utils import read_vo_depth

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def denorm(image, rgb_mean, rgb_std):
    """[H,W,3] normalised -> uint8 (float64 arithmetic, truncating cast; reference :8-11)"""
    new_image = np.clip((image * rgb_std + rgb_mean) * 255, 0, 255)
    return np.array(new_image, dtype=np.uint8)


def depth_image_to_point_cloud_array(depth_image):
    """[H,W] depth -> [H,W,3] float32 point map (x = column, y = row, z = depth) (reference :94-102)"""
    w_range = np.arange(0, depth_image.shape[1], dtype=np.float32)
    h_range = np.arange(0, depth_image.shape[0], dtype=np.float32)
    w_grid, h_grid = np.meshgrid(w_range, h_range)
    return np.stack([w_grid, h_grid, depth_image], axis=2)


def resize_nearest(src, w, h):
    """cv2.resize(src, (w, h), interpolation=INTER_NEAREST) restated from OpenCV's resizeNN: source index =
    min(floor(d * (n_src / n_dst)), n_src - 1), the scale in float64"""
    src = np.asarray(src)
    H, W = src.shape[:2]
    xs = np.minimum(np.floor(np.arange(w, dtype=np.float64) * (1.0 / (float(w) / float(W)))).astype(np.int64), W - 1)
    ys = np.minimum(np.floor(np.arange(h, dtype=np.float64) * (1.0 / (float(h) / float(H)))).astype(np.int64), H - 1)
    return src[ys][:, xs]


def vo_path_of(dataset, index, vo_folder=None):
    """<vo_folder>/<sequence>/<frame:010d>.png for the KITTI raw layout (reference :40-47)"""
    instance = dataset.imdb[index]
    vo_folder = '/data/kitti_depth_sfm/sfm_depth_png' if vo_folder is None else vo_folder
    return os.path.join(vo_folder, instance['folder'].split('/')[1], "%010d.png" % instance['index'])


def read_sparse_vo(dataset, index, output_h, output_w, vo_folder=None):
    """float64 [output_h, output_w] VO depth of frame `index` (reference :27-53, KITTI branch; the KITTI-360 branch is
    not carried).  A missing file raises FileNotFoundError."""
    return resize_nearest(read_vo_depth(vo_path_of(dataset, index, vo_folder)), output_w, output_h)


def post_optimization(image, depth_image, depth_prediction, reference_depth, h_seg, w_seg,
                      lab_dist_weight=1, iter_num=5, depth_dist_weight=1, image_dist_weight=1,
                      lambda0=0.000, lambda1=1.0, lambda2=0.001, max_distance=100, max_points=800):
    """the reference's signature and defaults (:170-178; max_distance is unused there too).  image: host uint8
    [H,W,3] (denorm's output); depth_image: the point map of depth_prediction (depth_image_to_point_cloud_array);
    depth_prediction: [H,W] tensor; reference_depth: [H,W] VO depth (numpy or tensor).  Returns the refined depth as a
    device tensor [H,W]."""
    u8 = np.asarray(image)
    assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3
    H, W = u8.shape[:2]
    assert np.asarray(depth_image).shape == (H, W, 3)
    dev = depth_prediction.device if isinstance(depth_prediction, torch.Tensor) and depth_prediction.is_cuda \
        else torch.device('cuda', torch.cuda.current_device())
    # the kernel takes a normalised image and denormalises it with truncation: u8 + 0.5 with mean 0, std 1/255
    # comes back as u8 exactly ((u8 + 0.5) / 255 * 255 is within 1e-12 of u8 + 0.5)
    img = torch.from_numpy(u8.transpose(2, 0, 1).astype(np.float32) + 0.5).to(dev)
    depth = torch.as_tensor(depth_prediction).to(dev, torch.float32).reshape(H, W)
    vo = torch.as_tensor(np.asarray(reference_depth) if not isinstance(reference_depth, torch.Tensor)
                         else reference_depth).to(dev, torch.float32).reshape(H, W)
    out = ops.post_optimize(img[None], depth[None], vo[None], h_seg=h_seg, w_seg=w_seg, iter_num=iter_num,
                            lab_dist_weight=lab_dist_weight, depth_dist_weight=depth_dist_weight,
                            image_dist_weight=image_dist_weight, lambda0=lambda0, lambda1=lambda1, lambda2=lambda2,
                            max_points=max_points, rgb_mean=(0.0, 0.0, 0.0), rgb_std=(1 / 255.0,) * 3)
    return out[0]
