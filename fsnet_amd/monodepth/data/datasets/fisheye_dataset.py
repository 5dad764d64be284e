"""KITTI-360 fisheye triplet dataset with the reference's module path, class name, constructor keys and sample contract
(monodepth/data/datasets/fisheye_dataset.py:1-262), on the base it shares with the perspective dataset
(kitti360_triplet.KITTI360TripletDataset): comma-separated split "sequence, pose index, image index, former,
latter" -> image / pose index triplets, the Mei calibration of both fisheye cameras (image_02.yaml / image_03.yaml),
camera-to-pose extrinsics, data_poses -> ('relative_pose', f), raw uint8 frames under ('image', f), P2 / original_P2 /
calib_meta of the camera drawn for the sample and a float64 patched_mask — then the configured augmentation.  With the
mirrored augmentation classes the frames stay uint8 and the pixel work runs on the device (DeviceAugment).

Random draws: one np.random.rand() per __getitem__ when use_right_image is true (left camera below 0.5), in the
reference's order, before the augmentation's own draws.

Deliberate deviation: the fisheye mask is read from the configured `fisheye_mask` path (the reference reads a
hard-coded '/home/monodepth/meta_data/kitti360_trainsub/fisheye_mask.png' whenever the key is set, :161-163).  It is
resized to the frame's size with cv2's INTER_NEAREST rule when the sizes differ and handed on as float64."""
import os
from copy import deepcopy

import numpy as np

from fsnet_amd.monodepth.data.datasets.kitti360_triplet import (  # noqa: F401  (the readers keep their names here)
    KITTI360TripletDataset, _read_camera_lines, read_cam2velo_from_sequence, read_poses_file)


def read_extrinsic_from_sequence(file):
    """calib_cam_to_pose.txt: lines "image_0k: r00 ... t2" -> dict(T_image0..T_image3) of 4x4 camera-to-pose
    transforms, identity for a camera the file does not list (reference :16-43)"""
    T = _read_camera_lines(file, ["image_00", "image_01", "image_02", "image_03"])
    return dict(T_image0=T["image_00"], T_image1=T["image_01"], T_image2=T["image_02"], T_image3=T["image_03"])


def read_fisheycalib(file):
    """image_02.yaml / image_03.yaml: the first line is not YAML and is skipped (reference :45-49)"""
    import yaml
    with open(file, 'r') as f:
        f.readline()
        calib = yaml.safe_load(f)
    return calib


def extract_P_from_fisheye_calib(calib):
    """3x4 f64 P from the Mei projection parameters: gamma1, gamma2 on the diagonal, u0, v0 (reference :51-58)"""
    P = np.zeros([3, 4])
    P[0, 0] = calib["projection_parameters"]["gamma1"]
    P[1, 1] = calib["projection_parameters"]["gamma2"]
    P[0, 2] = calib["projection_parameters"]["u0"]
    P[1, 2] = calib["projection_parameters"]["v0"]
    P[2, 2] = 1
    return P


def read_split_file(file):
    """KITTI-style split "folder index side" (reference :74-93)"""
    imdb = []
    with open(file, 'r') as f:
        for line in f.readlines():
            line = line.strip().split()
            folder = line[0]
            imdb.append(dict(folder=folder, index=int(line[1]), side=line[2], datetime=folder.split("/")[0]))
    return imdb


class KITTI360FisheyeDataset(KITTI360TripletDataset):
    camera_dirs = ('image_02', 'image_03')
    image_subdir = 'data_rgb'

    def __init__(self, **data_cfg):
        super().__init__(**data_cfg)
        fish_eye_mask = data_cfg.get('fisheye_mask', None)
        self.fish_eye_mask = None if fish_eye_mask is None else np.array(_read_mask(fish_eye_mask))

    def _data_dirs(self, data_cfg):
        self.resized_root = getattr(data_cfg, 'resized_root', None)
        if self.resized_root is not None:
            return self.resized_root, os.path.join(self.resized_root, 'calibration')
        return super()._data_dirs(data_cfg)

    def _load_calib(self):
        left_calib = read_fisheycalib(os.path.join(self.calib_dir, "image_02.yaml"))
        right_calib = read_fisheycalib(os.path.join(self.calib_dir, "image_03.yaml"))
        T_image2pose_dict = read_extrinsic_from_sequence(os.path.join(self.calib_dir, "calib_cam_to_pose.txt"))
        self.cam_calib = dict(P0=extract_P_from_fisheye_calib(left_calib), P1=extract_P_from_fisheye_calib(right_calib),
                              T_rect02baselink=T_image2pose_dict['T_image2'],
                              T_rect12baselink=T_image2pose_dict['T_image3'],
                              left_meta=left_calib, right_meta=right_calib)

    def _sample(self, index):
        data, right = super()._sample(index)
        mask = data.pop("patched_mask")                 # calib_meta comes before it in the reference's sample
        data['calib_meta'] = deepcopy(self.cam_calib['right_meta' if right else 'left_meta'])
        if self.fish_eye_mask is not None:
            h, w = mask.shape
            mask = self.fish_eye_mask
            if mask.shape[:2] != (h, w):
                from fsnet_amd.monodepth.networks.utils.postopt_utils import resize_nearest
                mask = resize_nearest(mask, w, h)
            mask = np.asarray(mask, dtype=np.float64)
        data["patched_mask"] = mask
        return data, right


def _read_mask(path):
    """cv2.imread(path, -1) of an 8-bit single-channel PNG: uint8 [H, W]"""
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError("fisheye mask %s not found" % path)
    return np.array(Image.open(path, 'r'))
