"""KITTI-360 perspective triplet dataset with the reference's module path, function and class names, constructor keys
and sample contract (monodepth/data/datasets/kitti360_dataset.py:1-220): the comma-separated split "sequence, pose
index, image index, former, latter" of the fisheye reader, the rectified pinhole cameras image_00 / image_01
(calibration/perspective.txt: P_rect_0k and R_rect_0k), camera-to-pose extrinsics composed with the rectifying rotation
(T_rect0k -> baselink = R_rect_0k @ T_image_0k), data_poses -> ('relative_pose', f), raw uint8 frames of
image_0k/data_rect under ('image', f) and ('original_image', f), P2 / original_P2 from the first three columns of
P_rect_0k and a patched_mask of ones — then the configured augmentation.  With the mirrored augmentation classes the frames stay uint8 and the pixel
work runs on the device (DeviceAugment), as for the two datasets mirrored before.

Random draws: one np.random.rand() per __getitem__ when use_right_image is true (left camera below 0.5), in the
reference's order, before the augmentation's own draws."""
import os
from copy import deepcopy

import numpy as np
import torch.utils.data

from fsnet_amd.monodepth.data.datasets.fisheye_dataset import read_poses_file  # noqa: F401  (same file, same reader)
from fsnet_amd.monodepth.data.datasets.utils import cam_relative_pose_nusc, read_image
from fsnet_amd.vision_base.utils.builder import build
from fsnet_amd.vision_base.utils.utils import EasyDict


def read_P01_from_sequence(file):
    """perspective.txt -> (P0 [3, 4], P1 [3, 4], R0 [4, 4], R1 [4, 4]): P_rect_00 / P_rect_01 and the rectifying
    rotations R_rect_00 / R_rect_01 in the upper-left block of an identity (reference :13-40)"""
    P = {"P_rect_00": None, "P_rect_01": None}
    R = {"R_rect_00": np.eye(4), "R_rect_01": np.eye(4)}
    with open(file, 'r') as f:
        for line in f.readlines():
            data = line.strip().split(" ")
            for k in P:
                if line.startswith(k):
                    P[k] = np.reshape(np.array([float(x) for x in data[1:13]]), [3, 4])
            for k in R:
                if line.startswith(k):
                    R[k][0:3, 0:3] = np.reshape(np.array([float(x) for x in data[1:10]]), [3, 3])
    for k, v in P.items():
        assert v is not None, "can not find {} in file {}".format(k, file)
    return P["P_rect_00"], P["P_rect_01"], R["R_rect_00"], R["R_rect_01"]


def read_extrinsic_from_sequence(file):
    """calib_cam_to_pose.txt -> (T0, T1): 4x4 camera-to-pose of image_00 and image_01, identity when the file does not
    list the camera (reference :42-58; the fisheye module's reader of the same name returns a dict of all four)"""
    T = {"image_00": np.eye(4), "image_01": np.eye(4)}
    with open(file, 'r') as f:
        for line in f.readlines():
            for k in T:
                if line.startswith(k):
                    data = line.strip().split(" ")
                    T[k][0:3, :] = np.reshape(np.array([float(x) for x in data[1:13]]), [3, 4])
    return T["image_00"], T["image_01"]


def read_T_from_sequence(file):
    """calib_cam_to_velo.txt: 12 numbers on the first line -> 4x4 camera 00 -> velodyne (reference :73-83)"""
    with open(file, 'r') as f:
        data = f.readlines()[0].strip().split(" ")
    T = np.eye(4)
    T[0:3, :] = np.array([float(x) for x in data[0:12]]).reshape([3, 4])
    return T


class KITTI360MonoDataset(torch.utils.data.Dataset):
    def __init__(self, **data_cfg):
        data_cfg = EasyDict(data_cfg)
        super().__init__()
        self.raw_path = getattr(data_cfg, 'raw_path', '/data/KITTI-360')
        self.meta_file = getattr(data_cfg, 'split_file', 'kitti360_meta.txt')
        self.img_dir = os.path.join(self.raw_path, 'data_2d_raw')
        self.pose_dir = os.path.join(self.raw_path, 'data_poses')
        self.calib_dir = os.path.join(self.raw_path, 'calibration')
        self.pc_dir = os.path.join(self.raw_path, 'data_3d_raw')

        self.frame_ids = list(getattr(data_cfg, 'frame_ids', [0, -1, 1]))
        self.imdb = []
        self.sequence_names = set()
        with open(self.meta_file, 'r') as f:
            for line in f.readlines():
                sequence_name, pose_index, img_index, former_index, latter_index = line.strip().split(',')
                pose_index, img_index = int(pose_index), int(img_index)
                index_dict = {0: img_index, -1: int(former_index), 1: int(latter_index)}
                self.sequence_names.add(sequence_name)
                self.imdb.append(dict(sequence_name=sequence_name,
                                      pose_indexes=[pose_index + ind for ind in self.frame_ids],
                                      img_indexes=[index_dict[ind] for ind in self.frame_ids]))
        self._load_calib()
        self._load_keypose()

        self.is_motion_mask = getattr(data_cfg, 'is_motion_mask', False)      # accepted, unused (as in the reference)
        if self.is_motion_mask:
            self.precompute_path = getattr(data_cfg, 'motion_mask_path', "")

        self.is_filter_static = getattr(data_cfg, 'is_filter_static', True)
        self.filter_threshold = getattr(data_cfg, 'filter_threshold', 0.03)
        if self.is_filter_static:
            self.imdb = self._filter_indexes()

        self.use_right_image = getattr(data_cfg, 'use_right_image', True)
        self.transform = build(**data_cfg.augmentation)

    def _relative_pose(self, poses, i, extrinsics):
        return cam_relative_pose_nusc(poses[0], poses[i + 1], np.linalg.inv(extrinsics)).astype(np.float32)

    def _filter_indexes(self):
        """drop samples that moved less than filter_threshold or more than 3 m to a neighbour frame (reference
        :136-157; always measured with the left camera's extrinsics)"""
        imdb = []
        print(f"Start Filtering indexes, original length {len(self)}")
        extrinsics = self.cam_calib['T_rect02baselink']
        for obj in self.imdb:
            poses = self.keypose[obj['sequence_name']][obj['pose_indexes']]
            is_overlook = False
            for i, _ in enumerate(self.frame_ids[1:]):
                translation = np.linalg.norm(self._relative_pose(poses, i, extrinsics)[0:3, 3])
                if translation < self.filter_threshold or translation > 3:
                    is_overlook = True
            if not is_overlook:
                imdb.append(obj)
        print(f"Finished filtering indexes, find dynamic instances {len(imdb)}")
        return imdb

    def _load_calib(self):
        P0, P1, R0, R1 = read_P01_from_sequence(os.path.join(self.calib_dir, "perspective.txt"))
        T0, T1 = read_extrinsic_from_sequence(os.path.join(self.calib_dir, "calib_cam_to_pose.txt"))
        self.cam_calib = dict(P0=P0, P1=P1, T_rect02baselink=R0 @ T0, T_rect12baselink=R1 @ T1)

    def _load_keypose(self):
        self.keypose = {}
        for sequence_name in self.sequence_names:
            _, poses = read_poses_file(os.path.join(self.pose_dir, sequence_name, 'poses.txt'))
            self.keypose[sequence_name] = poses

    def __len__(self):
        return len(self.imdb)

    def __getitem__(self, index):
        obj = self.imdb[index]
        sequence_name, pose_indexes, img_indexes = obj['sequence_name'], obj['pose_indexes'], obj['img_indexes']
        if (not self.use_right_image) or (np.random.rand() < 0.5):
            extrinsics, image_dir_name, P2 = self.cam_calib['T_rect02baselink'], 'image_00', self.cam_calib['P0']
        else:
            extrinsics, image_dir_name, P2 = self.cam_calib['T_rect12baselink'], 'image_01', self.cam_calib['P1']

        data = dict()
        poses = self.keypose[sequence_name][pose_indexes]
        for i, idx in enumerate(self.frame_ids[1:]):
            data[('relative_pose', idx)] = self._relative_pose(poses, i, extrinsics)
        image_dir = os.path.join(self.img_dir, sequence_name, image_dir_name, 'data_rect')
        for frame_id, i in zip(self.frame_ids, img_indexes):
            data[('image', frame_id)] = read_image(os.path.join(image_dir, f"{i:010d}.png"))
            data[('original_image', frame_id)] = data[('image', frame_id)].copy()

        data['P2'] = np.zeros((3, 4), dtype=np.float32)
        data['P2'][0:3, 0:3] = P2[0:3, 0:3]
        data['original_P2'] = data['P2'].copy()

        h, w, _ = data[("image", 0)].shape
        data["patched_mask"] = np.ones([h, w])
        return self.transform(deepcopy(data))
