"""What the two KITTI-360 triplet datasets share (the reference repeats it in monodepth/data/datasets/
fisheye_dataset.py and kitti360_dataset.py): the readers of calib_cam_to_pose.txt, calib_cam_to_velo.txt and
data_poses, the comma-separated split "sequence, pose index, image index, former, latter" -> image / pose index
triplets, the static-frame filter, the left / right camera draw and the sample up to P2 / original_P2 and a
patched_mask of ones.  KITTI360FisheyeDataset and KITTI360MonoDataset add their calibration, camera folders and extras.

Random draws: one np.random.rand() per sample when use_right_image is true (left camera below 0.5), in the
reference's order, before the augmentation's own draws."""
import os
from copy import deepcopy

import numpy as np
import torch.utils.data

from fsnet_amd.monodepth.data.datasets.utils import cam_relative_pose_nusc, read_image
from fsnet_amd.vision_base.utils.builder import build
from fsnet_amd.vision_base.utils.utils import EasyDict


def _read_camera_lines(file, keys):
    """calib_cam_to_pose.txt: lines "image_0k: r00 ... t2" -> {key: 4x4 camera-to-pose}, identity for a camera the file
    does not list"""
    out = {k: np.eye(4) for k in keys}
    with open(file, 'r') as f:
        for line in f.readlines():
            for k in keys:
                if line.startswith(k):
                    data = line.strip().split(" ")
                    out[k][0:3, :] = np.reshape(np.array([float(x) for x in data[1:13]]), [3, 4])
    return out


def read_poses_file(file):
    """data_poses/<seq>/poses.txt: "frame r00 ... t2" per line -> (key frames, f64 [N, 4, 4]) (reference
    fisheye_dataset.py:60-71)"""
    key_frames, poses = [], []
    with open(file, 'r') as f:
        for line in f.readlines():
            data = line.strip().split(" ")
            key_frames.append(int(data[0]))
            pose = np.eye(4)
            pose[0:3, :] = np.array([float(x) for x in data[1:13]]).reshape([3, 4])
            poses.append(pose)
    return key_frames, np.array(poses)


def read_cam2velo_from_sequence(file):
    """calib_cam_to_velo.txt: 12 numbers on the first line -> 4x4 camera 00 -> velodyne (reference
    fisheye_dataset.py:95-105, kitti360_dataset.py:73-83)"""
    with open(file, 'r') as f:
        data = f.readlines()[0].strip().split(" ")
    T = np.eye(4)
    T[0:3, :] = np.array([float(x) for x in data[0:12]]).reshape([3, 4])
    return T


class KITTI360TripletDataset(torch.utils.data.Dataset):
    """A subclass names its camera folders and supplies `_load_calib`, which fills `cam_calib` with P0 / P1 and
    T_rect02baselink / T_rect12baselink of the left / right camera."""
    camera_dirs = None          # (left, right) folder of a sequence
    image_subdir = None         # the frames' folder inside a camera folder
    keep_original_image = False  # also hand the raw frames on under ('original_image', f)

    def __init__(self, **data_cfg):
        data_cfg = EasyDict(data_cfg)
        super().__init__()
        self.raw_path = getattr(data_cfg, 'raw_path', '/data/KITTI-360')
        self.meta_file = getattr(data_cfg, 'split_file', 'kitti360_meta.txt')
        self.img_dir, self.calib_dir = self._data_dirs(data_cfg)
        self.pose_dir = os.path.join(self.raw_path, 'data_poses')
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

    def _data_dirs(self, data_cfg):
        """(root of the frames, calibration folder)"""
        return os.path.join(self.raw_path, 'data_2d_raw'), os.path.join(self.raw_path, 'calibration')

    def _relative_pose(self, poses, i, extrinsics):
        return cam_relative_pose_nusc(poses[0], poses[i + 1], np.linalg.inv(extrinsics)).astype(np.float32)

    def _filter_indexes(self):
        """drop samples that moved less than filter_threshold or more than 3 m to a neighbour frame (reference
        fisheye_dataset.py:169-190, kitti360_dataset.py:136-157; always measured with the left camera's extrinsics)"""
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

    def _load_keypose(self):
        self.keypose = {}
        for sequence_name in self.sequence_names:
            _, poses = read_poses_file(os.path.join(self.pose_dir, sequence_name, 'poses.txt'))
            self.keypose[sequence_name] = poses

    def __len__(self):
        return len(self.imdb)

    def _sample(self, index):
        """(the sample before the augmentation, 0 / 1 for the left / right camera it was drawn from)"""
        obj = self.imdb[index]
        sequence_name, pose_indexes, img_indexes = obj['sequence_name'], obj['pose_indexes'], obj['img_indexes']
        right = int(bool(self.use_right_image) and not np.random.rand() < 0.5)
        extrinsics, P2 = self.cam_calib['T_rect%d2baselink' % right], self.cam_calib['P%d' % right]

        data = dict()
        poses = self.keypose[sequence_name][pose_indexes]
        for i, idx in enumerate(self.frame_ids[1:]):
            data[('relative_pose', idx)] = self._relative_pose(poses, i, extrinsics)
        image_dir = os.path.join(self.img_dir, sequence_name, self.camera_dirs[right], self.image_subdir)
        for frame_id, i in zip(self.frame_ids, img_indexes):
            data[('image', frame_id)] = read_image(os.path.join(image_dir, f"{i:010d}.png"))
            if self.keep_original_image:
                data[('original_image', frame_id)] = data[('image', frame_id)].copy()

        data['P2'] = np.zeros((3, 4), dtype=np.float32)
        data['P2'][0:3, 0:3] = P2[0:3, 0:3]
        data['original_P2'] = data['P2'].copy()

        h, w, _ = data[("image", 0)].shape
        data["patched_mask"] = np.ones([h, w])
        return data, right

    def __getitem__(self, index):
        return self.transform(deepcopy(self._sample(index)[0]))
