"""KITTI-360 fisheye triplet dataset with the reference's module path, class name, constructor keys and sample contract
(monodepth/data/datasets/fisheye_dataset.py:1-262): comma-separated split "sequence, pose index, image index, former,
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
import torch.utils.data

from fsnet_amd.monodepth.data.datasets.utils import cam_relative_pose_nusc, read_image
from fsnet_amd.vision_base.utils.builder import build
from fsnet_amd.vision_base.utils.utils import EasyDict


def _read_camera_lines(file, keys):
    out = {k: np.eye(4) for k in keys}
    with open(file, 'r') as f:
        for line in f.readlines():
            for k in keys:
                if line.startswith(k):
                    data = line.strip().split(" ")
                    out[k][0:3, :] = np.reshape(np.array([float(x) for x in data[1:13]]), [3, 4])
    return out


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


def read_poses_file(file):
    """data_poses/<seq>/poses.txt: "frame r00 ... t2" per line -> (key frames, f64 [N, 4, 4]) (reference :60-71)"""
    key_frames, poses = [], []
    with open(file, 'r') as f:
        for line in f.readlines():
            data = line.strip().split(" ")
            key_frames.append(int(data[0]))
            pose = np.eye(4)
            pose[0:3, :] = np.array([float(x) for x in data[1:13]]).reshape([3, 4])
            poses.append(pose)
    return key_frames, np.array(poses)


def read_split_file(file):
    """KITTI-style split "folder index side" (reference :74-93)"""
    imdb = []
    with open(file, 'r') as f:
        for line in f.readlines():
            line = line.strip().split()
            folder = line[0]
            imdb.append(dict(folder=folder, index=int(line[1]), side=line[2], datetime=folder.split("/")[0]))
    return imdb


def read_cam2velo_from_sequence(file):
    """calib_cam_to_velo.txt: 12 numbers on the first line -> 4x4 (reference :95-105)"""
    with open(file, 'r') as f:
        line = f.readlines()[0]
        data = line.strip().split(" ")
        T = np.array([float(x) for x in data[0:12]]).reshape([3, 4])
    T_cam2velo = np.eye(4)
    T_cam2velo[0:3, :] = T
    return T_cam2velo


class KITTI360FisheyeDataset(torch.utils.data.Dataset):
    def __init__(self, **data_cfg):
        data_cfg = EasyDict(data_cfg)
        super().__init__()
        self.raw_path = getattr(data_cfg, 'raw_path', '/data/KITTI-360')
        self.meta_file = getattr(data_cfg, 'split_file', 'kitti360_meta.txt')
        self.resized_root = getattr(data_cfg, 'resized_root', None)
        if self.resized_root is not None:
            self.img_dir = self.resized_root
            self.calib_dir = os.path.join(self.resized_root, 'calibration')
        else:
            self.img_dir = os.path.join(self.raw_path, 'data_2d_raw')
            self.calib_dir = os.path.join(self.raw_path, 'calibration')
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

        fish_eye_mask = getattr(data_cfg, 'fisheye_mask', None)
        self.fish_eye_mask = None if fish_eye_mask is None else np.array(_read_mask(fish_eye_mask))
        self.transform = build(**data_cfg.augmentation)

    def _relative_pose(self, poses, i, extrinsics):
        return cam_relative_pose_nusc(poses[0], poses[i + 1], np.linalg.inv(extrinsics)).astype(np.float32)

    def _filter_indexes(self):
        """drop samples that moved less than filter_threshold or more than 3 m to a neighbour frame (reference
        :169-190; always measured with the left camera's extrinsics)"""
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
        left_calib = read_fisheycalib(os.path.join(self.calib_dir, "image_02.yaml"))
        right_calib = read_fisheycalib(os.path.join(self.calib_dir, "image_03.yaml"))
        T_image2pose_dict = read_extrinsic_from_sequence(os.path.join(self.calib_dir, "calib_cam_to_pose.txt"))
        self.cam_calib = dict(P0=extract_P_from_fisheye_calib(left_calib), P1=extract_P_from_fisheye_calib(right_calib),
                              T_rect02baselink=T_image2pose_dict['T_image2'],
                              T_rect12baselink=T_image2pose_dict['T_image3'],
                              left_meta=left_calib, right_meta=right_calib)

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
            extrinsics, image_dir_name = self.cam_calib['T_rect02baselink'], 'image_02'
            P2, calib_meta = self.cam_calib['P0'], self.cam_calib['left_meta']
        else:
            extrinsics, image_dir_name = self.cam_calib['T_rect12baselink'], 'image_03'
            P2, calib_meta = self.cam_calib['P1'], self.cam_calib['right_meta']

        data = dict()
        poses = self.keypose[sequence_name][pose_indexes]
        for i, idx in enumerate(self.frame_ids[1:]):
            data[('relative_pose', idx)] = self._relative_pose(poses, i, extrinsics)
        image_dir = os.path.join(self.img_dir, sequence_name, image_dir_name, 'data_rgb')
        for frame_id, i in zip(self.frame_ids, img_indexes):
            data[('image', frame_id)] = read_image(os.path.join(image_dir, f"{i:010d}.png"))

        data['P2'] = np.zeros((3, 4), dtype=np.float32)
        data['P2'][0:3, 0:3] = P2[0:3, 0:3]
        data['original_P2'] = data['P2'].copy()
        data['calib_meta'] = deepcopy(calib_meta)

        h, w, _ = data[("image", 0)].shape
        if self.fish_eye_mask is not None:
            m = self.fish_eye_mask
            if m.shape[:2] != (h, w):
                from fsnet_amd.monodepth.networks.utils.postopt_utils import resize_nearest
                m = resize_nearest(m, w, h)
            data["patched_mask"] = np.asarray(m, dtype=np.float64)
        else:
            data["patched_mask"] = np.ones([h, w])
        return self.transform(deepcopy(data))


def _read_mask(path):
    """cv2.imread(path, -1) of an 8-bit single-channel PNG: uint8 [H, W]"""
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError("fisheye mask %s not found" % path)
    return np.array(Image.open(path, 'r'))
