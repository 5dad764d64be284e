"""KITTI-360 perspective triplet dataset with the reference's module path, function and class names, constructor keys
and sample contract (monodepth/data/datasets/kitti360_dataset.py:1-220), on the base it shares with the fisheye dataset
(kitti360_triplet.KITTI360TripletDataset): the comma-separated split "sequence, pose index, image index, former,
latter" of the fisheye reader, the rectified pinhole cameras image_00 / image_01
(calibration/perspective.txt: P_rect_0k and R_rect_0k), camera-to-pose extrinsics composed with the rectifying rotation
(T_rect0k -> baselink = R_rect_0k @ T_image_0k), data_poses -> ('relative_pose', f), raw uint8 frames of
image_0k/data_rect under ('image', f) and ('original_image', f), P2 / original_P2 from the first three columns of
P_rect_0k and a patched_mask of ones — then the configured augmentation.  With the mirrored augmentation classes the frames stay uint8 and the pixel
work runs on the device (DeviceAugment), as for the two datasets mirrored before.

Random draws: one np.random.rand() per __getitem__ when use_right_image is true (left camera below 0.5), in the
reference's order, before the augmentation's own draws."""
import os

import numpy as np

from fsnet_amd.monodepth.data.datasets.kitti360_triplet import (  # noqa: F401  (the readers keep their names here)
    KITTI360TripletDataset, _read_camera_lines, read_cam2velo_from_sequence, read_poses_file)


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
    T = _read_camera_lines(file, ["image_00", "image_01"])
    return T["image_00"], T["image_01"]


read_T_from_sequence = read_cam2velo_from_sequence      # calib_cam_to_velo.txt -> 4x4 (reference :73-83)


class KITTI360MonoDataset(KITTI360TripletDataset):
    camera_dirs = ('image_00', 'image_01')
    image_subdir = 'data_rect'
    keep_original_image = True

    def _load_calib(self):
        P0, P1, R0, R1 = read_P01_from_sequence(os.path.join(self.calib_dir, "perspective.txt"))
        T0, T1 = read_extrinsic_from_sequence(os.path.join(self.calib_dir, "calib_cam_to_pose.txt"))
        self.cam_calib = dict(P0=P0, P1=P1, T_rect02baselink=R0 @ T0, T_rect12baselink=R1 @ T1)
