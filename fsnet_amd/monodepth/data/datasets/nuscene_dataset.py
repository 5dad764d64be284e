"""The nuScenes datasets with the reference's module path, class names, constructor keys and sample contract
(monodepth/data/datasets/nuscene_dataset.py:14-238).

NusceneJsonDataset is the one the shipped configs use (nusc_wpose_example, distill_nusc_example, the nuScenes leg of
multi_dataset_example): a JSON file of samples with the frame paths, the 3x3 intrinsics, the two relative poses and the
camera of each.  NusceneDepthMonoDataset / NusceneSweepDepthMonoDataset read the nuScenes tables themselves, through
vision_base.data.datasets.nuscenes_utils.NuScenes (the devkit where it is installed, the JSON table reader otherwise).

A sample: raw uint8 frames under ('image', f) and ('original_image', f), ('relative_pose', f) float32 [4, 4], a float64
patched_mask of ones (CAM_BACK of the JSON dataset: rows 700 and below zeroed, the car's own body), P2 / original_P2
float32 [3, 4], camera_type_index, camera_type and ('filename', 0) — then the configured augmentation.  With the
mirrored augmentation classes the frames stay uint8 and the pixel work runs on the device (DeviceAugment); the string
entries travel through both collate functions as lists.

Random draws: the static filter of the table datasets redraws with np.random.randint(len(self)), as the reference."""
import json
import os
from copy import deepcopy
from functools import partial

import numpy as np
import torch.utils.data

from fsnet_amd.monodepth.data.datasets.utils import (cam_relative_pose_nusc, get_transformation_matrix, read_image,
                                                     read_vo_depth)
from fsnet_amd.vision_base.utils.builder import build
from fsnet_amd.vision_base.utils.utils import EasyDict

CAMERAS = ['CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_RIGHT', 'CAM_BACK', 'CAM_BACK_LEFT', 'CAM_FRONT_LEFT']


class NusceneDepthMonoDataset(torch.utils.data.Dataset):
    def __init__(self, **data_cfg):
        data_cfg = EasyDict(data_cfg)
        super(NusceneDepthMonoDataset, self).__init__()
        self.nuscenes_version = getattr(data_cfg, 'nuscenes_version', 'v1.0-trainval')
        self.nuscenes_dir = getattr(data_cfg, 'nuscenes_dir', '/data/nuscene')
        self.nusc_meta_file = data_cfg.split_file
        with open(self.nusc_meta_file, 'r') as f:
            self.token_list = [line.strip().split(',') for line in f.readlines()]
        self.nusc = build('fsnet_amd.vision_base.data.datasets.nuscenes_utils.NuScenes', version=self.nuscenes_version,
                          dataroot=self.nuscenes_dir, verbose=True)
        self.number_scenes = len(self.nusc.scene)
        print(f"Found {self.number_scenes} in the {self.nuscenes_version}")
        self.nusc_get_sample = partial(self.nusc.get, 'sample')
        self.nusc_get_sample_data = partial(self.nusc.get, 'sample_data')
        self.nusc_get_sensor = partial(self.nusc.get, 'calibrated_sensor')
        self.nusc_get_ego_pose = partial(self.nusc.get, 'ego_pose')
        self.cameras = getattr(data_cfg, 'channels', CAMERAS)
        self.vo_path = getattr(data_cfg, 'vo_path', None)
        self.is_read_vo_depth = self.vo_path is not None
        self.frame_ids = getattr(data_cfg, 'frame_ids', [0, -1, 1])
        self.is_motion_mask = getattr(data_cfg, 'is_motion_mask', False)
        if self.is_motion_mask:
            self.precompute_path = data_cfg.precompute_path
        self.is_filter_static = getattr(data_cfg, 'is_filter_static', True)
        self.filter_threshold = getattr(data_cfg, 'filter_threshold', 0.03)
        self.transform = build(**data_cfg.augmentation)

    def __len__(self):
        return len(self.token_list) * len(self.cameras)

    def get_intrinsic(self, cs_record):
        return np.array(cs_record['camera_intrinsic'])

    def get_extrinsic(self, cs_record):
        return get_transformation_matrix(cs_record['translation'], cs_record['rotation'])

    def get_ego_pose(self, ego_record):
        return get_transformation_matrix(ego_record['translation'], ego_record['rotation'])

    def _camera_datas(self, token_index, camera_type):
        """the sample_data records of the frames, centre first: key frames of the tokens on the split's line"""
        samples = list(map(self.nusc_get_sample, self.token_list[token_index]))
        return list(map(self.nusc_get_sample_data, [sample['data'][camera_type] for sample in samples]))

    def _frames(self, index):
        """what the two table datasets share (reference :61-91 and :118-165): the records, the relative poses with the
        static filter, the frames.  Returns None when the filter asks for a redraw."""
        token_index = index // len(self.cameras)
        camera_type_index = index % len(self.cameras)
        camera_type = self.cameras[camera_type_index]
        camera_datas = self._camera_datas(token_index, camera_type)
        cs_records = list(map(self.nusc_get_sensor, [cd['calibrated_sensor_token'] for cd in camera_datas]))
        ego_records = list(map(self.nusc_get_ego_pose, [cd['ego_pose_token'] for cd in camera_datas]))
        image_arrays = list(map(read_image, [os.path.join(self.nuscenes_dir, cd['filename']) for cd in camera_datas]))
        P2 = self.get_intrinsic(cs_records[0])
        extrinsics = list(map(self.get_extrinsic, cs_records))
        poses = list(map(self.get_ego_pose, ego_records))
        data = dict()
        for i, idx in enumerate(self.frame_ids[1:]):
            data[('relative_pose', idx)] = cam_relative_pose_nusc(
                poses[0], poses[i + 1], np.linalg.inv(extrinsics[0])).astype(np.float32)
            if self.is_filter_static:
                translation = np.linalg.norm(data[('relative_pose', idx)][0:3, 3])
                if translation < self.filter_threshold or translation > 3:
                    return None
        for i, frame_id in enumerate(self.frame_ids):
            data[('image', frame_id)] = image_arrays[i]
            data[('original_image', frame_id)] = data[('image', frame_id)].copy()
        return data, camera_datas, P2, camera_type_index, camera_type

    @staticmethod
    def _finish(data, P2, camera_type_index):
        h, w, _ = data[("image", 0)].shape
        data["patched_mask"] = np.ones([h, w])
        data['P2'] = np.zeros((3, 4), dtype=np.float32)
        data['P2'][0:3, 0:3] = P2
        data['original_P2'] = data['P2'].copy()
        data['camera_type_index'] = camera_type_index

    def _read_vo(self, data, filename, index):
        vo_path = filename.replace('samples', self.vo_path).replace('.jpg', '.png')
        if os.path.isfile(vo_path):
            data[('vo_depth', 0)] = read_vo_depth(vo_path)
        else:
            print(f'No VO Depth file found at {index}, {vo_path}')

    def __getitem__(self, index):
        got = self._frames(index)
        if got is None:
            return self[np.random.randint(len(self))]
        data, camera_datas, P2, camera_type_index, camera_type = got
        if self.is_read_vo_depth:
            self._read_vo(data, camera_datas[0]['filename'], index)
        self._finish(data, P2, camera_type_index)
        data[('filename', 0)] = camera_datas[0]['filename']
        data['camera_type'] = camera_type
        return self.transform(deepcopy(data))


class NusceneSweepDepthMonoDataset(NusceneDepthMonoDataset):
    """Use Sweep around key frames: the neighbours are |frame_id| steps along sample_data's next / prev chain"""

    def _camera_datas(self, token_index, camera_type):
        main_sample = self.nusc_get_sample(self.token_list[token_index][0])
        main_camera_instance = self.nusc_get_sample_data(main_sample['data'][camera_type])
        camera_datas = [main_camera_instance]
        for frame_id in self.frame_ids[1:]:
            next_key = 'next' if frame_id > 0 else 'prev'
            tmp_camera_instance = main_camera_instance
            for _ in range(abs(frame_id)):
                tmp_camera_instance = self.nusc_get_sample_data(tmp_camera_instance[next_key])
            camera_datas.append(tmp_camera_instance)
        return camera_datas

    def __getitem__(self, index):
        got = self._frames(index)
        if got is None:
            return self[np.random.randint(len(self))]
        data, _, P2, camera_type_index, _ = got
        self._finish(data, P2, camera_type_index)
        return self.transform(deepcopy(data))


class NusceneJsonDataset(torch.utils.data.Dataset):
    def __init__(self, **data_cfg):
        data_cfg = EasyDict(data_cfg)
        super(NusceneJsonDataset, self).__init__()
        self.json_path = getattr(data_cfg, 'json_path',
                                 '/home/monodepth/meta_data/nusc_trainsub/json_nusc_front_train.json')
        with open(self.json_path, 'r') as f:
            self.json_dict = json.load(f)
        self.image_keys = getattr(data_cfg, 'image_keys', ['frame0', 'frame1', 'frame-1'])
        self.pose_keys = getattr(data_cfg, 'pose_keys', ['pose01', 'pose0-1'])
        self.intrinsic_key = getattr(data_cfg, 'intrinsic_key', 'P2')
        self.cameras = getattr(data_cfg, 'channels', CAMERAS)
        self.frame_ids = getattr(data_cfg, 'frame_ids', [0, 1, -1])
        self.transform = build(**data_cfg.augmentation)
        self.vo_path = getattr(data_cfg, 'vo_path', None)
        self.is_read_vo_depth = self.vo_path is not None

    def __len__(self):
        return len(self.json_dict['samples'])

    BACK_MASK_FROM_ROW = 700          # CAM_BACK sees the car's own body below this row of a 900-row frame

    def __getitem__(self, index):
        """one entry of the JSON list as a sample, keys in the reference's order (:198-238)"""
        entry = self.json_dict['samples'][index]
        frames = [read_image(entry[key]) for key in self.image_keys]
        camera_type = entry['camera_type']
        data = {('relative_pose', f): np.array(entry[key]).reshape([4, 4]).astype(np.float32)
                for f, key in ((1, 'pose01'), (-1, 'pose0-1'))}
        for frame_id, frame in zip(self.frame_ids, frames):
            data[('image', frame_id)] = frame
            data[('original_image', frame_id)] = frame.copy()
        NusceneDepthMonoDataset._finish(data, np.array(entry[self.intrinsic_key]).reshape(3, 3).astype(np.float32),
                                        entry['camera_type_indexes'])
        if camera_type == 'CAM_BACK':
            data['patched_mask'][self.BACK_MASK_FROM_ROW:, :] = 0
        data[('filename', 0)] = os.path.join(*entry[self.image_keys[0]].split('/')[-3:])
        data['camera_type'] = camera_type
        if self.is_read_vo_depth:
            NusceneDepthMonoDataset._read_vo(self, data, data[('filename', 0)], index)
        return self.transform(deepcopy(data))
