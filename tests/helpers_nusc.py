"""A tiny seeded nuScenes tree: the JSON tables the evaluator's export and the table datasets read (scene, sample,
sample_data, ego_pose, calibrated_sensor, sensor), one LiDAR sweep and six H x W camera frames per sample, the split
file and the JSON sample lists of NusceneJsonDataset — shared by tools/gen_golden.py::gen_nusc (which runs the REAL
reference classes over it) and the tests.

NS samples in one scene; the split's lines are "centre,previous,next" for the EVAL samples, so the evaluator (first
token of a line) and NusceneDepthMonoDataset (all three) read the same file.  The frames are PNG data under the
layout's .jpg names (PIL goes by content; a JPEG would decode differently from one libjpeg to the next).

CAM_FRONT is an exact camera: its rotation is the axis permutation of the real rig (quaternion 0.5, -0.5, 0.5, -0.5),
its translation, the LiDAR's and the intrinsics are dyadic, so the hand-placed points below project without any
rounding and the result does not depend on the order or fusion of the reference's matrix products: exact .5 pixel
ties (to even and to odd), duplicates whose minimum is neither first nor last, pairs on (r, W-1) / (r+1, 0), depths on
exact multiples of 1/256.  The other five cameras are ordinary rotations; a ring of random points around the car
covers all six, with points behind every camera."""
import json
import os

import numpy as np

VERSION = 'v1.0-mini'
CAMS = ['CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_RIGHT', 'CAM_BACK', 'CAM_BACK_LEFT', 'CAM_FRONT_LEFT']
H, W = 24, 40
NS = 4                         # samples in the scene
EVAL = [1, 2]                  # the samples of the split (each with its neighbours)
NPTS = 6000
SEED = 23
LIDAR_T = [1.0, 0.0, 1.75]
FRONT_T = [1.5, 0.0, 1.5]
FRONT_K = [[32.0, 0.0, 20.0], [0.0, 32.0, 12.0], [0.0, 0.0, 1.0]]
TALL_H, TALL_W = 704, 4        # one CAM_BACK frame tall enough for the rows 700+ of the patched mask


def _quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return [float(np.cos(angle / 2))] + [float(v) for v in np.sin(angle / 2) * axis]


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]


def cameras():
    """channel -> (translation, quaternion wxyz, intrinsic 3x3): CAM_FRONT exact, the rest yawed copies with a small
    pitch / roll and their own focal lengths"""
    base = [0.5, -0.5, 0.5, -0.5]
    yaws = dict(CAM_FRONT_RIGHT=-55.0, CAM_BACK_RIGHT=-110.0, CAM_BACK=180.0, CAM_BACK_LEFT=110.0, CAM_FRONT_LEFT=55.0)
    out = {'CAM_FRONT': (FRONT_T, base, FRONT_K)}
    for k, (cam, yaw) in enumerate(yaws.items()):
        q = _qmul(_quat([0, 0, 1], np.deg2rad(yaw + 0.3 * k)), _qmul(_quat([0, 1, 0], 0.004 * (k + 1)), base))
        t = [float(1.2 * np.cos(np.deg2rad(yaw))), float(0.5 * np.sin(np.deg2rad(yaw))), 1.5 + 0.01 * k]
        f = 31.0 + 0.37 * k
        out[cam] = (t, [float(v) for v in q], [[f, 0.0, 20.3 - 0.1 * k], [0.0, f + 0.2, 11.8 + 0.1 * k], [0.0, 0.0, 1.0]])
    return out


def _front_point(col, row, z):
    """ego-frame point that CAM_FRONT puts at u = col + 1 (before the - 1), v = row + 1, depth z; exact for dyadic input"""
    xc = (col + 1 - FRONT_K[0][2]) * z / FRONT_K[0][0]
    yc = (row + 1 - FRONT_K[1][2]) * z / FRONT_K[1][1]
    return [z + FRONT_T[0], -xc + FRONT_T[1], -yc + FRONT_T[2]]          # camera z = ego x, x = -ego y, y = -ego z


def special_points():
    """hand-placed ego-frame points of CAM_FRONT, in scan order"""
    P = []
    for col, z in ((4.5, 8.0), (5.5, 8.0), (4.5, 16.0), (7.5, 4.0)):       # u = k + .5: ties to even and to odd
        P.append(_front_point(col, 3, z))
    for row, z in ((6.5, 8.0), (7.5, 8.0), (6.5, 16.0)):                   # v ties
        P.append(_front_point(10, row, z))
    for z in (12.0, 9.0 + 3.0 / 256, 30.0, 9.5, 20.0):                     # five on one pixel: min third, last not min
        P.append(_front_point(12, 9, z))
    for z in (7.0, 7.0):                                                   # two equal
        P.append(_front_point(13, 9, z))
    for z in (5.0 + 1.0 / 256, 5.0):                                       # min last
        P.append(_front_point(14, 9, z))
    P.append(_front_point(W - 1, 14, 11.0))                                # edge pair: first on (14, W-1), min on (15, 0)
    P.append(_front_point(0, 15, 6.0))
    P.append(_front_point(0, 17, 6.5))                                     # edge pair: first on (17, 0), min on (16, W-1)
    P.append(_front_point(W - 1, 16, 4.0))
    P.append(_front_point(W - 1, 16, 25.0))
    P.append(_front_point(W - 1, H - 1, 13.0))                             # last pixel: no partner below
    P.append(_front_point(0, 0, 14.0))                                     # first pixel: no partner above
    P.append(_front_point(W, 5, 9.0))                                      # one column out of range
    P.append(_front_point(20, 20, 100.0 + 1.0 / 256))                      # beyond the 80 m of the metric
    return np.array(P, np.float64)


def sweep(rng, n=NPTS):
    """float32 [n + specials, 5] in the LiDAR frame (identity rotation: ego minus LIDAR_T)"""
    ang = rng.uniform(0, 2 * np.pi, n)
    dist = np.exp(rng.uniform(np.log(2.5), np.log(90.0), n))
    ego = np.stack([dist * np.cos(ang), dist * np.sin(ang), rng.uniform(-1.0, 4.0, n) + 0.02 * dist], 1)
    close = rng.uniform(-2.0, 2.0, (40, 3)) + np.array(LIDAR_T)             # inside remove_close's 2.2 m box
    sp = special_points()
    ego = np.concatenate([ego[:n // 2], sp[:len(sp) // 2], close, ego[n // 2:], sp[len(sp) // 2:]])
    pts = np.zeros((len(ego), 5), np.float32)
    pts[:, :3] = (ego - np.array(LIDAR_T)).astype(np.float32)
    pts[:, 3] = rng.uniform(0, 255, len(ego)).astype(np.float32)
    return pts


def ego_pose(i):
    """(translation, quaternion) of sample i: a car driving 1.1 m per sample on a gentle curve"""
    yaw = 0.4 + 0.015 * i
    q = _qmul(_quat([0, 0, 1], yaw), _quat([0, 1, 0], 0.002 * i))
    return [400.0 + 1.1 * i * float(np.cos(yaw)), 1100.0 + 1.1 * i * float(np.sin(yaw)), 0.0], [float(v) for v in q]


def make_tree(root, seed=SEED):
    """-> dict(dataroot, split, json_val, json_train, json_tall)"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    dataroot = os.path.join(root, 'nuscenes')
    tables = os.path.join(dataroot, VERSION)
    os.makedirs(tables, exist_ok=True)
    cams = cameras()
    sensor = [dict(token='sensor_' + c, channel=c, modality='camera') for c in CAMS]
    sensor.append(dict(token='sensor_LIDAR_TOP', channel='LIDAR_TOP', modality='lidar'))
    calibrated = [dict(token='cs_' + c, sensor_token='sensor_' + c, translation=cams[c][0], rotation=cams[c][1],
                       camera_intrinsic=cams[c][2]) for c in CAMS]
    calibrated.append(dict(token='cs_LIDAR_TOP', sensor_token='sensor_LIDAR_TOP', translation=LIDAR_T,
                           rotation=[1.0, 0.0, 0.0, 0.0], camera_intrinsic=[]))
    samples, sample_data, poses = [], [], []
    for i in range(NS):
        stamp = 1532402927000000 + 500000 * i
        samples.append(dict(token='sample_%d' % i, timestamp=stamp, scene_token='scene_0',
                            prev='sample_%d' % (i - 1) if i else '', next='sample_%d' % (i + 1) if i + 1 < NS else ''))
        t, q = ego_pose(i)
        poses.append(dict(token='pose_%d' % i, timestamp=stamp, translation=t, rotation=q))
        for c in CAMS + ['LIDAR_TOP']:
            lidar = c == 'LIDAR_TOP'
            name = 'samples/%s/n015__%s__%d.%s' % (c, c, stamp, 'pcd.bin' if lidar else 'jpg')
            os.makedirs(os.path.join(dataroot, 'samples', c), exist_ok=True)
            if lidar:
                sweep(rng).tofile(os.path.join(dataroot, name))
            else:
                Image.fromarray(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(
                    os.path.join(dataroot, name), format='PNG')
            sample_data.append(dict(
                token='sd_%s_%d' % (c, i), sample_token='sample_%d' % i, ego_pose_token='pose_%d' % i,
                calibrated_sensor_token='cs_' + c, timestamp=stamp, fileformat='pcd' if lidar else 'jpg',
                is_key_frame=True, height=0 if lidar else H, width=0 if lidar else W, filename=name,
                prev='sd_%s_%d' % (c, i - 1) if i else '', next='sd_%s_%d' % (c, i + 1) if i + 1 < NS else ''))
    scene = [dict(token='scene_0', name='scene-0001', nbr_samples=NS, first_sample_token='sample_0',
                  last_sample_token='sample_%d' % (NS - 1), description='seeded')]
    for name, table in (('sensor', sensor), ('calibrated_sensor', calibrated), ('sample', samples),
                        ('sample_data', sample_data), ('ego_pose', poses), ('scene', scene)):
        with open(os.path.join(tables, name + '.json'), 'w') as f:
            json.dump(table, f)
    split = os.path.join(root, 'nusc_val.txt')
    with open(split, 'w') as f:
        for i in EVAL:
            f.write('sample_%d,sample_%d,sample_%d\n' % (i, i - 1, i + 1))

    def entry(i, ci, frame0=None, intrinsic=None):
        c = CAMS[ci]
        path = lambda j: os.path.join(dataroot, 'samples', c, 'n015__%s__%d.jpg' % (c, 1532402927000000 + 500000 * j))
        pr = np.random.RandomState(1000 + 10 * i + ci)
        pose = lambda: (np.eye(4) + 0.01 * pr.randn(4, 4) * np.array([[1], [1], [1], [0]])).reshape(-1).tolist()
        return {'frame0': frame0 or path(i), 'frame1': path(i + 1), 'frame-1': path(i - 1),
                'P2': np.asarray(intrinsic or cams[c][2]).reshape(-1).tolist(), 'camera_type_indexes': ci,
                'camera_type': c, 'pose01': pose(), 'pose0-1': pose()}

    out = dict(dataroot=dataroot, split=split)
    entries = [entry(i, ci) for i in EVAL for ci in range(len(CAMS))]
    for key in ('json_val', 'json_train'):
        out[key] = os.path.join(root, key + '.json')
        with open(out[key], 'w') as f:
            json.dump(dict(samples=entries), f)
    tall = os.path.join(dataroot, 'samples', 'CAM_BACK', 'tall.jpg')
    Image.fromarray(rng.randint(0, 256, size=(TALL_H, TALL_W, 3)).astype(np.uint8)).save(tall, format='PNG')
    out['json_tall'] = os.path.join(root, 'json_tall.json')
    with open(out['json_tall'], 'w') as f:
        json.dump(dict(samples=[entry(1, 3, frame0=tall), entry(1, 0, frame0=tall)]), f)
    return out


AUG = 'vision_base.data.augmentations.augmentations'
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def raw_augmentation(prefix):
    """no augmentation at all (EmptyAug): the sample as the dataset composes it"""
    return dict(name=prefix + AUG + '.EmptyAug')


def val_augmentation(prefix, h, w):
    """the validation chain of configs/nusc_wpose_example:161-171"""
    return dict(name=prefix + 'vision_base.utils.builder.Sequential', cfg_list=[
        dict(name=prefix + AUG + '.ConvertToFloat'),
        dict(name=prefix + AUG + '.Resize', size=(h, w), preserve_aspect_ratio=False),
        dict(name=prefix + AUG + '.Normalize', mean=MEAN, stds=STD),
        dict(name=prefix + AUG + '.ConvertToTensor')],
        image_keys=[('image', 0)], calib_keys=['P2'])


def key_name(key):
    return repr(key).replace(' ', '')


def flatten_sample(sample, prefix, out, digest_frames=False):
    """a raw sample into npz entries <prefix><key>; returns the keys' names in order.  digest_frames: a uint8 frame
    is stored as (height, width, channels, crc32 of its bytes) — the frames are the tree's files, which the full
    entries of the JSON dataset already pin"""
    import zlib
    names = []
    for key, val in sample.items():
        names.append(key_name(key))
        val = np.asarray(val)
        if digest_frames and val.dtype == np.uint8 and val.ndim == 3:
            val = np.array(list(val.shape) + [zlib.crc32(np.ascontiguousarray(val).tobytes())], np.int64)
        out[prefix + key_name(key)] = val
    return names


def single_loss(depth_0, gt_depth):
    """NuscenesEvaluator._single_loss (nuscenes_unsupervised_eval.py:218-251) in numpy: oracle/eval_oracle.single_loss
    with the nuScenes crop, whose rows start at 0.03594771 of the height (the KITTI one: 0.40810811)"""
    from oracle import eval_oracle as EO
    gt_height, gt_width = gt_depth.shape[:2]
    pred_depth = EO.cv2_resize_linear(depth_0, gt_width, gt_height)
    mask = np.logical_and(gt_depth > 1e-3, gt_depth < 80.0)
    crop = np.array([0.03594771 * gt_height, 0.99189189 * gt_height,
                     0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
    crop_mask = np.zeros(mask.shape)
    crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
    mask = np.logical_and(mask, crop_mask)
    pred_depth = pred_depth[mask]
    gt_depth = gt_depth[mask]
    if len(pred_depth) == 0 or len(gt_depth) == 0:
        raise ValueError
    ratio = np.median(gt_depth) / np.median(pred_depth)
    scaled_depth = pred_depth * ratio
    scaled_depth[scaled_depth < 1e-3] = 1e-3
    scaled_depth[scaled_depth > 80.0] = 80.0
    error = EO.compute_errors(gt_depth, scaled_depth)
    pred_depth[pred_depth < 1e-3] = 1e-3
    pred_depth[pred_depth > 80.0] = 80.0
    abs_error = EO.compute_errors(gt_depth, pred_depth)
    return dict(ratio=ratio, error=error, abs_error=abs_error)
