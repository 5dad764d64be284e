"""Shared set-up of the patched-mask tests: a patched_mask that is not all ones through both device input pipelines.

The expected masks compose the oracle's general primitives (oracle/augment_oracle.py warp_affine_nearest /
resize_nearest) in the reference's order — nearest resample, crop or pad per mode, mirror (augmentations.py:163-190,
:484-487, :412-413) — and tests/golden/augment_mask.npz (tools/gen_golden.py::gen_augment_mask) pins that composition
against the reference's own Resize, RandomWarpAffine and RandomMirror.  Inputs are regenerated from seeds, exactly as
the generator made them."""
import os

import numpy as np

from oracle import augment_oracle as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_mask.npz")
FRAME_IDXS = [0, 1, -1]
AUG = 'vision_base.data.augmentations.augmentations'
BUILDER = 'vision_base.utils.builder'
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.0027]], dtype=np.float64)

# Resize chain: size, then (source shape, mask) per case — the smallest shapes that pad on either side, with a row
# scale that is no round number, and one mask whose every pixel's nearest coordinate matters
RESIZE_SIZE = (36, 64)
RESIZE_CASES = (((90, 150), ("rows", 70)),        # -> 36 x 60, pad_1: 4 zero columns
                ((80, 160), ("rows", 62)),        # -> 32 x 64, pad_0: 4 zero rows
                ((100, 160), ("ones", None)),     # -> 36 x 58, pad_1; the unmasked sample of a mixed, ragged batch
                ((90, 150), ("random", 4101)))    # -> 36 x 60, random 0/1 at p = 0.7
RESIZE_FRAME_SEED = 4000

# warp chain: the KITTI config's scale range on two 90 x 160 samples
WARP_OUT_W, WARP_OUT_H = 64, 40
WARP_KW = dict(scale_lower=0.6, scale_upper=1.4, shift_border=30)
WARP_SEED = 311
WARP_CASES = (((90, 160), ("rows", 70)), ((90, 160), ("random", 4201)))
WARP_FRAME_SEED = 4200


def make_mask(shape, spec):
    """float64 [H, W] like the datasets': ones, rows spec[1] and below zeroed, or seeded random 0/1 at p = 0.7"""
    kind, arg = spec
    m = np.ones(shape)
    if kind == "rows":
        m[arg:, :] = 0
    elif kind == "random":
        m = (np.random.RandomState(arg).rand(*shape) < 0.7).astype(np.float64)
    return m


def make_frames(shape, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=tuple(shape) + (3,)).astype(np.uint8) for _ in FRAME_IDXS]


def sample_dict(frames, mask):
    data = {}
    for i, f in zip(FRAME_IDXS, frames):
        data[('image', i)] = f.copy()
        data[('original_image', i)] = f.copy()
    data['patched_mask'] = mask.copy()
    data['P2'] = P2.copy()
    for i in FRAME_IDXS[1:]:
        data[('relative_pose', i)] = np.eye(4, dtype=np.float32)
    return data


def resize_inputs():
    return [(make_frames(shape, RESIZE_FRAME_SEED + n), make_mask(shape, spec))
            for n, (shape, spec) in enumerate(RESIZE_CASES)]


def warp_inputs():
    return [(make_frames(shape, WARP_FRAME_SEED + n), make_mask(shape, spec))
            for n, (shape, spec) in enumerate(WARP_CASES)]


# ---- expected masks: the oracle's primitives in the reference's order ------------------------------------------------
def expect_resize(mask, mirror, size=RESIZE_SIZE):
    h, w, mode, _ = A.resize_plan(mask.shape, size, True, True)
    out = A._crop_pad(A.resize_nearest(mask, w, h), mode, size)
    return np.ascontiguousarray(out[:, ::-1]) if mirror else out


def expect_warp(mask, M, mirror, out_w=WARP_OUT_W, out_h=WARP_OUT_H):
    out = A.warp_affine_nearest(mask, M, out_w, out_h)
    return np.ascontiguousarray(out[:, ::-1]) if mirror else out


def warp_matrices(shapes, seed=WARP_SEED, out_w=WARP_OUT_W, out_h=WARP_OUT_H, scale_lower=0.6, scale_upper=1.4,
                  shift_border=30):
    """RandomWarpAffine's draws (:464-477) for consecutive samples of one seeded instance"""
    rng = np.random.default_rng(seed)
    out = []
    for height, width in shapes:
        scale = max(height, width) * rng.uniform(scale_lower, scale_upper)
        center_w = rng.integers(low=shift_border, high=width - shift_border)
        center_h = rng.integers(low=shift_border, high=height - shift_border)
        fs = max(out_w, out_h) / scale
        out.append(np.array([[fs, 0, out_w / 2 - center_w * fs], [0, fs, out_h / 2 - center_h * fs]], dtype=np.float32))
    return out


# ---- the chains, for the reference (prefix '') and for the mirrored classes (prefix 'fsnet_amd.') --------------------
def _keys():
    return ([('image', i) for i in FRAME_IDXS] + [('original_image', i) for i in FRAME_IDXS],
            [('image', i) for i in FRAME_IDXS])


def geometry_cfg(kind, mirror, prefix='', gt_image_keys=('patched_mask',)):
    """the geometric stages alone — Resize or RandomWarpAffine, then RandomMirror drawn on (prob 1) or off (prob 0)"""
    keys, _ = _keys()
    aug, b = prefix + AUG, prefix + BUILDER
    if kind == "resize":
        stage = dict(name=aug + '.Resize', size=RESIZE_SIZE, preserve_aspect_ratio=True, force_pad=True)
    else:
        stage = dict(name=aug + '.RandomWarpAffine', output_w=WARP_OUT_W, output_h=WARP_OUT_H, random_seed=WARP_SEED,
                     **WARP_KW)
    return dict(name=b + '.Sequential', cfg_list=[
        dict(name=aug + '.ConvertToFloat'), stage,
        dict(name=aug + '.RandomMirror', mirror_prob=1.0 if mirror else 0.0)],
        image_keys=keys, calib_keys=['P2'], gt_image_keys=list(gt_image_keys))


def train_cfg(kind, mirror, prefix='fsnet_amd.', gt_image_keys=('patched_mask',), size=RESIZE_SIZE):
    """a full device chain around the same geometry: the Normalizes and ConvertToTensor of the shipped configs (no
    colour draws: the mask does not pass through them)"""
    keys, colour = _keys()
    cfg = geometry_cfg(kind, mirror, prefix, gt_image_keys)
    aug = prefix + AUG
    if kind == "resize":
        cfg["cfg_list"][1]["size"] = size
    cfg["cfg_list"] += [
        dict(name=aug + '.Normalize', mean=MEAN, stds=STD, image_keys=colour),
        dict(name=aug + '.Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]),
             image_keys=[('original_image', i) for i in FRAME_IDXS]),
        dict(name=aug + '.ConvertToTensor')]
    return cfg


def nusc_train_augmentation(size, prefix='fsnet_amd.'):
    """the training augmentation of configs/nusc_wpose_example:133-159, written out"""
    keys, colour = _keys()
    aug, b = prefix + AUG, prefix + BUILDER
    return dict(name=b + '.Sequential', cfg_list=[
        dict(name=aug + '.ConvertToFloat'),
        dict(name=aug + '.Resize', size=size, preserve_aspect_ratio=True, force_pad=True),
        dict(name=b + '.Shuffle', cfg_list=[
            dict(name=aug + '.RandomBrightness', distort_prob=1.0),
            dict(name=aug + '.RandomContrast', distort_prob=1.0, lower=0.6, upper=1.4),
            dict(name=b + '.Sequential', cfg_list=[
                dict(name=aug + '.ConvertColor', transform='HSV'),
                dict(name=aug + '.RandomSaturation', distort_prob=1.0, lower=0.6, upper=1.4),
                dict(name=aug + '.ConvertColor', current='HSV', transform='RGB')])],
             image_keys=colour),
        dict(name=aug + '.RandomMirror', mirror_prob=0.5,
             pose_axis_pairs=[(("relative_pose", i), 0) for i in FRAME_IDXS[1:]]),
        dict(name=aug + '.Normalize', mean=MEAN, stds=STD, image_keys=colour),
        dict(name=aug + '.Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]),
             image_keys=[('original_image', i) for i in FRAME_IDXS]),
        dict(name=aug + '.ConvertToTensor')],
        image_keys=keys, calib_keys=['P2'], gt_image_keys=['patched_mask'])


BACK_ROW = 16        # of the 24-row frames of tests/helpers_nusc.make_tree: the lower third is the car's own body


def small_nusc_dataset(json_path, size):
    """NusceneJsonDataset over helpers_nusc's tree with the CAM_BACK cut lowered to fit its 24 x 40 frames"""
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset

    class SmallNusc(NusceneJsonDataset):
        BACK_MASK_FROM_ROW = BACK_ROW

    return SmallNusc(json_path=json_path, augmentation=nusc_train_augmentation(size))
