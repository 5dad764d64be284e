"""Training input pipeline with the pixel work on the device.

Same class names, keyword arguments, random-number streams and dict keys as the reference's
vision_base/data/augmentations/augmentations.py, so configs/kitti_wpose_example:129-155 runs with its `name=`
strings repointed here.  The difference is WHERE pixels are touched: the reference's transforms run cv2 / numpy on
float32 HWC images inside DataLoader workers (3 x 375x1242 frames per sample — at a GPU step of a few ms four
workers cannot keep up); these transforms only draw their random numbers, do the O(1) bookkeeping the reference
does (P2, relative poses) and append to a per-sample *plan*.  Frames stay uint8.  `DeviceAugment.collate` (or
`materialize`) uploads the raw bytes of a batch once and one `fs_augment_frames` launch produces every
('image', i) / ('original_image', i) tensor and the patched mask on the GPU.

The rest of the reference's file — CropTop, CropRight, Pad2Shape, RandomCropToWidth, RandomHue, RandomEigenvalueNoise,
PhotometricDistort, Copy — works the same way.  Before the one resampling stage (RandomWarpAffine or Resize) a crop is
a numpy view of the raw frame and a pad an extent; after it crops, pads and mirrors compose into one output window per
sample; the colour ops are a list of up to 8 drawn ops.  Plans the four earlier launches can express still run them;
the others run `fs_augment_frames_ext` / `fs_resize_frames_ext`.  FilterObject is left out with the object
and lidar keys that RandomMirror refuses.

A transform that is given float images without a plan to extend (i.e. used outside this flow) raises: there is no
CPU pixel path here.
"""
import ctypes as C

import numpy as np
from numpy import random
import torch

from .utils import flip_relative_pose

PLAN = '_fs_aug_plan'
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 0, 1, 2
OP_HUE, OP_NOISE = 3, 4                   # plan["ops"] kinds the three-op launches cannot express
MAX_OPS = 8                               # FS_AUGX_OPS: slots of the extended launches' op list
IMAGE_FAMILY, ORIGINAL_FAMILY = 'image', 'original_image'      # what Copy may copy, and where to


def _plan(data):
    p = data.get(PLAN)
    if p is None:
        p = data[PLAN] = {"warp": None, "mirror": False, "ops": [], "normalize": {}, "hsv": False}
    return p


def _extra_gt(data, keys, shape):
    """ground-truth images other than the patched_mask, which rides in the frames' launch (e.g. a precomputed
    'motion_mask'): uint8 [H, W] of the frame's size, kept raw for DeviceAugment, which samples them with the frames'
    plan (fs_augment_masks)"""
    plan = _plan(data)
    extra = plan.setdefault("gt_extra", [])
    shape = _raw_hw(plan, shape)
    for key in keys:
        if key == 'patched_mask' or key not in data:
            continue
        m = data[key]
        if not (isinstance(m, np.ndarray) and m.dtype == np.uint8 and m.ndim == 2 and m.shape == tuple(shape[:2])):
            raise TypeError("ground-truth image %r must be uint8 [H, W] of the frame's size, got %s %s" % (
                key, getattr(m, "dtype", type(m)), getattr(m, "shape", "")))
        if key not in extra:
            extra.append(key)


def _patched_mask(data, keys, shape):
    """the sample's patched_mask when `keys` (a stage's gt_image_keys) lists it: every pixel is looked at.  All ones is
    the mask the kernels synthesise and leaves the plan alone; values in {0, 1} (NusceneJsonDataset zeroes the car's own
    body in CAM_BACK, nuscene_dataset.py:176-191) are recorded as uint8 for DeviceAugment, which samples them in the
    frames' launch (fs_augment_frames_masked / fs_resize_frames_masked).  The sample's own entry stays as the dataset
    made it."""
    if 'patched_mask' not in keys or 'patched_mask' not in data:
        return
    m = np.asarray(data['patched_mask'])
    pad = _plan(data).get("src_pad")
    shape = _raw_hw(_plan(data), shape)
    if m.shape[:2] != tuple(shape[:2]):
        raise NotImplementedError("the device path samples a patched_mask of the frame's size %s, got %s" % (
            tuple(shape[:2]), m.shape))
    if bool(np.all(m == 1)) and pad is None:
        return
    if m.ndim != 2 or not bool(np.all((m == 0) | (m == 1))):
        raise NotImplementedError("the device path samples a [H, W] patched_mask with values in {0, 1}")
    if pad is not None:      # Pad2Shape before the resampling stage: np.pad's zeros around the mask, ones included
        full = np.zeros(pad["hw"], dtype=np.uint8)
        full[:m.shape[0], :m.shape[1]] = m
        m = full
    _plan(data)["patched_mask"] = m.astype(np.uint8)


def _raw_hw(plan, shape):
    """the extent the sample's own arrays have: `shape` unless a Pad2Shape before the resampling stage widened it"""
    pad = plan.get("src_pad")
    return tuple(shape[:2]) if pad is None else pad["raw"]


def _frame_shape(data, key):
    img = data[key]
    if not (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3):
        raise TypeError("fsnet_amd augmentations plan device work over raw uint8 HWC frames; %r is %s" % (
            key, getattr(img, "dtype", type(img))))
    pad = data[PLAN].get("src_pad") if PLAN in data else None
    if pad is not None:      # the padded extent: collate places the frame in the top-left of a zeroed buffer
        return tuple(pad["hw"]) + img.shape[2:]
    return img.shape


# ---- geometry after the resampling stage: one output window over the warp's / resize's canvas -------------------
# Crops, pads and mirrors that follow the one resampling stage touch no pixel on the host.  They compose, in their
# order, into a map from the current image to the canvas — canvas x = sx * x + ox (sx = -1 after an odd number of
# mirrors), canvas y = y + oy — and a rectangle `valid` of the current image outside which the pixel is np.pad's zero.
def _stage(plan):
    return plan["warp"] if plan["warp"] is not None else plan.get("resize")


def _window(plan):
    win = plan.get("win")
    if win is None:
        st = _stage(plan)
        win = plan["win"] = dict(w=st["out_w"], h=st["out_h"], sx=1, ox=0, oy=0, valid=[0, 0, st["out_w"], st["out_h"]])
        if plan["mirror"]:                      # a RandomMirror drawn before the first crop / pad
            _win_mirror(win)
    return win


def _win_mirror(win):
    w = win["w"]
    win["ox"] += win["sx"] * (w - 1)
    win["sx"] = -win["sx"]
    vx0, vy0, vx1, vy1 = win["valid"]
    win["valid"] = [w - vx1, vy0, w - vx0, vy1]


def _win_crop(win, x0, x1, y0, y1):
    win["ox"] += win["sx"] * x0
    win["oy"] += y0
    w, h = x1 - x0, y1 - y0
    vx0, vy0, vx1, vy1 = win["valid"]
    win["valid"] = [min(max(vx0 - x0, 0), w), min(max(vy0 - y0, 0), h), min(max(vx1 - x0, 0), w), min(max(vy1 - y0, 0), h)]
    win["w"], win["h"] = w, h


def window_row(win):
    """the kernels' row (FsAugExtArgs::win): flip, x_off, y_off, valid rectangle"""
    return [int(win["sx"] < 0), win["ox"], win["oy"]] + list(win["valid"]) + [0]


def _current_hw(data, plan, key):
    """(height, width) of the image as the chain sees it now"""
    if plan.get("win") is not None:
        return plan["win"]["h"], plan["win"]["w"]
    st = _stage(plan)
    if st is not None:
        return st["out_h"], st["out_w"]
    return tuple(_frame_shape(data, key)[:2])


def _identity_stage(data, plan, image_keys, gt_image_keys):
    """a chain without RandomWarpAffine / Resize: a resize whose target is the source extent (the coordinate is the
    integer pixel with fraction 0, so the frame comes through exactly)"""
    shape = _frame_shape(data, image_keys[0])
    gt = [k for k in gt_image_keys if k in data]
    _extra_gt(data, gt, shape)
    _patched_mask(data, gt, shape)
    plan["resize"] = dict(h=shape[0], w=shape[1], mode='none', out_h=shape[0], out_w=shape[1], keys=list(image_keys),
                          gt_keys=gt, src_hw=(shape[0], shape[1]), identity=True)


def _copy_covers(plan, image_keys):
    """after a Copy the originals are images of their own: geometry that leaves them out would part them from theirs"""
    if plan.get("copy_to") and not set(plan["copy_to"]) <= set(image_keys):
        raise NotImplementedError("a mirror, crop or pad after Copy must list the copied keys among its image_keys")


def _pad_covers(data, plan, gt_image_keys):
    pad = plan.get("src_pad")
    if pad is not None and pad["gt_keys"] != [k for k in gt_image_keys if k in data]:
        raise NotImplementedError("a Pad2Shape before the resampling stage pads that stage's gt_image_keys")


def _after_resampling(data, plan, image_keys, gt_image_keys):
    """where a crop / pad stands: False while the frames are raw and nothing was drawn on them (the crop is a numpy
    view, the pad an extent), True once a resampling stage, a drawn mirror or a colour op precedes it"""
    plan.setdefault("gt_keys_seen", list(gt_image_keys))
    _copy_covers(plan, image_keys)
    st = _stage(plan)
    if st is None:
        if not (plan["mirror"] or plan["ops"]):
            return False
        _identity_stage(data, plan, image_keys, gt_image_keys)
        st = plan["resize"]
    if list(image_keys) != st["keys"] or [k for k in gt_image_keys if k in data] != [k for k in st["gt_keys"] if k in data]:
        raise NotImplementedError("a crop or pad after the resampling stage addresses that stage's image_keys and "
                                  "gt_image_keys")
    return True


def _crop(data, plan, image_keys, gt_image_keys, rows=None, cols=None):
    """data[key][rows[0]:rows[1], cols[0]:cols[1]] for the image and ground-truth image keys, numpy's slice rules"""
    h, w = _current_hw(data, plan, image_keys[0])
    y0, y1, _ = slice(*rows).indices(h) if rows is not None else (0, h, 1)
    x0, x1, _ = slice(*cols).indices(w) if cols is not None else (0, w, 1)
    if y1 <= y0 or x1 <= x0:
        raise ValueError("the crop [%s:%s, %s:%s] of a %d x %d image leaves an empty image" % (y0, y1, x0, x1, h, w))
    if _after_resampling(data, plan, image_keys, gt_image_keys):
        _win_crop(_window(plan), x0, x1, y0, y1)
        return
    if plan.get("src_pad") is not None:
        raise NotImplementedError("a crop after a Pad2Shape that precedes the resampling stage")
    for key in list(image_keys) + list(gt_image_keys):
        data[key] = data[key][y0:y1, x0:x1]              # a view: collate uploads only the window


class EmptyAug(object):
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, data):
        return data


class ExtractData(object):
    """reference :30-47"""
    def __init__(self, extract_keys=[], mapped_keys={}):
        self.extract_keys, self.mapped_keys = extract_keys, mapped_keys

    def __call__(self, data):
        out = {k: data[k] for k in self.extract_keys}
        for k, new in self.mapped_keys.items():
            out[new] = data[k]
        if PLAN in data:
            out[PLAN] = data[PLAN]
        return out


class ConvertToFloat(object):
    """reference :50-59.  Frames stay uint8 here; the kernel converts while it samples."""
    def __init__(self, image_keys=['image'], **kwargs):
        self.image_keys = image_keys

    def __call__(self, data):
        for key in self.image_keys:
            _frame_shape(data, key)
        _plan(data)
        return data


class Resize(object):
    """reference :112-198: cv2.resize to (h, w), then crop / zero-pad to `size`; P2 rows scale.  The validation input
    of every shipped config, and the first stage of the training input of the Resize-based ones
    (configs/multi_dataset_example:183, nusc / kitti360_fisheye examples), where colour ops, RandomMirror and the
    Normalizes follow and `gt_image_keys` carries the patched mask (cv2.INTER_NEAREST)."""
    def __init__(self, size, preserve_aspect_ratio=True, force_pad=True, image_keys=['image'], calib_keys=[],
                 gt_image_keys=[], **kwargs):
        self.size, self.preserve_aspect_ratio, self.force_pad = size, preserve_aspect_ratio, force_pad
        self.image_keys, self.calib_keys, self.gt_image_keys = image_keys, calib_keys, list(gt_image_keys)

    def __call__(self, data):
        shape = _frame_shape(data, self.image_keys[0])
        plan = _plan(data)
        if plan["warp"] is not None or plan.get("resize") is not None or plan["ops"] or plan["mirror"]:
            raise NotImplementedError("Resize is the first (and only geometric) stage of a device pipeline")
        _pad_covers(data, plan, self.gt_image_keys)
        _extra_gt(data, self.gt_image_keys, shape)
        _patched_mask(data, self.gt_image_keys, shape)
        data[('image_resize', 'original_shape')] = np.array([shape[0], shape[1]]).astype(int)
        if self.preserve_aspect_ratio:
            scale_factor_x = self.size[0] / shape[0]
            scale_factor_y = self.size[1] / shape[1]
            if self.force_pad:
                scale_factor = min(scale_factor_x, scale_factor_y)
                mode = 'pad_0' if scale_factor_x > scale_factor_y else 'pad_1'
            else:
                scale_factor = scale_factor_x
                mode = 'crop_1' if scale_factor_x > scale_factor_y else 'pad_1'
            h = int(np.round(shape[0] * scale_factor).astype(int))
            w = int(np.round(shape[1] * scale_factor).astype(int))
            scale_factor_yx = (scale_factor, scale_factor)
        else:
            scale_factor_yx = (self.size[0] / shape[0], self.size[1] / shape[1])
            mode, h, w = 'none', self.size[0], self.size[1]
        data[('image_resize', 'effective_size')] = np.array([h, w]).astype(int)
        if len(self.size) <= 1:
            raise NotImplementedError("Resize needs a (height, width) size on the device path")
        plan["resize"] = dict(h=h, w=w, mode=mode, out_h=self.size[0], out_w=self.size[1], keys=list(self.image_keys),
                              gt_keys=list(self.gt_image_keys), src_hw=(shape[0], shape[1]))
        for key in self.calib_keys:
            P = data[key]
            P[0, :] = P[0, :] * scale_factor_yx[1]
            P[1, :] = P[1, :] * scale_factor_yx[0]
            data[key] = P
        return data


class RandomWarpAffine(object):
    """reference :436-497: random scale about a random centre, resized to (output_w, output_h); P2 follows."""
    def __init__(self, scale_lower=0.6, scale_upper=1.4, shift_border=128, output_w=1280, output_h=384,
                 image_keys=['image'], gt_image_keys=[], calib_keys=[], border_mode=0, random_seed=None, **kwargs):
        if border_mode != 0:
            raise NotImplementedError("only cv2.BORDER_CONSTANT (0) is implemented on the device")
        self.scale_lower, self.scale_upper, self.shift_border = scale_lower, scale_upper, shift_border
        self.output_w, self.output_h = output_w, output_h
        self.image_keys, self.gt_image_keys, self.calib_keys = image_keys, gt_image_keys, calib_keys
        self.rng = np.random.default_rng(random_seed if random_seed is not None else np.random.randint(0, 2**32))

    def __call__(self, data):
        height, width = _frame_shape(data, self.image_keys[0])[0:2]
        plan = _plan(data)
        if plan["warp"] is not None or plan["mirror"] or plan["ops"]:
            raise NotImplementedError("the device pipeline warps once, before mirror and colour ops")
        scale = max(height, width) * self.rng.uniform(self.scale_lower, self.scale_upper)
        center_w = self.rng.integers(low=self.shift_border, high=width - self.shift_border)
        center_h = self.rng.integers(low=self.shift_border, high=height - self.shift_border)
        _pad_covers(data, plan, self.gt_image_keys)
        _extra_gt(data, self.gt_image_keys, (height, width))
        _patched_mask(data, self.gt_image_keys, (height, width))
        final_scale = max(self.output_w, self.output_h) / scale
        shift_w = self.output_w / 2 - center_w * final_scale
        shift_h = self.output_h / 2 - center_h * final_scale
        plan["warp"] = dict(M=np.array([[final_scale, 0, shift_w], [0, final_scale, shift_h]], dtype=np.float32),
                            out_w=self.output_w, out_h=self.output_h, keys=list(self.image_keys),
                            gt_keys=list(self.gt_image_keys), src_hw=(height, width))
        for key in self.calib_keys:
            P = data[key]
            P[0:2, :] *= final_scale
            P[0, 2] = P[0, 2] + shift_w
            P[0, 3] = P[0, 3] + shift_w * P[2, 3]
            P[1, 2] = P[1, 2] + shift_h
            P[1, 3] = P[1, 3] + shift_h * P[2, 3]
            data[key] = P
        return data


class CropTop(object):
    """reference :228-265: rows crop_top_index .. height (or the last output_height rows); P[1, 2], P[1, 3] follow."""
    def __init__(self, crop_top_index=None, output_height=None, image_keys=['image'], gt_image_keys=[], calib_keys=[],
                 **kwargs):
        if crop_top_index is None and output_height is None:
            print("Either crop_top_index or output_height should not be None, set crop_top_index=0 by default")
            crop_top_index = 0
        if crop_top_index is not None and output_height is not None:
            print("Neither crop_top_index or output_height is None, crop_top_index will take over")
        self.crop_top_index, self.output_height = crop_top_index, output_height
        self.image_keys, self.calib_keys, self.gt_image_keys = image_keys, calib_keys, gt_image_keys

    def __call__(self, data):
        plan = _plan(data)
        height = _current_hw(data, plan, self.image_keys[0])[0]
        upper = self.crop_top_index if self.crop_top_index is not None else height - self.output_height
        _crop(data, plan, self.image_keys, self.gt_image_keys, rows=(upper, height))
        for key in self.calib_keys:
            P = data[key]
            P[1, 2] = P[1, 2] - upper
            P[1, 3] = P[1, 3] - upper * P[2, 3]
            data[key] = P
        return data


class CropRight(object):
    """reference :268-301: columns 0 .. width - crop_right_index (or 0 .. output_width); P2 is not touched.  The
    reference's class cannot be called — its __init__ never stores image_keys, so the first __call__ raises
    AttributeError; this one stores them and does what the reference's __call__ spells out."""
    def __init__(self, crop_right_index=None, output_width=None, image_keys=['image'], gt_image_keys=[], **kwargs):
        if crop_right_index is None and output_width is None:
            print("Either crop_right_index or output_width should not be None, set crop_right_index=0 by default")
            crop_right_index = 0
        if crop_right_index is not None and output_width is not None:
            print("Neither crop_right_index or output_width is None, crop_right_index will take over")
        self.crop_right_index, self.output_width = crop_right_index, output_width
        self.image_keys, self.gt_image_keys = image_keys, gt_image_keys

    def __call__(self, data):
        plan = _plan(data)
        width = _current_hw(data, plan, self.image_keys[0])[1]
        righter = width - self.crop_right_index if self.crop_right_index is not None else self.output_width
        if righter > width:
            print("does not crop right since it is larger")
            return data
        _crop(data, plan, self.image_keys, self.gt_image_keys, cols=(0, righter))
        return data


class Pad2Shape(object):
    """reference :304-324: np.pad with zeros at the bottom and the right, up to target_shape (height, width)."""
    def __init__(self, target_shape, image_keys=['image'], gt_image_keys=[], **kwargs):
        self.target_shape, self.image_keys, self.gt_image_keys = target_shape, image_keys, gt_image_keys

    def __call__(self, data):
        plan = _plan(data)
        height, width = _current_hw(data, plan, self.image_keys[0])
        th, tw = int(self.target_shape[0]), int(self.target_shape[1])
        if th < height or tw < width:
            raise ValueError("Pad2Shape to %d x %d, smaller than the %d x %d image" % (th, tw, height, width))
        if plan["ops"]:
            raise NotImplementedError("Pad2Shape after a colour op: its zeros would have to skip the colour ops that "
                                      "precede it, which the device path does not do")
        if _after_resampling(data, plan, self.image_keys, self.gt_image_keys):
            win = _window(plan)
            win["w"], win["h"] = tw, th
        else:       # no pixel is copied: the frames keep their size, the plan the extent they are placed in
            raw = _raw_hw(plan, _frame_shape(data, self.image_keys[0]))
            plan["src_pad"] = dict(hw=(th, tw), raw=raw, gt_keys=[k for k in self.gt_image_keys if k in data])
        return data


class RandomCropToWidth(object):
    """reference :343-375: a random window of `width` columns from the global stream; P[0, 2], P[0, 3] follow.  Like
    the reference it takes no **kwargs."""
    def __init__(self, width: int, image_keys=['image'], gt_image_keys=[], calib_keys=[],):
        self.width = width
        self.image_keys, self.calib_keys, self.gt_image_keys = image_keys, calib_keys, gt_image_keys

    def __call__(self, data):
        plan = _plan(data)
        original_width = _current_hw(data, plan, self.image_keys[0])[1]
        if self.width > original_width:
            print("does not crop since it is larger")
            return data
        lefter = np.random.randint(0, original_width - self.width)     # equal widths: numpy's ValueError, as there
        righter = lefter + self.width
        _crop(data, plan, self.image_keys, self.gt_image_keys, cols=(lefter, righter))
        for key in self.calib_keys:
            P = data[key]
            P[0, 2] = P[0, 2] - lefter
            P[0, 3] = P[0, 3] - lefter * P[2, 3]
            data[key] = P
        return data


class RandomMirror(object):
    """reference :377-433 (global np.random stream, like the reference)."""
    def __init__(self, mirror_prob, image_keys=['image'], calib_keys=[], gt_image_keys=[], object_keys=[],
                 lidar_keys=[], pose_axis_pairs=[], is_switch_left_right=True, stereo_image_key_pairs=[],
                 stereo_calib_key_pairs=[], **kwargs):
        if object_keys or lidar_keys or stereo_image_key_pairs or stereo_calib_key_pairs:
            raise NotImplementedError("object / lidar / stereo-pair mirroring is outside the monodepth hot path")
        self.mirror_prob = mirror_prob
        self.image_keys, self.calib_keys, self.gt_image_keys = image_keys, calib_keys, gt_image_keys
        self.pose_axis_pairs = pose_axis_pairs

    def __call__(self, data):
        plan = _plan(data)
        plan.setdefault("gt_keys_seen", list(self.gt_image_keys))
        width = _current_hw(data, plan, self.image_keys[0])[1]      # the width the crops and pads so far left
        if random.rand() <= self.mirror_prob:
            # (the colour ops are per-pixel: a flip before or after them is the same image, so the kernel's fixed
            # order — sample mirrored, then colour — serves configs that mirror first and configs that mirror last)
            _copy_covers(plan, self.image_keys)
            plan["mirror"] = not plan["mirror"]
            if plan.get("win") is not None:
                _win_mirror(plan["win"])
            for key in self.calib_keys:
                P = data[key]
                P[0, 3] = -P[0, 3]
                P[0, 2] = width - P[0, 2] - 1
                data[key] = P
            for key, axis_num in self.pose_axis_pairs:
                data[key] = flip_relative_pose(data[key], axis_num)
        return data


class _ColourOp(object):
    def __init__(self, distort_prob, image_keys, random_seed):
        self.distort_prob, self.image_keys = distort_prob, image_keys
        self.rng = np.random.default_rng(random_seed if random_seed is not None else np.random.randint(0, 2**32))

    def _record(self, data, op, value):
        plan = _plan(data)
        prev = plan.setdefault("colour_keys", list(self.image_keys))
        if list(self.image_keys) != prev:
            raise NotImplementedError("all colour ops of a pipeline must address the same image keys")
        plan["ops"].append((op, value))
        return data


class RandomBrightness(_ColourOp):
    """reference :572-591"""
    def __init__(self, distort_prob, delta=32, image_keys=['image'], random_seed=None, **kwargs):
        assert 0.0 <= delta <= 255.0
        super().__init__(distort_prob, image_keys, random_seed)
        self.delta = delta

    def __call__(self, data):
        value = self.rng.uniform(-self.delta, self.delta) if self.rng.random() <= self.distort_prob else None
        if _plan(data)["hsv"]:
            raise NotImplementedError("brightness is applied in RGB")
        return self._record(data, OP_BRIGHTNESS, value)


class RandomContrast(_ColourOp):
    """reference :545-569"""
    def __init__(self, distort_prob, lower=0.5, upper=1.5, image_keys=['image'], random_seed=None, **kwargs):
        assert upper >= lower >= 0, "contrast bounds"
        super().__init__(distort_prob, image_keys, random_seed)
        self.lower, self.upper = lower, upper

    def __call__(self, data):
        value = self.rng.uniform(self.lower, self.upper) if self.rng.random() <= self.distort_prob else None
        if _plan(data)["hsv"]:
            raise NotImplementedError("contrast is applied in RGB")
        return self._record(data, OP_CONTRAST, value)


class ConvertColor(object):
    """reference :527-542.  RGB->HSV opens a saturation op, HSV->RGB closes it: the kernel fuses the round trip."""
    def __init__(self, current='RGB', transform='HSV', image_keys=['image'], **kwargs):
        if (current, transform) not in (('RGB', 'HSV'), ('HSV', 'RGB')):
            raise NotImplementedError("only RGB<->HSV is implemented on the device")
        self.current, self.transform, self.image_keys = current, transform, image_keys

    def __call__(self, data):
        plan = _plan(data)
        if self.transform == 'HSV':
            if plan["hsv"]:
                raise ValueError("image is already HSV")
            if any(o == OP_NOISE and v is not None for o, v in plan["ops"]):
                raise NotImplementedError("ConvertColor after RandomEigenvalueNoise: the noise made the image float64, "
                                          "and OpenCV converts only 8-bit, 16-bit and 32-bit float images to HSV")
            plan["hsv"] = True
            # the section's slot: a bare round trip unless RandomSaturation / RandomHue fill it in
            plan["hsv_section"] = dict(at=len(plan["ops"]), saturation=False, hue=False)
            plan["ops"].append((OP_SATURATION, None))
        else:
            if not plan["hsv"]:
                raise ValueError("image is not HSV")
            plan["hsv"] = False
            plan.pop("hsv_section", None)
        return data


class RandomSaturation(_ColourOp):
    """reference :200-226 (expects HSV, i.e. between the two ConvertColor stages; once per such section)."""
    def __init__(self, distort_prob, lower=0.5, upper=1.5, image_keys=['image'], random_seed=None, **kwargs):
        assert upper >= lower >= 0, "saturation bounds"
        super().__init__(distort_prob, image_keys, random_seed)
        self.lower, self.upper = lower, upper

    def __call__(self, data):
        plan = _plan(data)
        value = self.rng.uniform(self.lower, self.upper) if self.rng.random() <= self.distort_prob else None
        sec = plan.get("hsv_section")
        if not plan["hsv"] or sec is None or sec["saturation"]:
            raise NotImplementedError("RandomSaturation must be inside an HSV section (between the two ConvertColor "
                                      "stages) that has no RandomSaturation yet")
        sec["saturation"] = True
        plan["ops"][sec["at"]] = (OP_SATURATION, value)
        plan.setdefault("colour_keys", list(self.image_keys))
        return data


class RandomHue(_ColourOp):
    """reference :500-524 (expects HSV; once per section): h += shift in fp32, then h > 360 -> h - 360, then h < 0 ->
    h + 360.  Hue and saturation are different channels, so either order inside the section gives the same image: the
    shift is recorded right after the section's slot."""
    def __init__(self, distort_prob, delta=18.0, image_keys=['image'], random_seed=None, **kwargs):
        assert 0.0 <= delta <= 360.0
        super().__init__(distort_prob, image_keys, random_seed)
        self.delta = delta

    def __call__(self, data):
        plan = _plan(data)
        value = self.rng.uniform(-self.delta, self.delta) if self.rng.random() <= self.distort_prob else None
        sec = plan.get("hsv_section")
        if not plan["hsv"] or sec is None or sec["hue"]:
            raise NotImplementedError("RandomHue must be inside an HSV section (between the two ConvertColor stages) "
                                      "that has no RandomHue yet")
        sec["hue"] = True
        plan["ops"].insert(sec["at"] + 1, (OP_HUE, value))
        plan.setdefault("colour_keys", list(self.image_keys))
        return data


class RandomEigenvalueNoise(_ColourOp):
    """reference :594-626: ImageNet PCA noise.  The reference adds a float64 array to the float32 image, so the image is
    float64 from here on; the kernel carries the pixel in double to the end of the colour ops."""
    def __init__(self, distort_prob=1.0, alphastd=0.1,
                 eigen_value=np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32),
                 eigen_vector=np.array([[-0.58752847, -0.69563484, 0.41340352],
                                        [-0.5832747, 0.00994535, -0.81221408],
                                        [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32),
                 image_keys=['image'], random_seed=None, **kwargs):
        super().__init__(distort_prob, image_keys, random_seed)
        self._eig_val, self._eig_vec, self.alphastd = eigen_value, eigen_vector, alphastd

    def __call__(self, data):
        value = None
        if self.rng.random() <= self.distort_prob:
            alpha = self.rng.normal(scale=self.alphastd, size=(3, ))
            value = np.asarray(np.dot(self._eig_vec, self._eig_val * alpha) * 255, dtype=np.float64)
        if _plan(data)["hsv"]:
            raise NotImplementedError("the eigenvalue noise is applied in RGB")
        return self._record(data, OP_NOISE, value)


class PhotometricDistort(object):
    """reference :628-666: brightness, then contrast before or after one HSV section with saturation and hue.  The
    sub-ops are built in the reference's order, so they take their seeds from the global stream as there."""
    def __init__(self, distort_prob=1.0, contrast_lower=0.5, contrast_upper=1.5, saturation_lower=0.5,
                 saturation_upper=1.5, hue_delta=18.0, brightness_delta=32, image_keys=['image'], **kwargs):
        self.distort_prob = distort_prob
        self.transforms = [
            RandomContrast(distort_prob, contrast_lower, contrast_upper, image_keys=image_keys),
            ConvertColor(transform='HSV', image_keys=image_keys),
            RandomSaturation(distort_prob, saturation_lower, saturation_upper, image_keys=image_keys),
            RandomHue(distort_prob, hue_delta, image_keys=image_keys),
            ConvertColor(current='HSV', transform='RGB', image_keys=image_keys),
            RandomContrast(distort_prob, contrast_lower, contrast_upper, image_keys=image_keys)]
        self.rand_brightness = RandomBrightness(distort_prob, brightness_delta, image_keys=image_keys)

    def __call__(self, data):
        distortion = self.transforms[:-1] if random.rand() <= 0.5 else self.transforms[1:]      # contrast first / last
        for transform in [self.rand_brightness] + distortion:
            data = transform(data)
        return data


class Copy(object):
    """reference :668-680, for the one use the shipped configs make of it (configs/kitti360_fisheye_example:139):
    ('original_image', i) = ('image', i) as it is at this point of the chain.  The host hands the same uint8 view on;
    the plan records how many colour ops precede the copy, and the kernel writes the original after that many."""
    def __init__(self, from_keys, to_keys, **kwargs):
        self.from_keys, self.to_keys = from_keys, to_keys

    def __call__(self, data):
        plan = _plan(data)
        for a, b in zip(self.from_keys, self.to_keys):
            if not (isinstance(a, tuple) and isinstance(b, tuple) and len(a) == 2 and len(b) == 2
                    and a[0] == IMAGE_FAMILY and b[0] == ORIGINAL_FAMILY and a[1] == b[1]):
                raise NotImplementedError("the device path copies ('image', i) to ('original_image', i), not %r to %r"
                                          % (a, b))
        if plan["hsv"]:
            raise NotImplementedError("Copy inside an HSV section")
        if "copy_at" in plan:
            raise NotImplementedError("one Copy per chain")
        plan["copy_at"] = len(plan["ops"])
        plan["copy_to"] = list(self.to_keys)
        for a, b in zip(self.from_keys, self.to_keys):
            data[b] = data[a]
        return data


class Normalize(object):
    """reference :91-109: (x / 255 - mean) / std per channel, recorded per image key."""
    def __init__(self, mean, stds, image_keys=['image'], **kwargs):
        self.mean = np.array(mean, dtype=np.float32)
        self.stds = np.array(stds, dtype=np.float32)
        self.image_keys = image_keys

    def __call__(self, data):
        plan = _plan(data)
        if plan["hsv"]:
            raise ValueError("Normalize on an HSV image")
        for key in self.image_keys:
            if key in plan["normalize"]:
                raise NotImplementedError("one Normalize per image key")
            plan["normalize"][key] = (self.mean.copy(), self.stds.copy())
        return data


class ConvertToTensor(object):
    """reference :62-88.  Calibration / pose entries become tensors; frames stay raw for DeviceAugment."""
    def __init__(self, image_keys=['image'], gt_image_keys=[], calib_keys=[], lidar_keys=[], **kwargs):
        self.image_keys, self.gt_image_keys = image_keys, gt_image_keys
        self.calib_keys, self.lidar_keys = calib_keys, lidar_keys

    def __call__(self, data):
        for key in self.calib_keys + self.lidar_keys:
            data[key] = torch.tensor(data[key], dtype=torch.float32).contiguous()
        return data


# ------------------------------------------------------------------------------------------------
# execution
# ------------------------------------------------------------------------------------------------
def invert_affine(M):
    """cv2.warpAffine's inversion of the forward 2x3 matrix, in float64 (OpenCV imgwarp.cpp)."""
    m = np.asarray(M, dtype=np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = a11, m[1] * -D, m[3] * -D, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


class DeviceAugment(object):
    """Batch executor: `collate(samples)` is a DataLoader collate_fn (keeps everything on the host, stacks the raw
    frames into one pinned uint8 buffer), `materialize(batch, device)` runs the kernel; calling the object does both.

    frame_keys: image-key families that share a frame index, default ('image', 'original_image') as in
    mono_dataset.py:188-190 — ('original_image', i) is the unaugmented copy of ('image', i)."""

    def __init__(self, frame_idxs=(0, 1, -1), image_family='image', original_family='original_image',
                 mask_key='patched_mask', device=None):
        self.frame_idxs = list(frame_idxs)
        self.image_family, self.original_family, self.mask_key = image_family, original_family, mask_key
        self.device = device

    # -- host side ---------------------------------------------------------------------------------
    @staticmethod
    def _colour_plan(p, iplan_row, fplan_row):
        """pack one sample's colour ops / mirror flag into the kernels' plan rows (FsAugArgs layout)"""
        ops = list(p["ops"])
        if len(ops) > 3 or len({o for o, _ in ops}) != len(ops):
            raise NotImplementedError("at most one brightness, contrast and saturation op per sample")
        applied = 0
        order = [o for o, _ in ops]
        for o, v in ops:
            if o == OP_SATURATION:
                applied |= 8                      # the HSV round trip itself runs
            if v is not None:
                applied |= 1 << o
                fplan_row[o] = v
        while len(order) < 3:
            order.append(3)                       # 3 = no-op slot
        iplan_row[0:3] = order[:3]
        iplan_row[3] = applied
        iplan_row[4] = int(p["mirror"])

    def _check_normalize(self, s, p, mean, std):
        for idx in self.frame_idxs:
            want = p["normalize"].get((self.image_family, idx), (mean, std))
            if not (np.array_equal(want[0], mean) and np.array_equal(want[1], std)):
                raise NotImplementedError("one mean/std for all augmented frames")
            om, osd = p["normalize"].get((self.original_family, idx), (np.zeros(3, np.float32), np.ones(3, np.float32)))
            if np.any(om != 0) or np.any(osd != 1):
                raise NotImplementedError("('original_image', i) is normalised with mean 0 / std 1")

    def _stack_frames(self, samples, plans, stage, zeroed, checked=True):
        """the batch's raw frames in one uint8 [B, F, Hs, Ws, 3] buffer, sample b's in the top-left of its slab, and the
        mean / std of ('image', first index) -> (src, Hs, Ws, mean, std).  zeroed: the slack around smaller frames
        (ragged sizes, Pad2Shape's padding) is zero; a batch of equal frames may then stay uninitialised until the copy.
        checked: the frames of a sample share the plan's size, ('original_image', i) is the same picture, one
        Normalize serves the batch — the validation input has never asked for these."""
        B, F = len(samples), len(self.frame_idxs)
        Hs = max(p[stage]["src_hw"][0] for p in plans)
        Ws = max(p[stage]["src_hw"][1] for p in plans)
        ragged = any(tuple(p[stage]["src_hw"]) != (Hs, Ws) for p in plans)
        # pageable here (collate may run in a DataLoader worker); the loader's pin_memory thread pins it
        src = (torch.zeros if zeroed or ragged else torch.empty)(B, F, Hs, Ws, 3, dtype=torch.uint8)
        src_np = src.numpy()
        key0 = (self.image_family, self.frame_idxs[0])
        mean, std = plans[0]["normalize"].get(key0, (np.zeros(3, np.float32), np.ones(3, np.float32)))
        for b, (s, p) in enumerate(zip(samples, plans)):
            h, w = _raw_hw(p, p[stage]["src_hw"])
            for f, idx in enumerate(self.frame_idxs):
                frame = s[(self.image_family, idx)]
                if checked and frame.shape != (h, w, 3):
                    raise ValueError("frames of one sample must share their size")
                src_np[b, f, :h, :w] = frame
                okey = (self.original_family, idx)
                if checked and okey in s and s[okey] is not frame and (
                        s[okey].shape != frame.shape or not np.array_equal(s[okey][::16, ::16], frame[::16, ::16])):
                    raise ValueError("%r is expected to be the unaugmented copy of the image" % (okey,))
            if checked:
                self._check_normalize(s, p, mean, std)
        return src, Hs, Ws, mean, std

    def _colour_rows(self, plans):
        iplan = np.zeros((len(plans), 8), dtype=np.int32)
        fplan = np.zeros((len(plans), 4), dtype=np.float32)
        for b, p in enumerate(plans):
            self._colour_plan(p, iplan[b], fplan[b])
        return iplan, fplan

    def _finish(self, samples, plans, plan, Hs, Ws, stage, gt=True):
        """the collated batch around one plan: the patched-mask plane and the extra ground-truth images (training
        plans), then every other key of the samples"""
        batch = {PLAN: plan}
        if gt:
            self._collate_mask(plans, batch, Hs, Ws, stage)
            self._collate_gt(samples, plans, batch)
        self._collate_rest(samples, batch)
        return batch

    def _collate_resize(self, samples, plans):
        r0 = plans[0]["resize"]
        out_hw = (r0["out_h"], r0["out_w"])
        # training use (Resize-based configs): the resize also feeds ('original_image', i) and the patched mask, and
        # colour ops / a mirror may follow it
        train = any((self.original_family, i) in r0["keys"] for i in self.frame_idxs) or bool(r0.get("gt_keys"))
        for p in plans:
            r = p["resize"]
            if train and (p["warp"] is not None or p["hsv"] or (r["out_h"], r["out_w"]) != out_hw):
                raise NotImplementedError("a Resize-based training batch shares one output size and ends in RGB")
            if not train and (p["warp"] is not None or p["ops"] or p["mirror"] or (r["out_h"], r["out_w"]) != out_hw):
                raise NotImplementedError("a validation batch is Resize + Normalize with one output size")
            if not train and p.get("gt_extra"):
                raise NotImplementedError("ground-truth images %r travel with a training Resize (gt_image_keys), not "
                                          "the validation input" % (p["gt_extra"],))
        src, Hs, Ws, mean, std = self._stack_frames(samples, plans, "resize", True, checked=train)
        # crop_1 keeps the left out_w columns of a wider resize; pads are zero rows / columns after it
        dims = np.array([tuple(p["resize"]["src_hw"]) + (p["resize"]["h"], p["resize"]["w"]) for p in plans], np.int32)
        plan = dict(src=src, dims=torch.from_numpy(dims), mean=mean, std=std, out_hw=out_hw, kind="resize")
        if train:
            iplan, fplan = self._colour_rows(plans)
            plan.update(iplan=torch.from_numpy(iplan), fplan=torch.from_numpy(fplan), train=True,
                        mask='patched_mask' in r0.get("gt_keys", []))
            if not plan["mask"] and any(p.get("patched_mask") is not None for p in plans):
                raise ValueError("samples of one batch must carry the same ground-truth images")
        return self._finish(samples, plans, plan, Hs, Ws, "resize", gt=train)

    # -- plans the launches above cannot express: an output window, a padded source, the op list, a Copy split -----
    @staticmethod
    def _op_slots(p):
        """one sample's drawn colour ops as the extended launches' slots [(kind, flags, values)], cut at the Copy:
        -> (slots before the copy, slots after it).  An op whose draw missed is left out; the bare HSV round trip
        stays, because it changes bits."""
        ops, cut = p["ops"], p.get("copy_at", 0)
        before, after = [], []
        for i, (o, v) in enumerate(ops):
            slots = before if i < cut else after
            if o in (OP_BRIGHTNESS, OP_CONTRAST):
                if v is not None:
                    slots.append((o, 0, [v, 0.0, 0.0]))
            elif o == OP_SATURATION:
                hue = ops[i + 1][1] if i + 1 < len(ops) and ops[i + 1][0] == OP_HUE else None
                flags = (1 if v is not None else 0) | (2 if hue is not None else 0)
                slots.append((2, flags, [v if v is not None else 0.0, hue if hue is not None else 0.0, 0.0]))
            elif o == OP_NOISE:
                if v is not None:
                    slots.append((3, 0, [float(v[0]), float(v[1]), float(v[2])]))
        if len(before) + len(after) > MAX_OPS:
            raise NotImplementedError("more than %d drawn colour ops in one sample" % MAX_OPS)
        return before, after

    @classmethod
    def _needs_ext(cls, p):
        if p.get("win") is not None or p.get("src_pad") is not None or _stage(p).get("identity"):
            return True
        kinds = [o for o, _ in p["ops"]]
        if len(kinds) > 3 or len(set(kinds)) != len(kinds) or not set(kinds) <= {OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION}:
            return True
        return len(cls._op_slots(p)[0]) != 0

    def _collate_ext(self, samples, plans):
        B = len(samples)
        warp = plans[0]["warp"] is not None
        stage = "warp" if warp else "resize"
        sizes = set()
        for p in plans:
            if (p["warp"] is not None) != warp:
                raise ValueError("samples of one batch must share the resampling stage")
            if p["hsv"]:
                raise ValueError("pipeline ended in HSV")
            st = p[stage]
            sizes.add((p["win"]["h"], p["win"]["w"]) if p.get("win") is not None else (st["out_h"], st["out_w"]))
        if len(sizes) != 1:
            raise ValueError("samples of one batch must share the output size, got %s" % sorted(sizes))
        out_h, out_w = sizes.pop()
        dims = np.zeros((B, 4), dtype=np.int32)
        win = np.zeros((B, 8), dtype=np.int32)
        minv = np.zeros((B, 6), dtype=np.float64) if warp else None
        slots = [self._op_slots(p) for p in plans]
        split = max(len(b) for b, _ in slots)
        n_ops = split + max(len(a) for _, a in slots)
        if n_ops > MAX_OPS:
            raise NotImplementedError("the batch's colour ops need %d slots around its Copy, the launch has %d" % (
                n_ops, MAX_OPS))
        codes = np.full((B, MAX_OPS), 4, dtype=np.int32)            # 4: nothing
        vals = np.zeros((B, MAX_OPS, 3), dtype=np.float64)
        src, Hs, Ws, mean, std = self._stack_frames(samples, plans, stage, True)
        for b, p in enumerate(plans):
            st = p[stage]
            if warp:
                minv[b] = invert_affine(st["M"])
                dims[b] = (st["src_hw"][0], st["src_hw"][1], 0, 0)
            else:
                dims[b] = (st["src_hw"][0], st["src_hw"][1], st["h"], st["w"])
            w_ = p.get("win")
            if w_ is None:
                w_ = dict(sx=1, ox=0, oy=0, w=out_w, h=out_h, valid=[0, 0, out_w, out_h])
                if p["mirror"]:
                    _win_mirror(w_)
            win[b] = window_row(w_)
            before, after = slots[b]
            for q, (kind, flags, v) in list(enumerate(before)) + [(split + q, o) for q, o in enumerate(after)]:
                codes[b, q] = kind | flags << 4
                vals[b, q] = v
        with_mask = warp or 'patched_mask' in plans[0][stage].get("gt_keys", [])
        if not with_mask and any(p.get("patched_mask") is not None for p in plans):
            raise ValueError("samples of one batch must carry the same ground-truth images")
        plan = dict(src=src, dims=torch.from_numpy(dims), win=torch.from_numpy(win), codes=torch.from_numpy(codes),
                    vals=torch.from_numpy(vals), minv=torch.from_numpy(minv) if warp else None, n_ops=n_ops,
                    split=split, mean=mean, std=std, out_hw=(out_h, out_w), kind="ext", mask=with_mask)
        return self._finish(samples, plans, plan, Hs, Ws, stage)

    @staticmethod
    def _collate_mask(plans, batch, Hs, Ws, stage):
        """the patched masks that are not all ones (_patched_mask): one uint8 [B, Hs, Ws] plane in the frames' padded
        extent, ones for the samples that recorded none.  Nearest indices are clamped to a sample's own extent, so the
        zero padding is never read.  A batch without such a sample carries no plane and uploads nothing extra."""
        if all(p.get("patched_mask") is None for p in plans):
            return
        t = torch.zeros(len(plans), Hs, Ws, dtype=torch.uint8)
        for b, p in enumerate(plans):
            h, w = p[stage]["src_hw"]
            m = p.get("patched_mask")
            t.numpy()[b, :h, :w] = 1 if m is None else m
        batch[PLAN]["mask_src"] = t

    @staticmethod
    def _collate_gt(samples, plans, batch):
        """the extra uint8 ground-truth images of the batch (_extra_gt), zero-padded to one [B, Hs, Ws] per key"""
        keys = list(plans[0].get("gt_extra", []))
        if any(list(p.get("gt_extra", [])) != keys for p in plans):
            raise ValueError("samples of one batch must carry the same ground-truth images")
        gt = {}
        for key in keys:
            # (a Pad2Shape before the resampling stage widens the extent the kernels index, not the sample's array)
            Hs = max(max(s[key].shape[0], _stage(p)["src_hw"][0]) for s, p in zip(samples, plans))
            Ws = max(max(s[key].shape[1], _stage(p)["src_hw"][1]) for s, p in zip(samples, plans))
            t = torch.zeros(len(samples), Hs, Ws, dtype=torch.uint8)
            for b, s in enumerate(samples):
                h, w = s[key].shape
                t.numpy()[b, :h, :w] = s[key]
            gt[key] = t
        batch[PLAN]["gt"] = gt

    def _collate_rest(self, samples, batch):
        skip = {PLAN, self.mask_key} | set(batch[PLAN].get("gt", {}))
        for idx in self.frame_idxs:
            skip.add((self.image_family, idx)); skip.add((self.original_family, idx))
        for key in samples[0]:
            if key in skip:
                continue
            vals = [s[key] for s in samples]
            if isinstance(vals[0], torch.Tensor):
                batch[key] = torch.stack(vals)
            elif isinstance(vals[0], np.ndarray):
                batch[key] = torch.from_numpy(np.stack(vals))
            else:
                batch[key] = vals

    def _collate_warp(self, samples, plans):
        for p in plans:
            if p["warp"] is None:
                raise ValueError("samples of one batch must share the resampling stage")
            if p["hsv"]:
                raise ValueError("pipeline ended in HSV")
        w0 = plans[0]["warp"]
        for p in plans:
            if (p["warp"]["out_w"], p["warp"]["out_h"]) != (w0["out_w"], w0["out_h"]):
                raise ValueError("samples of one batch must share the output size")
        # equal frames fill the buffer completely: no 50 MB memset per batch at the training shape
        src, Hs, Ws, mean, std = self._stack_frames(samples, plans, "warp", False)
        iplan, fplan = self._colour_rows(plans)
        iplan[:, 5:7] = [p["warp"]["src_hw"] for p in plans]
        minv = np.stack([invert_affine(p["warp"]["M"]) for p in plans])
        plan = dict(src=src, minv=torch.from_numpy(minv), iplan=torch.from_numpy(iplan), fplan=torch.from_numpy(fplan),
                    mean=mean, std=std, out_hw=(w0["out_h"], w0["out_w"]), kind="warp")
        return self._finish(samples, plans, plan, Hs, Ws, "warp")

    def collate(self, samples):
        plans = [s[PLAN] for s in samples]
        for s, p in zip(samples, plans):
            if _stage(p) is None:       # a chain without RandomWarpAffine / Resize runs as a resize onto itself
                gt = p.get("gt_keys_seen", [self.mask_key] if self.mask_key in s else [])
                _identity_stage(s, p, [(self.image_family, idx) for idx in self.frame_idxs], gt)
        if any(self._needs_ext(p) for p in plans):
            return self._collate_ext(samples, plans)
        if plans[0].get("resize") is not None:
            return self._collate_resize(samples, plans)
        return self._collate_warp(samples, plans)

    # -- device side -------------------------------------------------------------------------------
    _UPLOADS = ("src", "mask_src", "minv", "iplan", "fplan", "dims", "win", "codes", "vals")

    def materialize(self, batch, device=None):
        from ....hip.binding import lib, check, stream_ptr, FsAugArgs, FsResizeArgs, FsAugExtArgs
        device = torch.device(device or self.device or "cuda")
        plan = batch.pop(PLAN)
        up = {k: plan[k].to(device, non_blocking=True) for k in self._UPLOADS if plan.get(k) is not None}

        def ptr(key):
            return up[key].data_ptr() if key in up else None

        def outputs(args, original, mask):
            """the launch's results, bound to the argument struct (with the mean / std and the sizes every struct has)
            and to the batch's keys"""
            B, F, Hs, Ws, _ = up["src"].shape
            H, W = plan["out_hw"]
            args.B, args.F, args.Hs, args.Ws, args.H, args.W = B, F, Hs, Ws, H, W
            for k in range(3):
                args.mean[k], args.std[k] = float(plan["mean"][k]), float(plan["std"][k])
            image = torch.empty(F, B, 3, H, W, dtype=torch.float32, device=device)
            original = torch.empty(F, B, 3, H, W, dtype=torch.float32, device=device) if original else None
            mask = torch.empty(B, H, W, dtype=torch.float64, device=device) if mask else None
            args.src, args.image = ptr("src"), image.data_ptr()
            args.original = original.data_ptr() if original is not None else None
            args.mask = mask.data_ptr() if mask is not None else None
            for f, idx in enumerate(self.frame_idxs):
                batch[(self.image_family, idx)] = image[f]
                if original is not None:
                    batch[(self.original_family, idx)] = original[f]
            if mask is not None:
                batch[self.mask_key] = mask
            return args

        if plan["kind"] == "ext":
            x = outputs(FsAugExtArgs(), self.original_family, plan["mask"] and self.mask_key)
            x.dims, x.win, x.ops, x.opv, x.minv = ptr("dims"), ptr("win"), ptr("codes"), ptr("vals"), ptr("minv")
            x.mask_src = ptr("mask_src") if x.mask else None
            x.n_ops, x.split = plan["n_ops"], plan["split"]
            if "minv" in up:
                check(lib.fs_augment_frames_ext(C.byref(x), stream_ptr()), "augment_frames_ext")
            else:
                check(lib.fs_resize_frames_ext(C.byref(x), stream_ptr()), "resize_frames_ext")
        elif plan["kind"] == "resize":
            r = outputs(FsResizeArgs(), plan.get("train"), plan.get("train") and plan.get("mask"))
            r.dims, r.iplan, r.fplan = ptr("dims"), ptr("iplan"), ptr("fplan")
            if "mask_src" in up:
                check(lib.fs_resize_frames_masked(C.byref(r), ptr("mask_src"), stream_ptr()), "resize_masked")
            else:
                check(lib.fs_resize_frames(C.byref(r), stream_ptr()), "resize_frames")
        else:
            a = outputs(FsAugArgs(), True, True)
            a.minv, a.iplan, a.fplan = ptr("minv"), ptr("iplan"), ptr("fplan")
            if "mask_src" in up:
                check(lib.fs_augment_frames_masked(C.byref(a), ptr("mask_src"), stream_ptr()), "augment_masked")
            else:
                check(lib.fs_augment_frames(C.byref(a), stream_ptr()), "augment_frames")
        self._materialize_gt(plan, batch, up, device)
        for key, val in list(batch.items()):
            if isinstance(val, torch.Tensor) and not val.is_cuda:
                batch[key] = val.to(device, non_blocking=True)
        return batch

    @staticmethod
    def _materialize_gt(plan, batch, up, device):
        """each extra ground-truth image through the frames' warp / resize and mirror or window: fp32 [B, H, W] on the
        device"""
        if not plan.get("gt"):
            return
        from ....hip import ops
        H, W = plan["out_hw"]
        for key, src in plan["gt"].items():
            src = src.to(device, non_blocking=True)
            if "win" in up:
                batch[key] = ops.augment_masks_ext(src, H, W, up["dims"], up["win"], minv=up.get("minv"))
            else:
                batch[key] = ops.augment_masks(src, H, W, minv=up.get("minv"), dims=up.get("dims"), iplan=up.get("iplan"))

    def __call__(self, samples, device=None):
        return self.materialize(self.collate(samples), device)
