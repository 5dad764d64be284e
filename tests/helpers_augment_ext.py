"""Shared set-up of the extended input-pipeline tests (tests/golden/augment_ext.npz, made by
tools/gen_golden.py::gen_augment_ext from the reference's own classes): the six chains as data, their configs for either
builder, the seeded inputs, and the chains restated in numpy over oracle/augment_oracle.py's functions.

A chain is a list of steps, dict(op=<class name>, **keywords); Shuffle / Sequential steps hold `children`."""
import os

import numpy as np

from oracle import augment_oracle as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_ext.npz")
FRAME_IDXS = [0, 1, -1]
IMGS = [('image', i) for i in FRAME_IDXS]
ORIGS = [('original_image', i) for i in FRAME_IDXS]
POSE_PAIRS = [(("relative_pose", i), 0) for i in FRAME_IDXS[1:]]
SIZES = [(75, 110), (90, 130), (90, 130), (75, 110)]            # two raw sizes: every batch is ragged
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
OUT_H, OUT_W = 16, 48
OURS = 'fsnet_amd.vision_base.data.augmentations.augmentations'
OURS_BUILDER = 'fsnet_amd.vision_base.utils.builder'
CASES = ("a", "b", "c", "d", "e", "f")


def _shuffle(seed):
    return dict(op='Shuffle', image_keys=IMGS, children=[
        dict(op='RandomBrightness', distort_prob=1.0, random_seed=seed),
        dict(op='RandomContrast', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seed + 1),
        dict(op='Sequential', children=[
            dict(op='ConvertColor', transform='HSV'),
            dict(op='RandomSaturation', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seed + 2),
            dict(op='ConvertColor', current='HSV', transform='RGB')])])


def _tail():
    return [dict(op='Normalize', mean=MEAN, stds=STD, image_keys=IMGS),
            dict(op='Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]), image_keys=ORIGS),
            dict(op='ConvertToTensor')]


def _window_steps():
    return [dict(op='Resize', size=(OUT_H, OUT_W), preserve_aspect_ratio=False),
            dict(op='CropTop', crop_top_index=2),
            dict(op='RandomCropToWidth', width=42),
            dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=POSE_PAIRS),
            dict(op='Pad2Shape', target_shape=(17, 45)),
            dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=POSE_PAIRS)]


def case(tag):
    """-> dict(steps, common keywords, build_seed (np.random.seed before the chain is built), out_hw)"""
    both = dict(image_keys=IMGS + ORIGS, calib_keys=['P2'], gt_image_keys=['patched_mask'])
    first = [dict(op='ConvertToFloat')]
    if tag == "a":      # the KITTI chain (configs/kitti_wpose_example:129-155) with its crop_top turned on
        steps = first + [dict(op='CropTop', crop_top_index=11),
                         dict(op='RandomWarpAffine', output_w=OUT_W, output_h=OUT_H, shift_border=20, random_seed=301),
                         dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=POSE_PAIRS), _shuffle(310)] + _tail()
        return dict(steps=steps, common=both, build_seed=1, out_hw=(OUT_H, OUT_W))
    if tag == "b":      # configs/kitti360_fisheye_example:133-159, color_augmented_image_keys = the image keys
        steps = first + [dict(op='Resize', size=(OUT_H, OUT_W), preserve_aspect_ratio=True, force_pad=True),
                         dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=POSE_PAIRS),
                         dict(op='Copy', from_keys=IMGS, to_keys=ORIGS), _shuffle(320)] + _tail()
        return dict(steps=steps, common=dict(both, image_keys=IMGS), build_seed=2, out_hw=(OUT_H, OUT_W))
    if tag == "c":
        return dict(steps=first + _window_steps() + _tail(), common=both, build_seed=3, out_hw=(17, 45))
    if tag == "d":      # no resampling stage
        steps = first + [dict(op='CropTop', output_height=15), dict(op='RandomCropToWidth', width=50),
                         dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=POSE_PAIRS),
                         dict(op='PhotometricDistort', image_keys=IMGS)] + _tail()
        return dict(steps=steps, common=both, build_seed=4, out_hw=(15, 50))
    if tag == "e":      # hue wraps, the f64 tail, a Copy after four ops
        steps = first + [dict(op='RandomWarpAffine', output_w=OUT_W, output_h=OUT_H, shift_border=20, random_seed=351),
                         dict(op='Sequential', image_keys=IMGS, children=[
                             dict(op='RandomBrightness', distort_prob=1.0, random_seed=352),
                             dict(op='Sequential', children=[
                                 dict(op='ConvertColor', transform='HSV'),
                                 dict(op='RandomHue', distort_prob=1.0, delta=180, random_seed=353),
                                 dict(op='RandomSaturation', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=354),
                                 dict(op='ConvertColor', current='HSV', transform='RGB')]),
                             dict(op='RandomEigenvalueNoise', random_seed=355),
                             dict(op='RandomContrast', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=356)]),
                         dict(op='Copy', from_keys=IMGS, to_keys=ORIGS),
                         dict(op='RandomBrightness', distort_prob=1.0, image_keys=IMGS, random_seed=357)] + _tail()
        return dict(steps=steps, common=dict(both, image_keys=IMGS), build_seed=5, out_hw=(OUT_H, OUT_W))
    if tag == "f":      # c's geometry with a holed patched_mask and a uint8 motion_mask
        return dict(steps=first + _window_steps() + _tail(), build_seed=6, out_hw=(17, 45),
                    common=dict(both, gt_image_keys=['patched_mask', 'motion_mask']))
    raise KeyError(tag)


def cfg(steps, common=None, prefix=OURS, builder=OURS_BUILDER):
    """the builder's config of a chain, for the reference's classes or for fsnet_amd's"""
    def one(step):
        step = dict(step)
        op = step.pop('op')
        if 'children' in step:
            return dict(name=builder + '.' + op, cfg_list=[one(c) for c in step.pop('children')], **step)
        return dict(name=prefix + '.' + op, **step)
    return dict(name=builder + '.Sequential', cfg_list=[one(s) for s in steps], **(common or {}))


def sample(tag, n, frame_seed):
    """sample n of a case: uint8 frames of SIZES[n], P2, two relative poses, the ground-truth images"""
    from scipy.spatial.transform import Rotation as R
    H, W = SIZES[n]
    fr = np.random.RandomState(frame_seed + n)
    frames = [fr.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in FRAME_IDXS]
    P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.0027]], dtype=np.float64)
    data = {}
    for i, f in zip(FRAME_IDXS, frames):
        data[('image', i)] = f.copy()
        data[('original_image', i)] = f.copy()
    data['patched_mask'] = np.ones([H, W])
    data['P2'] = P2
    for i in FRAME_IDXS[1:]:
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = R.from_euler('xyz', fr.uniform(-0.05, 0.05, 3)).as_matrix()
        T[:3, 3] = fr.uniform(-1, 1, 3)
        data[('relative_pose', i)] = T
    if tag == "f":
        data['patched_mask'] = np.kron((fr.uniform(size=(H // 5, W // 5)) > 0.3).astype(np.float64), np.ones((5, 5)))
        data['motion_mask'] = np.kron((fr.uniform(size=(H // 5, W // 5)) > 0.5).astype(np.uint8),
                                      np.ones((5, 5), dtype=np.uint8))
    return data


def chw(x):
    """an output image as float32 [3, H, W]: the reference's ConvertToTensor leaves keys it was not given as HWC arrays"""
    x = np.asarray(x)
    return np.ascontiguousarray(x.transpose(2, 0, 1)) if x.ndim == 3 and x.shape[2] == 3 else x


# ---- the chains in numpy, over the oracle's functions ---------------------------------------------------------------
class NumpyChain(object):
    """a chain's steps run on float HWC arrays as the reference's classes run them, every OpenCV call through
    oracle/augment_oracle.py.  Built like the reference's chain: seeded steps own a Generator, unseeded ones take their
    seed from the global stream in construction order.  `log` collects what was drawn in the last call."""

    def __init__(self, steps, common=None):
        self.steps = [self._prepare(dict(common or {}, **s)) for s in steps]
        self.log = {}

    def _prepare(self, step):
        step = dict(step)
        op = step['op']
        if 'children' in step:
            inherit = {k: v for k, v in step.items() if k not in ('op', 'children')}
            step['children'] = [self._prepare(dict(inherit, **c)) for c in step['children']]
        elif op == 'PhotometricDistort':
            keys = dict(image_keys=step['image_keys'])
            mk = lambda name, **kw: self._prepare(dict(op=name, distort_prob=1.0, **keys, **kw))      # noqa: E731
            c1 = mk('RandomContrast', lower=0.5, upper=1.5)
            sat = mk('RandomSaturation', lower=0.5, upper=1.5)
            hue = mk('RandomHue', delta=18.0)
            c2 = mk('RandomContrast', lower=0.5, upper=1.5)
            step['brightness'] = mk('RandomBrightness', delta=32)
            to_hsv, to_rgb = dict(op='ConvertColor', transform='HSV', **keys), dict(op='ConvertColor', transform='RGB', **keys)
            step['transforms'] = [c1, to_hsv, sat, hue, to_rgb, c2]
        elif op in ('RandomWarpAffine', 'RandomBrightness', 'RandomContrast', 'RandomSaturation', 'RandomHue',
                    'RandomEigenvalueNoise'):
            seed = step.get('random_seed')
            step['rng'] = np.random.default_rng(seed if seed is not None else np.random.randint(0, 2**32))
        return step

    def __call__(self, data):
        self.log = dict(mirrors=[], wraps=set(), contrast_first=None)
        for step in self.steps:
            data = self._run(step, data)
        return data

    def _run(self, s, d):
        op = s['op']
        imgs, gts = s.get('image_keys', ['image']), s.get('gt_image_keys', [])
        if op == 'Sequential':
            for c in s['children']:
                d = self._run(c, d)
        elif op == 'Shuffle':
            for k in np.random.permutation(len(s['children'])):
                d = self._run(s['children'][k], d)
        elif op == 'ConvertToFloat':
            for k in imgs:
                d[k] = d[k].astype(np.float32)
        elif op == 'CropTop':
            height = d[imgs[0]].shape[0]
            upper = s['crop_top_index'] if s.get('crop_top_index') is not None else height - s['output_height']
            for k in imgs + gts:
                d[k] = d[k][upper:height]
            P = d['P2']
            P[1, 2] = P[1, 2] - upper
            P[1, 3] = P[1, 3] - upper * P[2, 3]
        elif op == 'RandomCropToWidth':
            width = d[imgs[0]].shape[1]
            left = np.random.randint(0, width - s['width'])
            for k in imgs + gts:
                d[k] = d[k][:, left:left + s['width']]
            P = d['P2']
            P[0, 2] = P[0, 2] - left
            P[0, 3] = P[0, 3] - left * P[2, 3]
        elif op == 'Pad2Shape':
            h, w = d[imgs[0]].shape[:2]
            for k in imgs + gts:
                pads = [(0, s['target_shape'][0] - h), (0, s['target_shape'][1] - w)] + [(0, 0)] * (d[k].ndim - 2)
                d[k] = np.pad(d[k], pads, 'constant')
        elif op == 'RandomMirror':
            width = d[imgs[0]].shape[1]
            drawn = bool(np.random.rand() <= s['mirror_prob'])
            self.log['mirrors'].append(drawn)
            if drawn:
                for k in imgs + gts:
                    d[k] = np.ascontiguousarray(d[k][:, ::-1])
                d['P2'] = A.mirror_P2(d['P2'], width)
                for k, axis in s['pose_axis_pairs']:
                    d[k] = A.flip_relative_pose(d[k], axis)
        elif op == 'Resize':
            shape = d[imgs[0]].shape
            h, w, mode, syx = A.resize_plan(shape, s['size'], s.get('preserve_aspect_ratio', True), s.get('force_pad', True))
            d[('image_resize', 'original_shape')] = np.array([shape[0], shape[1]]).astype(int)
            d[('image_resize', 'effective_size')] = np.array([h, w]).astype(int)
            for k in imgs:
                d[k] = A._crop_pad(A.resize_linear(d[k], w, h), mode, s['size'])
            for k in gts:
                d[k] = A._crop_pad(A.resize_nearest(d[k], w, h), mode, s['size'])
            P = d['P2']
            P[0, :] = P[0, :] * syx[1]
            P[1, :] = P[1, :] * syx[0]
        elif op == 'RandomWarpAffine':
            height, width = d[imgs[0]].shape[:2]
            ow, oh, border, rng = s['output_w'], s['output_h'], s['shift_border'], s['rng']
            scale = max(height, width) * rng.uniform(s.get('scale_lower', 0.6), s.get('scale_upper', 1.4))
            cw = rng.integers(low=border, high=width - border)
            ch = rng.integers(low=border, high=height - border)
            fs = max(ow, oh) / scale
            M = np.array([[fs, 0, ow / 2 - cw * fs], [0, fs, oh / 2 - ch * fs]], dtype=np.float32)
            for k in imgs:
                d[k] = A.warp_affine_linear(d[k], M, ow, oh)
            for k in gts:
                d[k] = A.warp_affine_nearest(d[k], M, ow, oh)
            d['P2'] = A.warp_P2(d['P2'], fs, ow / 2 - cw * fs, oh / 2 - ch * fs)
        elif op == 'RandomBrightness':
            if s['rng'].random() <= s['distort_prob']:
                delta = s['rng'].uniform(-s.get('delta', 32), s.get('delta', 32))
                for k in imgs:
                    d[k] = d[k] + delta
        elif op == 'RandomContrast':
            if s['rng'].random() <= s['distort_prob']:
                alpha = s['rng'].uniform(s.get('lower', 0.5), s.get('upper', 1.5))
                for k in imgs:
                    d[k] = d[k] * alpha
        elif op == 'ConvertColor':
            for k in imgs:
                assert d[k].dtype == np.float32, "cv2.cvtColor takes no float64 image"
                d[k] = A.rgb2hsv(d[k]) if s['transform'] == 'HSV' else A.hsv2rgb(d[k])
        elif op == 'RandomSaturation':
            if s['rng'].random() <= s['distort_prob']:
                ratio = s['rng'].uniform(s.get('lower', 0.5), s.get('upper', 1.5))
                for k in imgs:
                    d[k][:, :, 1] *= ratio
        elif op == 'RandomHue':
            if s['rng'].random() <= s['distort_prob']:
                shift = s['rng'].uniform(-s.get('delta', 18.0), s.get('delta', 18.0))
                for k in imgs:
                    h = d[k][:, :, 0]
                    h += shift
                    if (h > 360.0).any():
                        self.log['wraps'].add('down')
                    h[h > 360.0] -= 360.0
                    if (h < 0.0).any():
                        self.log['wraps'].add('up')
                    h[h < 0.0] += 360.0
        elif op == 'RandomEigenvalueNoise':
            if s['rng'].random() <= s.get('distort_prob', 1.0):
                alpha = s['rng'].normal(scale=s.get('alphastd', 0.1), size=(3, ))
                vec = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                                [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
                val = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
                noise = np.dot(vec, val * alpha) * 255
                for k in imgs:
                    d[k] = d[k] + noise
        elif op == 'PhotometricDistort':
            first = bool(np.random.rand() <= 0.5)
            self.log['contrast_first'] = first
            for c in [s['brightness']] + (s['transforms'][:-1] if first else s['transforms'][1:]):
                d = self._run(c, d)
        elif op == 'Copy':
            for a, b in zip(s['from_keys'], s['to_keys']):
                d[b] = d[a].copy()
        elif op == 'Normalize':
            for k in imgs:
                d[k] = A.normalize(d[k], s['mean'], s['stds'])
        elif op == 'ConvertToTensor':
            pass
        else:
            raise KeyError(op)
        return d
