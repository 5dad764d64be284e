"""The Eigen-test side of the tiny KITTI-raw tree of tests/helpers_kitti.py: a split with an index-0 line and both
camera sides, and the depth/%010d.png files KittiDepthMonoEigenTestDataset reads when its config carries depth_path —
shared by tools/gen_golden.py::gen_kitti_eigen_test_dataset (which runs the REAL reference class over it) and the
tests."""
import os

import numpy as np

from tests import helpers_kitti as HK

SPLIT = ((0, "l"), (1, "r"), (3, "l"), (0, "r"), (7, "r"))


def make_eigen_tree(root, seed=5, depth_seed=21, H=HK.H, W=HK.W):
    """-> (raw, split): helpers_kitti.make_tree unchanged, plus <drive>/depth/%010d.png (16-bit greyscale, a quarter
    of the pixels set, written with PIL) and the split above"""
    from PIL import Image
    raw, _ = HK.make_tree(root, seed=seed, H=H, W=W)
    rng = np.random.RandomState(depth_seed)
    d = os.path.join(raw, HK.DATE, HK.DRIVE, "depth")
    os.makedirs(d, exist_ok=True)
    for i in range(HK.NFRAMES):
        depth = rng.randint(256, 80 * 256, size=(H, W)).astype(np.uint16)
        depth[rng.rand(H, W) > 0.25] = 0
        Image.fromarray(depth).save(os.path.join(d, "%010d.png" % i))
    split = os.path.join(root, "eigen_split.txt")
    with open(split, "w") as f:
        for i, side in SPLIT:
            f.write("%s/%s %d %s\n" % (HK.DATE, HK.DRIVE, i, side))
    return raw, split


def eigen_cfg(raw, split, prefix, with_depth):
    """ConvertToFloat + Normalize + ConvertToTensor only, as helpers_kitti.dataset_cfg (no cv2 calls: the reference
    class runs unshimmed but for the PNG reader)"""
    aug = prefix + 'vision_base.data.augmentations.augmentations'
    frames = [('image', 0), ('image', -1)]
    cfg = dict(raw_path=raw, split_file=split,
               augmentation=dict(name=prefix + 'vision_base.utils.builder.Sequential', cfg_list=[
                   dict(name=aug + '.ConvertToFloat'),
                   dict(name=aug + '.Normalize', mean=np.array([0.485, 0.456, 0.406]), stds=np.array([0.229, 0.224, 0.225]),
                        image_keys=frames),
                   dict(name=aug + '.Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]),
                        image_keys=[('original_image', 0)]),
                   dict(name=aug + '.ConvertToTensor')],
                   image_keys=frames + [('original_image', 0)], calib_keys=['P2']))
    if with_depth:
        cfg["depth_path"] = os.path.join(raw, "unused_depth_root")      # only its presence matters (reference :334-340)
    return cfg
