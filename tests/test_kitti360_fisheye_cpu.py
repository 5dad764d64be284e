"""KITTI-360 fisheye reader mirror (fsnet_amd/monodepth/data/datasets/fisheye_dataset.py) against the REAL reference
class run over the same seeded tree (tests/golden/kitti360_fisheye.npz, tools/gen_golden.py::gen_kitti360_fisheye),
the helper's numpy ground truth against the reference's _precompute, the fixture's two conditions, and the
device_errors hook surface of both evaluators.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import helpers_kitti360 as HK

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kitti360_fisheye.npz")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HK.make_tree(str(tmp_path_factory.mktemp("kitti360")))


def _scan(raw, i):
    from fsnet_amd.monodepth.data.datasets.utils import read_pc_from_bin
    return read_pc_from_bin(os.path.join(raw, "data_3d_raw", HK.SEQ, "velodyne_points/data", "%010d.bin" % i))


def _left(raw):
    from fsnet_amd.monodepth.data.datasets.fisheye_dataset import extract_P_from_fisheye_calib, read_fisheycalib
    calib_dir = os.path.join(raw, "calibration")
    lc = read_fisheycalib(os.path.join(calib_dir, "image_02.yaml"))
    return extract_P_from_fisheye_calib(lc), lc, HK.velo_to_cam02(calib_dir)


def test_readers_parse_the_tree(tree):
    from fsnet_amd.monodepth.data.datasets import fisheye_dataset as FD
    from fsnet_amd.monodepth.data.datasets.utils import cam_relative_pose_nusc
    raw, train, val, mask_path = tree
    calib_dir = os.path.join(raw, "calibration")
    P, calib = HK.mei_calib(0)
    lc = FD.read_fisheycalib(os.path.join(calib_dir, "image_02.yaml"))
    assert lc["mirror_parameters"]["xi"] == calib["mirror_parameters"]["xi"]
    assert lc["distortion_parameters"]["k2"] == calib["distortion_parameters"]["k2"]
    P0 = FD.extract_P_from_fisheye_calib(lc)
    assert P0.dtype == np.float64 and P0.shape == (3, 4) and P0[2, 2] == 1 and P0[0, 1] == 0 and P0[2, 3] == 0
    assert np.array_equal(P0[:2, :3].astype(np.float32), P[:2, :3]) and P0[0, 0] == float(P[0, 0])
    T00, T01, T02, T03, T_cam2velo = HK.extrinsics()
    ext = FD.read_extrinsic_from_sequence(os.path.join(calib_dir, "calib_cam_to_pose.txt"))
    for k, T in zip(("T_image0", "T_image1", "T_image2", "T_image3"), (T00, T01, T02, T03)):
        assert np.array_equal(ext[k], T), k
    assert np.array_equal(FD.read_cam2velo_from_sequence(os.path.join(calib_dir, "calib_cam_to_velo.txt")), T_cam2velo)
    frames, poses = FD.read_poses_file(os.path.join(raw, "data_poses", HK.SEQ, "poses.txt"))
    assert frames == list(range(100, 100 + HK.NFRAMES + 2)) and poses.shape == (HK.NFRAMES + 2, 4, 4)
    assert np.array_equal(poses[:, 3], np.tile([0, 0, 0, 1.0], (HK.NFRAMES + 2, 1)))
    scan = _scan(raw, HK.EVAL_FRAMES[0])
    assert scan.dtype == np.float32 and scan.shape == (20000, 4)
    A, B = np.eye(4), np.eye(4)
    B[0, 3] = 1.0
    assert np.allclose(cam_relative_pose_nusc(A, B, np.eye(4))[0, 3], -1.0)
    with open(os.path.join(os.path.dirname(train), "k.txt"), "w") as f:
        f.write("2011_09_26/2011_09_26_drive_0022_sync 473 r\n")
    assert FD.read_split_file(os.path.join(os.path.dirname(train), "k.txt"))[0] == dict(
        folder="2011_09_26/2011_09_26_drive_0022_sync", index=473, side="r", datetime="2011_09_26")


@pytest.mark.parametrize("tag", ["static_left", "all_left", "static_right"])
def test_dataset_matches_reference_class(tree, tag):
    from fsnet_amd.monodepth.data.datasets.fisheye_dataset import KITTI360FisheyeDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    g = np.load(GOLD)
    raw, train, val, mask_path = tree
    kw = dict(static_left=dict(is_filter_static=True, use_right_image=False),
              all_left=dict(is_filter_static=False, use_right_image=False),
              static_right=dict(is_filter_static=True, use_right_image=True, fisheye_mask=mask_path))[tag]
    ds = KITTI360FisheyeDataset(**HK.dataset_cfg(raw, train, prefix='fsnet_amd.', **kw))
    assert ds.frame_ids == [0, -1, 1] and ds.is_motion_mask is False
    assert np.array_equal(np.array([o["img_indexes"] + o["pose_indexes"] for o in ds.imdb], np.int64), g[tag + "_index"])
    if tag == "static_right":
        np.random.seed(3)
    sides = set()
    for i in range(len(ds)):
        smp = ds[i]
        k = "%s_s%d_" % (tag, i)
        assert PLAN in smp
        for f in (0, -1, 1):
            frame = smp[("image", f)]
            assert frame.dtype == np.uint8 and frame.shape == (HK.H, HK.W, 3)
            assert hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest() == str(g[k + "image_%d" % f])
        for key, f in (("pose_m", -1), ("pose_p", 1)):
            pose = np.asarray(smp[("relative_pose", f)])
            assert pose.dtype == np.float32 and np.abs(pose - g[k + key]).max() <= 1e-12
        assert np.array_equal(np.asarray(smp["P2"]), g[k + "P2"])
        assert np.array_equal(np.asarray(smp["original_P2"]), g[k + "original_P2"])
        assert smp["calib_meta"] == json.loads(str(g[k + "calib_meta"]))
        sides.add(smp["calib_meta"]["mirror_parameters"]["xi"])
        pm = smp["patched_mask"]
        assert pm.dtype == np.float64 and np.array_equal(pm, g[k + "patched_mask"].astype(np.float64))
    assert len(sides) == (2 if tag == "static_right" else 1)       # seeded draws pick both cameras


def test_helper_ground_truth_equals_reference(tree):
    g = np.load(GOLD)
    raw = tree[0]
    P0, lc, T = _left(raw)
    assert int(g["n_gt"]) == len(HK.EVAL_FRAMES)
    for j, i in enumerate(HK.EVAL_FRAMES):
        depth, mask = HK.ground_truth(_scan(raw, i), T, P0, lc)
        want_d, want_m = HK.dense(g["gt%d_idx" % j], g["gt%d_val" % j], g["gt%d_midx" % j])
        assert np.array_equal(depth, want_d) and np.array_equal(mask, want_m)
        assert mask.sum() > 1000 and (depth > 0).sum() > 5000


def test_fixture_conditions(tree):
    """every point with z > 0 projects inside the image; no two points share the reference's float sub2ind value"""
    raw = tree[0]
    P0, lc, T = _left(raw)
    for i in HK.EVAL_FRAMES:
        velo = _scan(raw, i)
        u, v, z, _ = HK.gt_points(velo, T, P0, lc)
        assert len(u) < len(velo)                               # some points lie behind the camera
        assert ((u >= 0) & (u < HK.W) & (v >= 0) & (v < HK.H)).all()
        assert HK.float_sub2ind_unique(velo, T, P0, lc)


def test_concat_dataset_builds_the_reader(tree):
    from fsnet_amd.vision_base.data.datasets.dataset_utils import ConcatDataset
    raw, train, val, _ = tree
    cfg = HK.dataset_cfg(raw, train, prefix='fsnet_amd.', use_right_image=False)
    child = dict(name="fsnet_amd.monodepth.data.datasets.fisheye_dataset.KITTI360FisheyeDataset", split_file=train)
    ds = ConcatDataset([child, dict(child, is_filter_static=False)],
                       **{k: v for k, v in cfg.items() if k != "split_file"})
    assert len(ds) == 8 + 10
    assert ds[9]["P2"].shape == (3, 4)


def test_device_errors_hook_path():
    import inspect
    from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import KittiEigenEvaluator
    from fsnet_amd.monodepth.evaluation.kitti360_fisheye_eval import Kitti360FisheyeEvaluator
    from fsnet_amd.monodepth.pipeline_hooks.evaluation_hooks import base_evaluation_hooks as BH
    for cls in (KittiEigenEvaluator, Kitti360FisheyeEvaluator):
        assert list(inspect.signature(cls.device_errors).parameters) == ["self", "depth_0", "index"]
    assert Kitti360FisheyeEvaluator.device_errors is not KittiEigenEvaluator.device_errors
    for hook in (BH.KittiEvaluationHook, BH.KittiEvaluationHook_postopt):
        src = inspect.getsource(hook.__call__)
        assert "device_errors(" in src and "ops.depth_eval(" not in src
    ev = Kitti360FisheyeEvaluator(gt_depths=[np.zeros((4, 5), np.float32)])
    assert ev.close_masks[0].dtype == bool and ev.close_masks[0].all()
    with pytest.raises(ValueError):
        Kitti360FisheyeEvaluator()


@pytest.mark.parametrize("name", ["lidar_mei.hip", "eval.hip"])
def test_new_kernels_do_not_spill(name):
    """the check of tests/test_no_spills_cpu.py on the files of fs_lidar_mei_depth and fs_depth_eval_masked"""
    from tests.test_no_spills_cpu import test_no_scratch
    test_no_scratch(name)
