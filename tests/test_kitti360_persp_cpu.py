"""KITTI-360 perspective reader mirror (fsnet_amd/monodepth/data/datasets/kitti360_dataset.py) against the REAL
reference class run over the same seeded tree (tests/golden/kitti360_persp.npz,
tools/gen_golden.py::gen_kitti360_persp), the host mirror of the ground-truth export (monodepth_utils.project_depth_map)
against the reference's _precompute, the two shipped KITTI-360 configs building their datasets over the tree, and a
ConcatDataset of the KITTI and the KITTI-360 readers.  CPU only."""
import os

import numpy as np
import pytest

from tests import helpers_kitti360 as HK
from tests import helpers_kitti360_persp as HP

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kitti360_persp.npz")
REF = "/root/reference"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HP.make_tree(str(tmp_path_factory.mktemp("kitti360p")))


def _png(raw, cam, i):
    from PIL import Image
    return np.array(Image.open(os.path.join(raw, "data_2d_raw", HP.SEQ, cam, "data_rect", "%010d.png" % i)))


def test_readers_parse_the_tree(tree):
    from fsnet_amd.monodepth.data.datasets import kitti360_dataset as KD
    raw = tree[0]
    calib_dir = os.path.join(raw, "calibration")
    P0, P1, R0, R1 = HP.perspective()
    p0, p1, r0, r1 = KD.read_P01_from_sequence(os.path.join(calib_dir, "perspective.txt"))
    assert p0.shape == (3, 4) and p0.dtype == np.float64 and np.array_equal(p0, P0) and np.array_equal(p1, P1)
    for r, R in ((r0, R0), (r1, R1)):
        assert r.shape == (4, 4) and np.array_equal(r[:3, :3], R) and np.array_equal(r[3], [0, 0, 0, 1.0])
        assert np.array_equal(r[:3, 3], [0, 0, 0]) and not np.array_equal(R, np.eye(3))
    T00, T01, _, _, T_cam2velo = HK.extrinsics()
    ext = KD.read_extrinsic_from_sequence(os.path.join(calib_dir, "calib_cam_to_pose.txt"))
    assert isinstance(ext, tuple) and len(ext) == 2                      # not the fisheye module's dict
    assert np.array_equal(ext[0], T00) and np.array_equal(ext[1], T01)
    assert np.array_equal(KD.read_T_from_sequence(os.path.join(calib_dir, "calib_cam_to_velo.txt")), T_cam2velo)
    frames, poses = KD.read_poses_file(os.path.join(raw, "data_poses", HP.SEQ, "poses.txt"))
    assert frames == list(range(100, 100 + HP.NFRAMES + 2)) and poses.shape == (HP.NFRAMES + 2, 4, 4)
    with open(os.path.join(calib_dir, "only_p0.txt"), "w") as f:
        f.write("P_rect_00: " + " ".join(["1.0"] * 12) + "\n")
    with pytest.raises(AssertionError):
        KD.read_P01_from_sequence(os.path.join(calib_dir, "only_p0.txt"))


def test_calibration_is_composed_like_the_reference(tree):
    from fsnet_amd.monodepth.data.datasets.kitti360_dataset import KITTI360MonoDataset
    raw, train, _ = tree
    ds = KITTI360MonoDataset(**HP.dataset_cfg(raw, train, prefix='fsnet_amd.', is_filter_static=False))
    P0, P1, R0, R1 = HP.perspective()
    T00, T01 = HK.extrinsics()[:2]
    for key, R, T in (('T_rect02baselink', R0, T00), ('T_rect12baselink', R1, T01)):
        R4 = np.eye(4)
        R4[:3, :3] = R
        assert np.array_equal(ds.cam_calib[key], R4 @ T)
    assert np.array_equal(ds.cam_calib['P0'], P0) and np.array_equal(ds.cam_calib['P1'], P1)


@pytest.mark.parametrize("tag", ["static_left", "all_left", "static_right"])
def test_dataset_matches_reference_class(tree, tag):
    from fsnet_amd.monodepth.data.datasets.kitti360_dataset import KITTI360MonoDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    g = np.load(GOLD)
    raw, train, _ = tree
    kw = dict(static_left=dict(is_filter_static=True, use_right_image=False),
              all_left=dict(is_filter_static=False, use_right_image=False),
              static_right=dict(is_filter_static=True, use_right_image=True))[tag]
    ds = KITTI360MonoDataset(**HP.dataset_cfg(raw, train, prefix='fsnet_amd.', **kw))
    assert ds.frame_ids == [0, -1, 1] and ds.is_motion_mask is False
    index = np.array([o["img_indexes"] + o["pose_indexes"] for o in ds.imdb], np.int64)
    assert len(ds) == len(g[tag + "_index"]) and np.array_equal(index, g[tag + "_index"])
    if tag == "static_right":
        np.random.seed(HP.GOLDEN_DRAW_SEED)
    P = HP.perspective()[:2]
    cams = []
    for i in range(len(ds)):
        smp = ds[i]
        k = "%s_s%d_" % (tag, i)
        assert PLAN in smp
        cam = int(g[tag + "_cam"][i])
        for f, img_index in zip(ds.frame_ids, ds.imdb[i]["img_indexes"]):
            frame = smp[("image", f)]
            assert frame.dtype == np.uint8 and frame.shape == (HP.H, HP.W, 3)
            assert np.array_equal(frame, _png(raw, "image_0%d" % cam, img_index)), (i, f, cam)
        cams.append(cam)
        for key, f in (("pose_m", -1), ("pose_p", 1)):
            pose = np.asarray(smp[("relative_pose", f)])
            assert pose.dtype == np.float32 and np.array_equal(pose, g[k + key]), (i, f)
        assert np.array_equal(np.asarray(smp["P2"]), g[k + "P2"])
        assert np.array_equal(np.asarray(smp["original_P2"]), g[k + "original_P2"])
        assert np.array_equal(np.asarray(smp["original_P2"])[:, :3], P[cam][:, :3].astype(np.float32))
        assert not np.asarray(smp["original_P2"])[:, 3].any()               # the baseline column is not carried
        pm = np.asarray(smp["patched_mask"])
        assert pm.shape == (HP.H, HP.W) and (pm == 1).all()
    assert len(set(cams)) == (2 if tag == "static_right" else 1)           # the seeded draws pick both cameras


def test_host_mirror_equals_reference_ground_truth(tree):
    from fsnet_amd.monodepth.networks.utils.monodepth_utils import project_depth_map
    g = np.load(GOLD)
    raw = tree[0]
    P = HP.velo_to_image(raw)
    assert int(g["n_gt"]) == len(HP.EVAL_FRAMES)
    for j, i in enumerate(HP.EVAL_FRAMES):
        scan = HP.scan(raw, i)
        before = scan.copy()
        depth = project_depth_map(scan, P, np.array([HP.H, HP.W]))
        assert np.array_equal(scan, before)                                 # the caller's scan is not written to
        want = HP.dense(g["gt%d_idx" % j], g["gt%d_val" % j])
        assert depth.dtype == np.float64 and depth.shape == (HP.H, HP.W)
        assert int((depth.astype(np.float32) != want).sum()) == 0
        dup, pairs = HP.fixture_counts(scan, P)
        assert dup >= 1000 and pairs >= 1


def test_host_mirror_keeps_the_edge_pair_quirk():
    """three points by hand on a 3 x 4 image: (0, 3) then (1, 0) then (0, 3) share the export index; the first one's
    pixel takes the minimum of all three, the partner pixel keeps its own (last) value"""
    from fsnet_amd.monodepth.networks.utils.monodepth_utils import project_depth_map
    P = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])         # u = x, v = y (p2 = 1)
    velo = np.array([[4, 1, 0, 0.5], [1, 2, 0, 0.5], [4, 1, 0, 0.5], [3, 3, 0, 0.5], [3, 3, 0, 0.5]], np.float32)
    depth = project_depth_map(velo, P, np.array([3, 4]))
    want = np.zeros((3, 4))
    want[0, 3], want[1, 0], want[2, 2] = 1.0, 1.0, 3.0
    assert np.array_equal(depth, want)
    velo = velo[[1, 0, 2, 3]]                                               # the partner's point first
    depth = project_depth_map(velo, P, np.array([3, 4]))
    want[0, 3], want[1, 0] = 4.0, 1.0
    assert np.array_equal(depth, want)
    assert not project_depth_map(np.zeros((0, 4), np.float32), P, np.array([3, 4])).any()


def test_evaluator_surface():
    import inspect
    from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import Kitti360Evaluator, KittiEigenEvaluator
    assert issubclass(Kitti360Evaluator, KittiEigenEvaluator)
    for name in ("_single_loss", "single_call", "device_errors", "log"):       # the metric is the parent's
        assert getattr(Kitti360Evaluator, name) is getattr(KittiEigenEvaluator, name)
    assert Kitti360Evaluator._precompute is not KittiEigenEvaluator._precompute
    assert list(inspect.signature(Kitti360Evaluator.__init__).parameters)[1:4] == ["data_path", "split_file",
                                                                                  "gt_saved_file"]
    ev = Kitti360Evaluator(gt_depths=[np.zeros((4, 5), np.float32)])
    assert ev.group_size == 8
    with pytest.raises(ValueError):
        Kitti360Evaluator()


def test_evaluator_composes_the_projection_like_the_reference(tree):
    from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import Kitti360Evaluator
    raw = tree[0]
    ev = Kitti360Evaluator(gt_depths=[np.zeros((2, 2), np.float32)])
    ev._load_calib(os.path.join(raw, "calibration"))
    assert set(ev.cam_calib) == {"P0", "R0", "T_cam2velo"}
    assert np.array_equal(ev.velo_to_image(), HP.velo_to_image(raw))


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from fsnet_amd.hip import binding, lib
    assert binding.ABI_VERSION == 15 and lib.fs_abi_version() == 15
    assert lib.fs_lidar_pinhole_depth_workspace_bytes(2, 94, 310) == 2 * 94 * 310 * 16
    assert lib.fs_lidar_pinhole_depth_workspace_bytes(1, 5, 1) == -1          # W = 1: every pixel shares one index
    assert lib.fs_lidar_pinhole_depth_workspace_bytes(0, 5, 5) == -1
    assert lib.fs_lidar_pinhole_depth(None, None, 0, None, 1, 4, 4, None, None, 0, None) == 1      # FS_EINVAL


def test_new_kernels_do_not_spill():
    from tests.test_no_spills_cpu import test_no_scratch
    test_no_scratch("lidar_pinhole.hip")


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("name", ["kitti360_wpose_example", "distill_kitti360_example"])
def test_shipped_configs_build_their_datasets(tree, tmp_path, name):
    """the reference's own config files, repointed as tests/test_reference_configs_cpu.py repoints them, with the
    KITTI-360 path and the split files set to the synthetic tree: both dataset sections build and yield samples"""
    from tests.test_reference_configs_cpu import _load_cfg
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    from fsnet_amd.vision_base.utils.builder import build
    raw, train, val = tree
    cfg = _load_cfg(tmp_path, name)
    assert cfg.trainer.evaluate_hook.dataset_eval_cfg.name.endswith("kitti_unsupervised_eval.Kitti360Evaluator")
    cfg.path.kitti360_path = raw
    child = cfg.train_dataset.cfg_list[0]
    assert child.name == "fsnet_amd.monodepth.data.datasets.kitti360_dataset.KITTI360MonoDataset"
    child.raw_path, child.split_file = raw, train
    cfg.val_dataset.raw_path, cfg.val_dataset.split_file = raw, val
    # RandomWarpAffine draws its centre from [shift_border, size - shift_border): the default of 128 px, meant for
    # 376 x 1408 frames, leaves no centre in a 94 x 310 one (in the reference too)
    warp = cfg.train_dataset.augmentation.cfg_list[1]
    assert warp.name.endswith(".RandomWarpAffine")
    warp.shift_border = 16
    np.random.seed(0)
    ds = build(**cfg.train_dataset)
    assert len(ds) == 8                                                        # 10 split lines, two filtered as static
    smp = ds[3]
    assert PLAN in smp and smp[("image", 0)].dtype == np.uint8 and smp[("image", 0)].shape == (HP.H, HP.W, 3)
    assert {("relative_pose", 1), ("relative_pose", -1), "P2", "original_P2", "patched_mask"} <= set(smp)
    vs = build(**cfg.val_dataset)
    assert type(vs).__name__ == "KITTI360MonoDataset" and len(vs) == len(HP.EVAL_FRAMES)
    smp = vs[0]
    assert np.array_equal(smp[("image", 0)], _png(raw, "image_00", HP.EVAL_FRAMES[0]))
    dev_cfg = dict(cfg.trainer.evaluate_hook.dataset_eval_cfg)
    assert build(gt_depths=[np.zeros((3, 3), np.float32)], **{k: v for k, v in dev_cfg.items()
                                                             if k in ("name", "is_evaluate_absolute")}) is not None


def test_concat_of_kitti_and_kitti360(tree, tmp_path):
    from tests import helpers_kitti as HKI
    from fsnet_amd.vision_base.data.datasets.dataset_utils import ConcatDataset
    raw360, train360, _ = tree
    raw, split = HKI.make_tree(str(tmp_path))
    cfg = HKI.dataset_cfg(raw, split, prefix='fsnet_amd.')
    common = {k: v for k, v in cfg.items() if k not in ("raw_path", "split_file")}
    kitti = dict(name="fsnet_amd.monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset", raw_path=raw,
                 split_file=split)
    k360 = dict(name="fsnet_amd.monodepth.data.datasets.kitti360_dataset.KITTI360MonoDataset", raw_path=raw360,
                split_file=train360, frame_ids=[0, 1, -1])
    n_kitti = len(ConcatDataset([kitti], **common))
    ds = ConcatDataset([kitti, k360], **common)
    assert n_kitti > 0 and len(ds) == n_kitti + 8
    np.random.seed(2)
    a, b = ds[0], ds[n_kitti + 2]
    assert a[("image", 0)].shape[:2] == (HKI.H, HKI.W) and b[("image", 0)].shape[:2] == (HP.H, HP.W)
    assert set(a) == set(b)
