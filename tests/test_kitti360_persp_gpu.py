"""KITTI-360 perspective evaluation on the device: fs_lidar_pinhole_depth against the REAL reference's ground truth
(tests/golden/kitti360_persp.npz), against the KITTI export's golden (tests/golden/velo_gt.npz) and against the host
mirror on random clouds; its determinism and graph capture; Kitti360Evaluator's cached-file round trip and metric; the
evaluation hook and one training step of kitti360_wpose_example's meta-arch fed from the mirrored dataset."""
import os

import numpy as np
import pytest
import torch

from tests import helpers_kitti360 as HK
from tests import helpers_kitti360_persp as HP

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "kitti360_persp.npz")
VELO_GOLD = os.path.join(os.path.dirname(__file__), "golden", "velo_gt.npz")
NEAR = 1e-9
MAX_EXPLAINED = 2


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HP.make_tree(str(tmp_path_factory.mktemp("kitti360p")))


def _scans(raw):
    return [HP.scan(raw, i) for i in HP.EVAL_FRAMES]


def _partner(py, px, H, W):
    """the one other pixel that shares (py, px)'s export index row * (W - 1) + col - 1, or None"""
    if px == W - 1 and py + 1 < H:
        return py + 1, 0
    if px == 0 and py > 0:
        return py - 1, W - 1
    return None


def _explained(scan, P, pix, H, W):
    """a mismatch at flat pixel `pix` is explained when a point that lands on the pixel or on its partner pixel, or on
    a pixel next to one of them, has u or v within NEAR of a half-integer: only there can the last ulp of the f64
    product (numpy's matrix product against the kernel's index-order sums) move a point to another pixel"""
    u, v, row, col, _ = HP.pixel_points(scan, P)
    near_half = (np.abs(u - np.floor(u) - 0.5) < NEAR) | (np.abs(v - np.floor(v) - 0.5) < NEAR)
    py, px = divmod(int(pix), W)
    cells = [(py, px)] + ([_partner(py, px, H, W)] if _partner(py, px, H, W) else [])
    around = np.zeros(len(u), bool)
    for cy, cx in cells:
        around |= (np.abs(row - cy) <= 1) & (np.abs(col - cx) <= 1)
    return bool(np.any(around & near_half))


def _compare(got, want, scan, P, tag):
    """exact values (copies of float32 x); every differing pixel explained, at most MAX_EXPLAINED of them"""
    H, W = want.shape
    assert got.dtype == np.float32 and got.shape == want.shape
    diff = np.flatnonzero((got != want).reshape(-1))
    print("%s: %d pixels hit, %d differ" % (tag, int((want > 0).sum()), len(diff)))
    for pix in diff:
        assert _explained(scan, P, pix, H, W), "%s: pixel %d unexplained (%r != %r)" % (
            tag, pix, got.reshape(-1)[pix], want.reshape(-1)[pix])
    assert len(diff) <= MAX_EXPLAINED, (tag, len(diff))


def test_kernel_matches_reference_golden(dev, tree):
    from fsnet_amd.hip import ops
    g = np.load(GOLD)
    raw = tree[0]
    scans, P = _scans(raw), HP.velo_to_image(raw)
    G = len(scans)
    depth = ops.lidar_pinhole_depth(scans, np.stack([P] * G), HP.H, HP.W, dev).cpu().numpy()
    for j in range(G):
        want = HP.dense(g["gt%d_idx" % j], g["gt%d_val" % j])
        dup, pairs = HP.fixture_counts(scans[j], P)
        assert dup >= 1000 and pairs >= 1 and (want > 0).sum() > 5000
        _compare(depth[j], want, scans[j], P, "frame %d" % j)


def test_kernel_matches_kitti_export_golden(dev, tmp_path):
    """the device form of generate_depth_map(cam=2, vel_depth=True) over the KITTI tree: 50-95 % of the pixels hit, so
    duplicates and the edge-pair quirk decide most of the map"""
    from tests import helpers_kitti as HK
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.networks.utils.monodepth_utils import load_velodyne_points, read_calib_file
    raw, split = HK.make_tree(str(tmp_path))
    HK.add_velodyne(raw)
    gt = np.load(VELO_GOLD)["gt"].astype(np.float32)
    lines = [l.split() for l in open(split)]
    assert len(lines) == gt.shape[0]
    calib_dir = os.path.join(raw, lines[0][0].split("/")[0])
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    v2c = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    velo2cam = np.vstack((np.hstack((v2c["R"].reshape(3, 3), v2c["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    P = np.dot(np.dot(cam2cam["P_rect_02"].reshape(3, 4), R_cam2rect), velo2cam)
    H, W = (int(v) for v in cam2cam["S_rect_02"][::-1])
    assert (H, W) == gt.shape[1:]
    scans = [load_velodyne_points(os.path.join(raw, folder, "velodyne_points/data", "%010d.bin" % int(frame_id)))
             for folder, frame_id, _ in lines]
    depth = ops.lidar_pinhole_depth(scans, np.stack([P] * len(scans)), H, W, dev).cpu().numpy()
    assert 0.5 < float((gt > 0).mean()) < 0.95
    for k in range(len(scans)):
        _compare(depth[k], gt[k], scans[k], P, "kitti frame %d" % k)


def _cloud(rng, P, H, W, n):
    """n points drawn in the image (a margin outside included) at depths 2-60 m and carried back to the velodyne frame
    through the pseudo-inverse of P's camera part; plus points with x == 0 (both zeros), points behind the camera
    (projected z <= 0, x >= 0), points with x < 0, the origin (projected z = P[2, 3]) and far outliers"""
    M = np.vstack([P, [0, 0, 0, 1.0]])
    u, v, z = rng.uniform(-3, W + 4, n), rng.uniform(-3, H + 4, n), rng.uniform(2, 60, n)
    img = np.stack([u * z, v * z, z, np.ones(n)], 1)
    pts = np.linalg.solve(M, img.T).T.astype(np.float32)
    extra = rng.uniform(-1, 1, (n // 4, 4)).astype(np.float32) * np.array([3, 60, 8, 1], np.float32)
    extra[: n // 16, 0] = 0.0
    extra[n // 16: n // 12, 0] = -0.0
    extra[n // 12: n // 8, 0] = np.abs(extra[n // 12: n // 8, 0])
    pts = np.concatenate([pts, extra, np.zeros((3, 4), np.float32)])
    pts = pts[rng.permutation(len(pts))]
    pts[:, 3] = rng.uniform(0, 1, len(pts))
    return np.ascontiguousarray(pts)


@pytest.mark.parametrize("shape", [(13, 17), (64, 9), (9, 2)])
def test_kernel_matches_host_mirror_on_random_clouds(dev, shape):
    """narrow images with thousands of points: most groups are edge pairs.  Values compare as numbers, so the host's
    -0.0 (a point with x = -0.0 that survives) equals the kernel's +0.0."""
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.networks.utils.monodepth_utils import project_depth_map
    H, W = shape
    rng = np.random.RandomState(100 * H + W)
    c, s = np.cos(0.5), np.sin(0.5)
    # velodyne (x forward, y left, z up) -> camera (x right, y down, z forward), yawed by 0.5 rad: points with x >= 0
    # far to one side lie behind the image plane
    R = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    scans, Ps = [], []
    for k, t3 in enumerate((0.002, 0.0, 0.3)):
        K = np.array([[7.0 + k, 0, W / 2.0, 0.3], [0, 6.5, H / 2.0, 0.1], [0, 0, 1, t3]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, (0.05, -0.1, 0.0)
        P = K @ T
        Ps.append(P)
        scans.append(_cloud(rng, P, H, W, 4000 + 1000 * k))
    scans.insert(1, np.zeros((0, 4), np.float32))                       # an empty scan inside the group
    Ps.insert(1, Ps[0])
    depth = ops.lidar_pinhole_depth(scans, np.stack(Ps), H, W, dev).cpu().numpy()
    assert not depth[1].any()
    pairs = 0
    for k, (scan, P) in enumerate(zip(scans, Ps)):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = project_depth_map(scan, P, np.array([H, W])).astype(np.float32)
        _compare(depth[k], want, scan, P, "%dx%d cloud %d" % (H, W, k))
        if len(scan):
            assert (want > 0).mean() > 0.5
            pairs += HP.fixture_counts(scan, P, H, W)[1]
    assert pairs >= (H - 1)                                              # the edge pairs were exercised
    all_behind = scans[0].copy()
    all_behind[:, 0] = -np.abs(all_behind[:, 0]) - 1e-3
    assert not ops.lidar_pinhole_depth([all_behind], Ps[0][None], H, W, dev).any()


def test_kernel_edge_pair_by_hand(dev):
    from fsnet_amd.hip import ops
    P = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])         # u = x, v = y
    velo = np.array([[4, 1, 0, 0.5], [1, 2, 0, 0.5], [4, 1, 0, 0.5], [3, 3, 0, 0.5], [3, 3, 0, 0.5]], np.float32)
    want = np.zeros((2, 3, 4), np.float32)
    want[0, 0, 3], want[0, 1, 0], want[0, 2, 2] = 1.0, 1.0, 3.0
    want[1, 0, 3], want[1, 1, 0], want[1, 2, 2] = 4.0, 1.0, 3.0
    got = ops.lidar_pinhole_depth([velo, velo[[1, 0, 2, 3]]], np.stack([P, P]), 3, 4, dev).cpu().numpy()
    assert np.array_equal(got, want)
    # half to even: u = 2.5 -> 2 -> column 1, u = 3.5 -> 4 -> column 3
    velo = np.array([[2.5, 1, 0, 0], [3.5, 1, 0, 0]], np.float32)
    got = ops.lidar_pinhole_depth([velo], P[None], 3, 4, dev).cpu().numpy()[0]
    assert got[0, 1] == 2.5 and got[0, 3] == 3.5 and np.count_nonzero(got) == 2
    with pytest.raises(ValueError):
        ops.LidarPinholeDepth(1, 5, 1, dev)


def test_ground_truth_deterministic_and_capturable(dev, tree):
    from fsnet_amd.hip import ops
    raw = tree[0]
    scans, P = _scans(raw), HP.velo_to_image(raw)
    G = len(scans)
    Ps = np.stack([P * (1.0 + 0.01 * k) for k in range(G)])                  # a matrix of its own per frame
    a = ops.lidar_pinhole_depth(scans, Ps, HP.H, HP.W, dev).clone()
    b = ops.lidar_pinhole_depth(scans, Ps, HP.H, HP.W, dev).clone()
    d1 = torch.cat([ops.lidar_pinhole_depth([s], Ps[k:k + 1], HP.H, HP.W, dev) for k, s in enumerate(scans)])
    d3 = torch.cat([ops.lidar_pinhole_depth(scans[k:k + 3], Ps[k:k + 3], HP.H, HP.W, dev) for k in range(0, G, 3)])
    op = ops.LidarPinholeDepth(G, HP.H, HP.W, dev)
    op.stage(scans, Ps)
    HK.run_captured(op, dict(depth=-1.0))
    assert (a > 0).sum() > 20000
    for d in (b, d1, d3, op.depth):
        assert torch.equal(d.view(torch.int32), a.view(torch.int32))


def test_evaluator_round_trip_and_metric(dev, tree, tmp_path):
    from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import Kitti360Evaluator
    g = np.load(GOLD)
    raw, _, val = tree
    gt_file = str(tmp_path / "gt.npz")
    ev = Kitti360Evaluator(raw, val, gt_file, device=dev, group_size=3)
    assert os.path.isfile(gt_file)
    data = np.load(gt_file)["data"]                                       # the reference's own loader
    assert data.dtype == np.float32 and data.shape == (len(HP.EVAL_FRAMES), HP.H, HP.W)
    ev2 = Kitti360Evaluator(raw, val, gt_file, device=dev)
    P = HP.velo_to_image(raw)
    for j in range(len(HP.EVAL_FRAMES)):
        assert np.array_equal(ev.gt_depths[j], ev2.gt_depths[j]) and np.array_equal(ev.gt_depths[j], data[j])
        want_gt = HP.dense(g["gt%d_idx" % j], g["gt%d_val" % j])
        _compare(np.asarray(ev.gt_depths[j]), want_gt, HP.scan(raw, HP.EVAL_FRAMES[j]), P, "export %d" % j)
        pred = torch.from_numpy(g["pred%d" % j]).to(dev)
        a, b = ev.single_call(pred, j), ev2.single_call(pred, j)
        # medians do not depend on the order in which fs_depth_eval compacts the valid pixels; its f64 error sums may
        # differ in their last bits with that order
        assert a["ratio"] == b["ratio"]
        for key in ("error", "abs_error"):
            assert np.allclose(a[key], b[key], rtol=1e-12, atol=0)
        want = g["loss%d" % j]
        HK.check_metric(a, dict(ratio=want[0], error=want[1:8], abs_error=want[8:15]), int((want_gt > 1e-3).sum()))
        assert int(ev.device_errors(pred, j).cpu().numpy()[15]) > 1000


def _model(h, w, dev):
    """kitti360_wpose_example's meta-arch (MonoDepthWPose, ResNet-18, 16 bins, depth 0.5-100, overlapped_mask) at
    h x w, fp32"""
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import fsnet_oracle as O
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    cfg = meta_arch_cfg(h, w, with_pose=False, num_output_channels=16, min_depth=0.5, max_depth=100.0)
    assert cfg["name"].endswith("MonoDepthWPose") and cfg["head_cfg"]["overlapped_mask"] is True
    m = build(**cfg)
    m.load_state_dict(O.init_state(seed=2, with_pose=False), strict=True)
    return m.to(dev)


def test_evaluation_hook_end_to_end(dev, tree, tmp_path):
    """KittiEvaluationHook with Kitti360Evaluator over the mirrored validation dataset (kitti360_wpose_example's
    validation chain: ConvertToFloat, Resize without aspect ratio, Normalize, ConvertToTensor), against the same network
    output put through the host pipeline: the oracle's inverse resize and the Eigen metric restated in
    oracle/eval_oracle.py"""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.monodepth.data.datasets.kitti360_dataset import KITTI360MonoDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import eval_oracle as EO
    raw, _, val = tree
    h, w = 64, 128
    ds = KITTI360MonoDataset(raw_path=raw, split_file=val, is_filter_static=False, use_right_image=False,
                             augmentation=HK.val_augmentation(h, w))
    assert len(ds) == len(HP.EVAL_FRAMES)
    m = _model(h, w, dev)
    hook = build(name="fsnet_amd.monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks.KittiEvaluationHook",
                 test_run_hook_cfg=dict(name="fsnet_amd.vision_base.pipeline_hooks.train_val_hooks.base_validation_hooks.BaseValidationHook"),
                 dataset_eval_cfg=dict(name="fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval.Kitti360Evaluator",
                                       data_path=raw, split_file=val, gt_saved_file=str(tmp_path / "gt.npz"), device=dev),
                 batch_size=2, num_workers=0)
    res = hook(m, ds)
    ev = hook.dataset_eval_func
    assert type(ev).__name__ == "Kitti360Evaluator" and os.path.isfile(str(tmp_path / "gt.npz"))
    m.eval()
    want = []
    with torch.no_grad():
        for i in range(len(ds)):
            batch = DeviceAugment([0])([ds[i]], dev)
            assert batch[('image', 0)].shape == (1, 3, h, w)
            depth = m(batch, dict(is_training=False))["depth"][0, 0, :h, :w].float().cpu().numpy()
            depth_0 = 1 / EO.cv2_resize_linear(1 / depth, HP.W, HP.H)
            want.append(EO.single_loss(depth_0, np.asarray(ev.gt_depths[i]).copy())["error"])
    m.train()
    RT.set_compute_dtype(torch.bfloat16)
    want = np.array(want, np.float64).mean(0)
    print("hook", res["mean_errors"], "host", want)
    assert np.abs(res["mean_errors"][:4] - want[:4]).max() <= 1e-4 * max(1.0, np.abs(want[:4]).max())
    assert np.abs(res["mean_errors"][4:] - want[4:]).max() <= 2e-3


def _train_cfg(raw, split, h, w, cls, **kw):
    return dict(name=cls, raw_path=raw, split_file=split,
                augmentation=HK.train_augmentation(h, w, origs_in_image_keys=True), **kw)


def test_training_step_from_the_dataset(dev, tree):
    """KITTI360MonoDataset (both pinhole cameras, P2, ones patched_mask, relative poses) through DeviceAugment's Resize
    into one training step of kitti360_wpose_example's meta-arch, against the same samples collated on the host and fed
    directly.  The two batches' images come from different code (kernel vs numpy) and agree to float32 rounding, so
    the losses are compared to 2e-5 relative, the bound the fisheye counterpart uses for the same reason."""
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    from fsnet_amd.vision_base.utils.builder import build
    raw, train, _ = tree
    h, w = 64, 128
    ds = build(**_train_cfg(raw, train, h, w, "fsnet_amd.monodepth.data.datasets.kitti360_dataset.KITTI360MonoDataset",
                            use_right_image=True))
    np.random.seed(1)
    samples = [ds[i] for i in range(4)]
    assert len({float(np.asarray(s["original_P2"])[0, 2]) for s in samples}) == 2       # both cameras in the batch
    direct = HK.direct_batch(samples, h, w, dev)
    batch = DeviceAugment([0, -1, 1])([dict(s) for s in samples], dev)
    assert PLAN not in batch and batch['patched_mask'].dtype == torch.float64 and batch['P2'].shape == (4, 3, 4)
    for k in direct:
        print(k, float((batch[k].double() - direct[k].double()).abs().max()))
    losses = HK.step_losses((batch, direct), lambda: _model(h, w, dev))
    print("losses", losses)
    assert np.isfinite(losses).all() and 0 < losses[0] < 10
    assert abs(losses[0] - losses[1]) <= 2e-5 * abs(losses[1])


def test_mixed_kitti_and_kitti360_batch(dev, tree, tmp_path):
    """one batch mixing KITTI (24 x 80) and KITTI-360 (94 x 310) source frames through DeviceAugment's per-sample
    dims: the resized images equal the host restatement per sample, and the training step's loss agrees to the same
    2e-5 relative bound"""
    from tests import helpers_kitti as HKI
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from fsnet_amd.vision_base.utils.builder import build
    raw360, train360, _ = tree
    raw, split = HKI.make_tree(str(tmp_path))
    h, w = 64, 128
    kitti = build(**_train_cfg(raw, split, h, w, "fsnet_amd.monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset",
                               frame_idxs=[0, -1, 1], is_filter_static=True))
    k360 = build(**_train_cfg(raw360, train360, h, w,
                              "fsnet_amd.monodepth.data.datasets.kitti360_dataset.KITTI360MonoDataset"))
    np.random.seed(5)
    samples = [kitti[0], k360[1], kitti[1], k360[4]]
    assert {s[('image', 0)].shape[:2] for s in samples} == {(HKI.H, HKI.W), (HP.H, HP.W)}
    direct = HK.direct_batch(samples, h, w, dev)
    batch = DeviceAugment([0, -1, 1])([dict(s) for s in samples], dev)
    for k in direct:
        d = float((batch[k].double() - direct[k].double()).abs().max())
        print(k, d)
        # float32 lerps of values <= 255, then / 255 / std: a few float32 ulps of 2.7
        assert d <= 1e-5, k
    losses = HK.step_losses((batch, direct), lambda: _model(h, w, dev))
    print("losses", losses)
    assert np.isfinite(losses).all() and 0 < losses[0] < 10
    assert abs(losses[0] - losses[1]) <= 2e-5 * abs(losses[1])
