"""KITTI-360 fisheye evaluation on the device: fs_lidar_mei_depth against the REAL reference's ground truth
(tests/golden/kitti360_fisheye.npz), its determinism and graph capture, fs_depth_eval_masked against the reference's
_single_loss and a numpy restatement, and the evaluator's cached-file round trip."""
import os

import numpy as np
import pytest
import torch

from tests import helpers_kitti360 as HK

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "kitti360_fisheye.npz")
NEAR = 1e-9


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HK.make_tree(str(tmp_path_factory.mktemp("kitti360")))


def _inputs(raw):
    from fsnet_amd.monodepth.evaluation.kitti360_fisheye_eval import Kitti360FisheyeEvaluator
    from fsnet_amd.monodepth.data.datasets.utils import read_pc_from_bin
    ev = Kitti360FisheyeEvaluator(gt_depths=[np.zeros((2, 2), np.float32)])
    ev._load_calib(os.path.join(raw, "calibration"))
    scans = [read_pc_from_bin(os.path.join(raw, "data_3d_raw", HK.SEQ, "velodyne_points/data", "%010d.bin" % i))
             for i in HK.EVAL_FRAMES]
    return ev, scans, ev.velo_to_camera(), ev.mei_row()


def _explained(scan, T, P, calib, pix, H, W):
    """a mismatch at flat pixel `pix` is explained when a point contributing to that pixel has a coordinate within
    NEAR px of an integer or a norm within NEAR of 8 (the f64 transform's last ulp may then move it).  Contributing:
    the helper's int32-truncated index is the pixel, or a coordinate lies within NEAR below the pixel's left / top
    edge while the other one truncates into the pixel's column / row (the device result may have crossed that edge)."""
    u, v, _, norm = HK.gt_points(scan, T, P, calib)
    py, px = divmod(int(pix), W)
    iu, iv = u.astype(np.int32), v.astype(np.int32)
    on = (iu == px) & (iv == py)
    edge = ((np.abs(u - px) < NEAR) & (iv == py)) | ((np.abs(v - py) < NEAR) & (iu == px))
    near_int = (np.abs(u - np.round(u)) < NEAR) | (np.abs(v - np.round(v)) < NEAR) | (np.abs(norm - 8.0) < NEAR)
    return bool(np.any((on | edge) & near_int))


def test_ground_truth_matches_reference(dev, tree):
    from fsnet_amd.hip import ops
    g = np.load(GOLD)
    raw = tree[0]
    ev, scans, T, mei = _inputs(raw)
    P, calib = ev.cam_calib['P0'], ev.cam_calib['left_calib']
    G = len(scans)
    depth, mask = ops.lidar_mei_depth(scans, np.stack([T] * G), np.stack([mei] * G), HK.H, HK.W, dev)
    depth, mask = depth.cpu().numpy(), mask.cpu().numpy().astype(bool)
    for j in range(G):
        want_d, want_m = HK.dense(g["gt%d_idx" % j], g["gt%d_val" % j], g["gt%d_midx" % j])
        d = depth[j]
        valid_diff = np.flatnonzero(((d > 0) != (want_d > 0)).reshape(-1))
        mask_diff = np.flatnonzero((mask[j] != want_m).reshape(-1))
        both = (d > 0) & (want_d > 0)
        ulps = np.abs(d[both].view(np.int32).astype(np.int64) - want_d[both].view(np.int32).astype(np.int64))
        far = np.flatnonzero(both.reshape(-1))[ulps > 1]
        print("frame %d: %d valid pixels, %d valid-set / %d mask mismatches, %d depths off by 1 ulp, %d by more" % (
            j, int((want_d > 0).sum()), len(valid_diff), len(mask_diff), int((ulps == 1).sum()), len(far)))
        for pix in np.concatenate([valid_diff, mask_diff, far]):
            assert _explained(scans[j], T, P, calib, pix, HK.H, HK.W), "frame %d pixel %d unexplained" % (j, pix)
        assert (want_d > 0).sum() > 5000


def test_ground_truth_deterministic_and_capturable(dev, tree):
    from fsnet_amd.hip import ops
    raw = tree[0]
    _, scans, T, mei = _inputs(raw)
    G = len(scans)
    Ts, meis = np.stack([T] * G), np.stack([mei] * G)
    a = [t.clone() for t in ops.lidar_mei_depth(scans, Ts, meis, HK.H, HK.W, dev)]
    b = [t.clone() for t in ops.lidar_mei_depth(scans, Ts, meis, HK.H, HK.W, dev)]
    ones = [ops.lidar_mei_depth([s], T[None], mei[None], HK.H, HK.W, dev) for s in scans]
    d1 = torch.cat([o[0] for o in ones])
    m1 = torch.cat([o[1] for o in ones])
    threes = [ops.lidar_mei_depth(scans[k:k + 3], Ts[k:k + 3], meis[k:k + 3], HK.H, HK.W, dev) for k in range(0, G, 3)]
    d3 = torch.cat([o[0] for o in threes])
    m3 = torch.cat([o[1] for o in threes])
    op = ops.LidarMeiDepth(G, HK.H, HK.W, dev)
    op.stage(scans, Ts, meis)
    HK.run_captured(op, dict(depth=-1.0, close_mask=7))
    for d, m in ((b[0], b[1]), (d1, m1), (d3, m3), (op.depth, op.close_mask)):
        assert torch.equal(d.view(torch.int32), a[0].view(torch.int32)) and torch.equal(m, a[1])


def _cases(rng, H, W, h, w):
    gt = np.zeros((H, W), np.float32)
    m = rng.rand(H, W) < 0.3
    gt[m] = (rng.rand(int(m.sum())) * 70).astype(np.float32)          # some beyond 60 m and below 0.3 m: masked out
    close = rng.rand(H, W) < 0.6
    pred = (rng.rand(h, w) * 40 + 0.5).astype(np.float32)
    return pred, gt, close


def test_masked_metric_matches_reference_and_restatement(dev):
    from oracle import eval_oracle as EO
    from fsnet_amd.monodepth.evaluation.kitti360_fisheye_eval import Kitti360FisheyeEvaluator
    g = np.load(GOLD)
    n = int(g["n_gt"])
    gts, masks = zip(*[HK.dense(g["gt%d_idx" % j], g["gt%d_val" % j], g["gt%d_midx" % j]) for j in range(n)])
    ev = Kitti360FisheyeEvaluator(gt_depths=list(gts), close_masks=list(masks), device=dev)
    for j in range(n):
        want = g["loss%d" % j]
        got = ev.single_call(torch.from_numpy(g["pred%d" % j]).to(dev), j)
        nv = int(((gts[j] > np.float32(0.3)) & (gts[j] < np.float32(60)) & masks[j]).sum())
        HK.check_metric(got, dict(ratio=want[0], error=want[1:8], abs_error=want[8:15]), nv)
        row = ev.device_errors(torch.from_numpy(g["pred%d" % j]).to(dev), j).cpu().numpy()
        assert int(row[15]) == nv
    rng = np.random.RandomState(23)
    for H, W, h, w in ((350, 350, 175, 175), (120, 200, 120, 200), (64, 90, 31, 47)):
        pred, gt, close = _cases(rng, H, W, h, w)
        want = HK.single_loss(EO.cv2_resize_linear(pred, W, H), gt, close)
        got = ev._single_loss(torch.from_numpy(pred).to(dev), gt, close)
        HK.check_metric(got, want, int(((gt > np.float32(0.3)) & (gt < np.float32(60)) & close).sum()))
    # negative predictions (a fisheye depth is Z x norm, negative where the ray table is invalid): np.median orders
    # them below the positive ones
    pred, gt, close = _cases(rng, 120, 200, 120, 200)
    pred[rng.rand(120, 200) < 0.45] *= -1.0
    want = HK.single_loss(pred, gt, close)
    got = ev._single_loss(torch.from_numpy(pred).to(dev), gt, close)
    HK.check_metric(got, want, int(((gt > np.float32(0.3)) & (gt < np.float32(60)) & close).sum()))
    # the crop flag and the mask-less form of fs_depth_eval_masked, against the same restatement
    from fsnet_amd.hip import ops
    for crop, with_mask in ((True, True), (False, False), (True, False)):
        pred, gt, close = _cases(rng, 120, 200, 60, 100)
        valid = (gt > np.float32(0.3)) & (gt < np.float32(60))
        if with_mask:
            valid &= close
        if crop:
            c = np.array([0.40810811 * 120, 0.99189189 * 120, 0.03594771 * 200, 0.96405229 * 200]).astype(np.int32)
            garg = np.zeros((120, 200), bool)
            garg[c[0]:c[1], c[2]:c[3]] = True
            valid &= garg
        want = HK.single_loss(EO.cv2_resize_linear(pred, 200, 120), np.where(valid, gt, 0).astype(np.float32),
                              np.ones((120, 200), bool))
        row = ops.depth_eval_masked(torch.from_numpy(pred).to(dev)[None], torch.from_numpy(gt).to(dev)[None],
                                    torch.from_numpy(close).to(dev)[None] if with_mask else None, crop=crop)[0]
        row = row.cpu().numpy()
        assert int(row[15]) == int(valid.sum()), (crop, with_mask)
        HK.check_metric(dict(ratio=row[0], error=row[1:8], abs_error=row[8:15]), want, int(valid.sum()))
    with pytest.raises(ValueError):
        ev._single_loss(torch.ones(50, 60, device=dev), np.full((50, 60), 70.0, np.float32), np.ones((50, 60), bool))
    with pytest.raises(ValueError):
        ev._single_loss(torch.ones(50, 60, device=dev), np.full((50, 60), 5.0, np.float32), np.zeros((50, 60), bool))


def test_evaluator_round_trip(dev, tree, tmp_path):
    from fsnet_amd.monodepth.evaluation.kitti360_fisheye_eval import Kitti360FisheyeEvaluator
    raw, _, val, _ = tree
    gt_file = str(tmp_path / "gt.npz")
    ev = Kitti360FisheyeEvaluator(raw, val, gt_file, device=dev, group_size=3)
    assert os.path.isfile(gt_file)
    data = np.load(gt_file)["data"]                                       # the reference's own loader
    assert data.dtype == np.float32 and data.shape == (len(HK.EVAL_FRAMES), HK.H, HK.W)
    cm = np.load(gt_file)["close_masks"]
    assert cm.dtype == bool and cm.shape == data.shape
    ev2 = Kitti360FisheyeEvaluator(raw, val, gt_file, device=dev)
    rng = np.random.RandomState(4)
    for j in range(len(HK.EVAL_FRAMES)):
        assert np.array_equal(ev.gt_depths[j], ev2.gt_depths[j]) and np.array_equal(ev.close_masks[j], ev2.close_masks[j])
        pred = torch.from_numpy((rng.rand(175, 175) * 30 + 0.5).astype(np.float32)).to(dev)
        a, b = ev.single_call(pred, j), ev2.single_call(pred, j)
        # medians do not depend on the order in which the kernel compacts the valid pixels; the f64 error sums may
        # differ in their last bits with that order — as in fs_depth_eval, whose compaction (an atomicAdd slot per
        # valid pixel) and per-thread sums this kernel shares
        assert a["ratio"] == b["ratio"]
        for key in ("error", "abs_error"):
            assert np.allclose(a[key], b[key], rtol=1e-12, atol=0)


def _fisheye_model(h, w, dev):
    """configs[3]'s meta-arch (MonoDepthWPose + FishEyeDecoder, ResNet-18, 64 bins, max depth 150) at h x w, fp32"""
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import fsnet_oracle as O
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    m = build(**meta_arch_cfg(h, w, with_pose=False, num_output_channels=64, max_depth=150.0, fisheye=True))
    m.load_state_dict(O.init_state(seed=5, with_pose=False, num_out=64, max_depth=150.0), strict=True)
    return m.to(dev)


def test_evaluation_hook_end_to_end(dev, tree, tmp_path):
    """KittiEvaluationHook with Kitti360FisheyeEvaluator over the mirrored validation dataset (configs[3]'s validation
    chain: ConvertToFloat, Resize without aspect ratio, Normalize, ConvertToTensor), against the same network output
    put through the host pipeline: the oracle's inverse resize and the restated fisheye _single_loss"""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.monodepth.data.datasets.fisheye_dataset import KITTI360FisheyeDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import eval_oracle as EO
    raw, _, val, _ = tree
    h, w = 64, 64
    ds = KITTI360FisheyeDataset(raw_path=raw, split_file=val, is_filter_static=False, use_right_image=False,
                                augmentation=HK.val_augmentation(h, w))
    assert len(ds) == len(HK.EVAL_FRAMES)
    m = _fisheye_model(h, w, dev)
    hook = build(name="fsnet_amd.monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks.KittiEvaluationHook",
                 test_run_hook_cfg=dict(name="fsnet_amd.vision_base.pipeline_hooks.train_val_hooks.base_validation_hooks.BaseValidationHook"),
                 dataset_eval_cfg=dict(name="fsnet_amd.monodepth.evaluation.kitti360_fisheye_eval.Kitti360FisheyeEvaluator",
                                       data_path=raw, split_file=val, gt_saved_file=str(tmp_path / "gt.npz"), device=dev),
                 batch_size=2, num_workers=0)
    res = hook(m, ds)
    ev = hook.dataset_eval_func
    m.eval()
    want = []
    with torch.no_grad():
        for i in range(len(ds)):
            batch = DeviceAugment([0])([ds[i]], dev)
            assert batch[('image', 0)].shape == (1, 3, h, w)
            depth = m(batch, dict(is_training=False))["depth"][0, 0, :h, :w].float().cpu().numpy()
            depth_0 = 1 / EO.cv2_resize_linear(1 / depth, HK.W, HK.H)
            want.append(HK.single_loss(depth_0, np.asarray(ev.gt_depths[i]), np.asarray(ev.close_masks[i]))["error"])
    m.train()
    RT.set_compute_dtype(torch.bfloat16)
    want = np.array(want, np.float64).mean(0)
    print("hook", res["mean_errors"], "host", want)
    assert np.abs(res["mean_errors"][:4] - want[:4]).max() <= 1e-4 * max(1.0, np.abs(want[:4]).max())
    assert np.abs(res["mean_errors"][4:] - want[4:]).max() <= 2e-3


def test_training_step_from_the_dataset(dev, tree):
    """KITTI360FisheyeDataset (Mei calibration, P2, calib_meta, float64 patched_mask, relative poses) through
    DeviceAugment's Resize into one training step of configs[3]'s meta-arch, against the same samples collated on the
    host (numpy restatement of the resize and Normalize) and fed directly.  The two batches' images come from different
    code (kernel vs numpy) and agree to float32 rounding, so the losses are compared to 2e-5 relative, the bound of the
    fisheye training-step test against its oracle."""
    from fsnet_amd.monodepth.data.datasets.fisheye_dataset import KITTI360FisheyeDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    raw, train, _, _ = tree
    h, w = 64, 64
    ds = KITTI360FisheyeDataset(raw_path=raw, split_file=train, use_right_image=True,
                                augmentation=HK.train_augmentation(h, w, origs_in_image_keys=False))
    np.random.seed(1)
    samples = [ds[i] for i in range(4)]
    assert len({s["calib_meta"]["mirror_parameters"]["xi"] for s in samples}) == 2      # both cameras in the batch
    direct = HK.direct_batch(samples, h, w, dev, fisheye=True)
    batch = DeviceAugment([0, -1, 1])([dict(s) for s in samples], dev)
    assert PLAN not in batch and batch['patched_mask'].dtype == torch.float64 and batch['P2'].shape == (4, 3, 4)
    for k in list(direct):
        if isinstance(direct[k], torch.Tensor):
            print(k, float((batch[k].double() - direct[k].double()).abs().max()))
    losses = HK.step_losses((batch, direct), lambda: _fisheye_model(h, w, dev))
    print("losses", losses)
    assert np.isfinite(losses).all() and 0 < losses[0] < 10
    assert abs(losses[0] - losses[1]) <= 2e-5 * abs(losses[1])
