"""Motion-mask precompute on the device (csrc/optflow.hip through ops.optical_flow_farneback / ops.motion_mask /
ops.augment_masks and the precompute hooks) against the CPU restatement (tests/helpers_optflow.py): each stage fed
the kernel's own previous stage, the whole pipeline, accuracy on synthetic scenes, determinism and capture, the hook
end to end, masks through the augmentation plans."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import augment_oracle as AO
from tests import helpers_kitti as HK
from tests import helpers_optflow as HO
from tests.test_motion_mask_cpu import CORRIDOR_EPE

pytestmark = pytest.mark.gpu


def _ops():
    from fsnet_amd.hip import ops
    return ops


def flow_of(dev, img0, img1, ws=None, **cfg):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.ndim == 4 else a[None])).to(dev)   # noqa: E731
    return _ops().optical_flow_farneback(t(img0), t(img1), workspace=ws, **dict(HO.FLOW_CFG, **cfg))


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_stages_against_restatement(dev):
    ops = _ops()
    img0, img1, _, _, _ = HO.corridor_pair(96, 320, seed=1)
    for flags in (0, HO.GAUSSIAN):
        cfg = dict(levels=0, iterations=2, flags=flags)
        ws = torch.empty(ops.optflow_workspace_bytes(1, 96, 320, **dict(HO.FLOW_CFG, **cfg)), dtype=torch.uint8,
                         device=dev)
        out = flow_of(dev, img0, img1, ws, **cfg)[0].cpu().numpy()
        v = {k: t.cpu().numpy() for k, t in HO.workspace_views(ws, 1, 96, 320).items()}
        assert np.array_equal(v["gray"][0, 0], HO.gray(img0)) and np.array_equal(v["gray"][0, 1], HO.gray(img1))
        for f in (0, 1):
            assert rel_err(v["img"][0, f], HO.level_image(v["gray"][0, f], 96, 320, 3, 0.0)) <= 1e-5
            assert rel_err(v["R"][0, f], HO.poly_exp(v["img"][0, f], 5, 1.2)) <= 1e-5
        R0, R1 = v["R"][0, 0], v["R"][0, 1]
        fin = v["f1"][0]                                  # the flow that entered the second (last) iteration
        assert rel_err(v["M"][0], HO.update_matrices(R0, R1, fin)) <= 1e-5
        want = HO.window_solve(HO.update_matrices(R0, R1, fin), 15, flags)
        assert np.percentile(np.abs(out - want), 99.9) <= 1e-3, flags
    # the coarse levels' blur (sigma > 0, ksize up to 19) and bilinear resize, one level at a time
    g0, g1 = HO.gray(img0), HO.gray(img1)
    i0, i1 = (torch.from_numpy(a[None]).to(dev) for a in (img0, img1))
    for lv, h, w, ksize, sigma in HO.pyramid_plan(96, 320, 0.5, 3):
        got = _ops().optflow_level_image(i0, i1, lv, h, w, **HO.FLOW_CFG)[0].cpu().numpy()
        for f, gg in enumerate((g0, g1)):
            assert rel_err(got[f], HO.level_image(gg, h, w, ksize, 0.0 if lv == 0 else sigma)) <= 1e-5, (lv, f)
    big = HO.corridor_pair(375, 1242, seed=2)[0]
    for lv, h, w, ksize, sigma in HO.pyramid_plan(375, 1242, 0.5, 3):       # ksize 19 at the coarsest level
        got = _ops().optflow_level_image(*(torch.from_numpy(big[None]).to(dev),) * 2, lv, h, w, **HO.FLOW_CFG)
        assert rel_err(got[0, 0].cpu().numpy(), HO.level_image(HO.gray(big), h, w, ksize, 0.0 if lv == 0 else sigma)) \
            <= 1e-5, lv
    # the whole pipeline with its pyramid
    for flags in (0, HO.GAUSSIAN):
        out = flow_of(dev, img0, img1, flags=flags)[0].cpu().numpy()
        want = HO.farneback(img0, img1, **dict(HO.FLOW_CFG, flags=flags))
        d = np.abs(out - want)
        assert np.median(d) <= 1e-4 and (d > 0.05).mean() <= 1e-3, (flags, np.median(d), (d > 0.05).mean())


def test_flow_accuracy_on_corridor(dev):
    img0, img1, _, _, rigid = HO.corridor_pair(96, 320, seed=1)
    f = flow_of(dev, img0, img1)[0].cpu().numpy()
    epe = np.median(np.hypot(*(f - rigid).transpose(2, 0, 1)))
    assert epe < CORRIDOR_EPE, epe


def test_motion_mask_on_moving_box(dev):
    """calibrated on the restatement: recall 1.000, false positives 0.76 % (96x320, seed 1, shift 4, thr 2)"""
    img0, img1, P2, T, _, box, near = HO.moving_box_pair(96, 320, seed=1, shift=4)
    flow = flow_of(dev, img0, img1)
    mask = _ops().motion_mask(flow, torch.from_numpy(P2)[None], torch.from_numpy(T)[None], 2.0, 0)[0].cpu().numpy()
    m = mask.astype(bool)
    assert m[box].mean() >= 0.8, m[box].mean()
    assert m[~near].mean() <= 0.02, m[~near].mean()
    # the kernel's mask of a given flow equals the reference's torch block, away from the threshold
    d = HO.epipolar_distance(flow[0].cpu().numpy(), P2, T).numpy()
    want = HO.motion_mask(flow[0].cpu().numpy(), P2, T, 2.0, 0)
    close = np.abs(np.abs(d) - 2.0) <= 1e-4 * 2.0
    assert np.array_equal(mask[~close], want[~close])


def test_motion_mask_mode1_and_ieee(dev):
    """mode 1 (|d| / |flow|) against the reference's block on a generic pose; a zero pose gives F = 0, so d = NaN and
    nothing is masked in either mode, as in the reference"""
    from scipy.spatial.transform import Rotation
    P2 = np.array([[700.0, 0, 300, 0], [0, 700, 100, 0], [0, 0, 1, 0]])
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("xyz", [0.01, -0.02, 0.005]).as_matrix()
    T[:3, 3] = (0.1, -0.05, -0.8)
    rng = np.random.RandomState(0)
    flow = rng.uniform(-3, 3, size=(32, 48, 2)).astype(np.float32)
    flow[5:9, 7:11] = 0.0                                  # zero flow: d / 0 = inf, masked
    f = torch.from_numpy(flow)[None].to(dev)
    m = _ops().motion_mask(f, torch.from_numpy(P2)[None], torch.from_numpy(T)[None], 0.5, 1)[0].cpu().numpy()
    want = HO.motion_mask(flow, P2, T, 0.5, 1)
    d = HO.epipolar_distance(flow, P2, T).numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(d) / np.hypot(flow[..., 0], flow[..., 1])
    far = ~(np.abs(q - 0.5) <= 1e-4 * 0.5)
    assert np.array_equal(m[far], want[far]) and m[5:9, 7:11].all()
    for mode in (0, 1):
        z = _ops().motion_mask(f, torch.from_numpy(P2)[None], torch.eye(4, dtype=torch.float64)[None], 0.5, mode)
        assert int(z.sum()) == 0


def test_flow_and_mask_bit_identical(dev):
    ops = _ops()
    img0, img1, P2, T, _, _, _ = HO.moving_box_pair(96, 320, seed=1, shift=4)
    pairs = [HO.corridor_pair(96, 320, seed=s)[:2] for s in (2, 3, 4)]
    i0 = torch.from_numpy(np.stack([img0] + [p[0] for p in pairs])).to(dev)
    i1 = torch.from_numpy(np.stack([img1] + [p[1] for p in pairs])).to(dev)
    a = ops.optical_flow_farneback(i0[:1], i1[:1], **HO.FLOW_CFG)
    b = ops.optical_flow_farneback(i0[:1], i1[:1], **HO.FLOW_CFG)
    c = ops.optical_flow_farneback(i0, i1, **HO.FLOW_CFG)
    assert torch.equal(a, b) and torch.equal(a[0], c[0])
    P = torch.from_numpy(np.stack([P2] * 4)).to(dev)
    Tt = torch.from_numpy(np.stack([T] * 4)).to(dev)
    ma = ops.motion_mask(a, P[:1], Tt[:1], 2.0, 0)
    assert torch.equal(ma, ops.motion_mask(b, P[:1], Tt[:1], 2.0, 0))
    assert torch.equal(ma[0], ops.motion_mask(c, P, Tt, 2.0, 0)[0])
    # captured into a graph and replayed
    ws = torch.empty(ops.optflow_workspace_bytes(4, 96, 320, **HO.FLOW_CFG), dtype=torch.uint8, device=dev)
    out = torch.empty(4, 96, 320, 2, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.optical_flow_farneback(i0, i1, workspace=ws, out=out, **HO.FLOW_CFG)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.optical_flow_farneback(i0, i1, workspace=ws, out=out, **HO.FLOW_CFG)
        gm = ops.motion_mask(out, P, Tt, 2.0, 0)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, c) and torch.equal(gm[0], ma[0])


def test_hook_end_to_end(dev, tmp_path):
    from fsnet_amd.monodepth.pipeline_hooks.precomputing_hooks.base_precompute_hooks import (
        MotionMaskARFlowPrecomputeHook, MotionMaskPrecomputeHook)
    from fsnet_amd.monodepth.data.datasets.mono_dataset import KittiDepthMonoDataset
    from fsnet_amd.monodepth.data.datasets import utils as U
    raw, split = HK.make_tree(str(tmp_path), seed=5, H=64, W=96)
    cfg = dict(HK.dataset_cfg(raw, split, prefix='fsnet_amd.'),
               name='fsnet_amd.monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset')
    fcfg = dict(pyr_scale=0.5, levels=2, winsize=9, iterations=2, poly_n=5, poly_sigma=1.1, flags=0)
    out = tmp_path / "masks"
    hook = MotionMaskPrecomputeHook(cfg, fcfg, distance_threshold=1.5, output_dir=str(out))
    hook()
    ds = KittiDepthMonoDataset(**{k: v for k, v in cfg.items() if k != 'name'})
    files = sorted(os.listdir(out))
    assert files == ["%08d.png" % i for i in range(len(ds))]
    for i in range(len(ds)):
        s = ds[i]
        f = flow_of(dev, s[("image", 0)], s[("image", 1)], **fcfg)
        want = _ops().motion_mask(f, torch.as_tensor(np.asarray(s["P2"], np.float64))[None],
                                  torch.as_tensor(np.asarray(s[("relative_pose", 1)], np.float64))[None], 1.5,
                                  0)[0].cpu().numpy()
        png = Image.open(str(out / files[i]))
        assert png.mode == "L" and np.array_equal(np.array(png), want)
    # a second call skips what exists; the batched, threaded form writes the same files
    stamp = {f: os.path.getmtime(str(out / f)) for f in files}
    os.remove(str(out / files[0]))
    MotionMaskPrecomputeHook(cfg, fcfg, distance_threshold=1.5, output_dir=str(out), batch_size=3, num_workers=2)()
    assert all(os.path.getmtime(str(out / f)) == stamp[f] for f in files[1:])
    out2 = tmp_path / "masks2"
    MotionMaskPrecomputeHook(cfg, fcfg, distance_threshold=1.5, output_dir=str(out2), batch_size=3, num_workers=2)()
    for f in files:
        assert np.array_equal(np.array(Image.open(str(out / f))), np.array(Image.open(str(out2 / f))))
    # the ARFlow hook over precomputed flow files
    fdir = tmp_path / "flow"
    fdir.mkdir()
    rng = np.random.RandomState(4)
    for i in range(len(ds)):
        U.write_png16(str(fdir / ("%08d.png" % i)), rng.randint(2 ** 15 - 300, 2 ** 15 + 300, size=(64, 96, 3)))
    acfg = dict(cfg, is_precompute_flow=True, flow_path=str(fdir))
    out3 = tmp_path / "masks3"
    MotionMaskARFlowPrecomputeHook(acfg, {}, distance_threshold=0.5, output_dir=str(out3))()
    for i in range(len(ds)):
        s = ds[i]
        flow = U.read_flow_png(str(fdir / ("%08d.png" % i)))
        P2, pose = np.asarray(s["original_P2"], np.float64), np.asarray(s[("relative_pose", 1)])
        want = HO.motion_mask(flow, P2, pose, 0.5, 1)
        d = HO.epipolar_distance(flow, P2, pose).numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.abs(d) / np.hypot(flow[..., 0], flow[..., 1])
        far = ~(np.abs(q - 0.5) <= 1e-4 * 0.5)
        got = np.array(Image.open(str(out3 / ("%08d.png" % i))))
        assert np.array_equal(got[far], want[far])


@pytest.mark.parametrize("kind", ["warp", "resize"])
def test_mask_augmentation_matches_oracle(dev, kind):
    from fsnet_amd.vision_base.data.augmentations import augmentations as A
    from tests.test_motion_mask_cpu import _sample
    keys = [("image", f) for f in (0, 1, -1)] + [("original_image", f) for f in (0, 1, -1)]
    gt = ['patched_mask', 'motion_mask']
    np.random.seed(7)
    if kind == "warp":
        geo = A.RandomWarpAffine(output_w=256, output_h=96, shift_border=64, image_keys=keys, gt_image_keys=gt,
                                 calib_keys=['P2'], random_seed=1)
    else:
        geo = A.Resize(size=(96, 256), image_keys=keys, gt_image_keys=gt, calib_keys=['P2'])
    mirror = A.RandomMirror(0.5, image_keys=keys, gt_image_keys=gt)
    chain = [A.ConvertToFloat(image_keys=keys), geo, mirror, A.ConvertToTensor(image_keys=keys, gt_image_keys=gt)]
    samples, raws = [], []
    for seed in range(4):
        d = _sample(H=300 - 10 * seed, W=420, seed=seed)
        raws.append(d["motion_mask"].copy())
        for t in chain:
            d = t(d)
        samples.append(d)
    plans = [s[A.PLAN] for s in samples]
    batch = A.DeviceAugment(frame_idxs=(0, 1, -1)).materialize(A.DeviceAugment(frame_idxs=(0, 1, -1)).collate(samples),
                                                               dev)
    got = batch["motion_mask"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (4, 96, 256)
    for b, (m, p) in enumerate(zip(raws, plans)):
        if kind == "warp":
            want = AO.warp_affine_nearest(m, p["warp"]["M"], 256, 96)
        else:
            r = p["resize"]
            want = AO._crop_pad(AO.resize_nearest(m, r["w"], r["h"]), r["mode"], (96, 256))
        if p["mirror"]:
            want = want[:, ::-1]
        assert np.array_equal(got[b], want.astype(np.float32)), b
    assert any(p["mirror"] for p in plans) and not all(p["mirror"] for p in plans)


def test_masks_match_real_reference_hooks(dev, tmp_path):
    """tests/golden/motion_mask.npz: the REAL MotionMaskPrecomputeHook (box and Gaussian windows) and
    MotionMaskARFlowPrecomputeHook over a seeded 96x320 make_tree tree (tools/gen_golden.py::gen_motion_mask; the
    reference's flow is the restatement through the cv2 shim).  This project's hooks run over the same tree; their
    files equal the reference's except pixels whose |d| lies within 1e-4 thr of the threshold or whose kernel flow
    differs from the restated flow by more than 1e-3 px (reported)."""
    from fsnet_amd.monodepth.pipeline_hooks.precomputing_hooks.base_precompute_hooks import (
        MotionMaskARFlowPrecomputeHook, MotionMaskPrecomputeHook)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_mask.npz"))
    H, W = HO.GOLDEN_HW
    raw, split = HK.make_tree(str(tmp_path), seed=HO.GOLDEN_TREE_SEED, H=H, W=W)
    cfg = HO.raw_dataset_cfg(raw, split, prefix='fsnet_amd.')
    n = int(g["n"])
    for tag, fcfg in (("box", HO.GOLDEN_FLOW_CFG), ("gauss", HO.GOLDEN_FLOW_CFG_G)):
        odir = tmp_path / ("mm_" + tag)
        hook = MotionMaskPrecomputeHook(cfg, fcfg, distance_threshold=HO.GOLDEN_THR[0], output_dir=str(odir))
        hook()
        assert len(hook.dataset) == n and sorted(os.listdir(odir)) == list(g[tag + "_names"])
        excluded = 0
        for i in range(n):
            s = hook.dataset[i]
            P2, pose = np.asarray(s["P2"], np.float64), np.asarray(s[("relative_pose", 1)])
            assert np.array_equal(P2, g["s%d_P2" % i]) and np.array_equal(pose, g["s%d_pose" % i])
            want_flow = HO.farneback(s[("image", 0)], s[("image", 1)], **fcfg)
            assert float(np.abs(want_flow).astype(np.float64).sum()) == float(g[tag + "_flow_abs_sum"][i])
            flow = flow_of(dev, s[("image", 0)], s[("image", 1)], **fcfg)[0].cpu().numpy()
            d = HO.epipolar_distance(want_flow, P2, pose).numpy()
            skip = (np.abs(np.abs(d) - HO.GOLDEN_THR[0]) <= 1e-4 * HO.GOLDEN_THR[0]) | \
                (np.abs(flow - want_flow).max(-1) > 1e-3)
            got = np.array(Image.open(str(odir / ("%08d.png" % i))))
            want = g[tag + "_masks"][i]
            assert np.array_equal(got[~skip], want[~skip]), (tag, i, int((got[~skip] != want[~skip]).sum()))
            excluded += int(skip.sum())
        print("golden %s: %d of %d pixels excluded" % (tag, excluded, n * H * W))
        assert excluded <= 0.05 * n * H * W
    fdir = tmp_path / "flow"
    HO.write_flow_pngs(str(fdir), n, H, W)
    odir = tmp_path / "mm_arflow"
    MotionMaskARFlowPrecomputeHook(dict(cfg, is_precompute_flow=True, flow_path=str(fdir)), {},
                                   distance_threshold=HO.GOLDEN_THR[1], output_dir=str(odir))()
    assert sorted(os.listdir(odir)) == list(g["arflow_names"])
    from fsnet_amd.monodepth.data.datasets.utils import read_flow_png
    excluded = 0
    for i in range(n):
        flow = read_flow_png(str(fdir / ("%08d.png" % i)))
        d = HO.epipolar_distance(flow, g["s%d_original_P2" % i], g["s%d_pose" % i]).numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.abs(d) / np.hypot(flow[..., 0], flow[..., 1])
        skip = np.abs(q - HO.GOLDEN_THR[1]) <= 1e-4 * HO.GOLDEN_THR[1]
        got = np.array(Image.open(str(odir / ("%08d.png" % i))))
        assert np.array_equal(got[~skip], g["arflow_masks"][i][~skip]), i
        excluded += int(skip.sum())
    print("golden arflow: %d of %d pixels excluded" % (excluded, n * H * W))


def _train_setup(dev, tmp_path):
    """KittiDepthMonoDataset(is_motion_mask=True) over a make_tree tree with blocky 0/1 mask PNGs, through the
    kitti_wpose_example pipeline with gt_image_keys=['patched_mask', 'motion_mask'], one DeviceAugment batch"""
    from fsnet_amd.monodepth.data.datasets.mono_dataset import KittiDepthMonoDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, DeviceAugment
    from tests import helpers_augment as HA
    H, W = 64, 128
    g = dict(HA.golden())
    g["out_h"], g["out_w"] = np.int64(H), np.int64(W)
    raw, split = HK.make_tree(str(tmp_path), seed=5, H=300, W=420)
    mdir = tmp_path / "masks"
    mdir.mkdir()
    rng = np.random.RandomState(9)
    for i in range(3):
        coarse = (rng.rand(300 // 20 + 1, 420 // 20 + 1) > 0.5).astype(np.uint8)
        Image.fromarray(np.kron(coarse, np.ones((20, 20), np.uint8))[:300, :420]).save(str(mdir / ("%08d.png" % i)))
    cfg = HK.dataset_cfg(raw, split, prefix='fsnet_amd.')
    cfg["augmentation"] = HA.pipeline_cfg(g)
    cfg["augmentation"]["gt_image_keys"] = ['patched_mask', 'motion_mask']
    cfg.update(is_motion_mask=True, motion_mask_path=str(mdir))
    ds = KittiDepthMonoDataset(**cfg)
    aug = DeviceAugment(HA.FRAME_IDXS)
    np.random.seed(3)
    samples = [ds[i] for i in range(3)]
    raws = [np.array(Image.open(str(mdir / ("%08d.png" % i)))) for i in range(3)]
    plans = [s[PLAN] for s in samples]
    batch = aug.materialize(aug.collate(samples), dev)
    # the same mask computed directly: nearest warp of the PNG with the sample's plan, then its mirror
    direct = []
    for m, p in zip(raws, plans):
        w = AO.warp_affine_nearest(m, p["warp"]["M"], W, H)
        direct.append((w[:, ::-1] if p["mirror"] else w).astype(np.float32))
    return batch, torch.from_numpy(np.stack(direct)).to(dev), H, W


def _step(dev, batch, H, W, use_graph=False, masks=None):
    """fresh model from fixed weights, `len(masks)` training steps on `batch` with batch['motion_mask'] = masks[k]
    -> (losses, parameter gradients after the last step)"""
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    torch.manual_seed(0)
    m = build(**meta_arch_cfg(H, W, with_pose=False)).to(dev).train()
    tc = training_cfg()
    opt = build_optimizer(m, **tc.optimizer)
    hook = build(use_graph=use_graph, graph_warmup=2, **tc.training_hook)
    losses = []
    for mk in masks:
        data = dict(batch)
        data["motion_mask"] = mk
        out = hook(data, m, opt)
        losses.append(float(out["loss"].detach()))
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.detach().double().flatten() for p in m.parameters() if p.grad is not None]).cpu()
    RT.tie_noise = True
    RT.set_compute_dtype(torch.bfloat16)
    return losses, grads, hook


def test_motion_mask_reaches_the_loss_through_training(dev, tmp_path):
    """the dataset's motion_mask, through DeviceAugment, drives the training step exactly like the same mask fed
    directly; the inverse mask (same loss value: the mask only detaches) changes the gradients.  Two runs of one step
    are equal up to the order of fp atomics, so gradients compare at a relative 1e-3 against an O(1) effect."""
    batch, direct, H, W = _train_setup(dev, tmp_path)
    mm = batch["motion_mask"]
    assert mm.dtype == torch.float32 and mm.shape == (3, H, W) and torch.equal(mm, direct)
    assert 0.2 < float(mm.mean()) < 0.8
    la, ga, _ = _step(dev, batch, H, W, masks=[mm])
    lb, gb, _ = _step(dev, batch, H, W, masks=[direct.clone()])
    lc, gc, _ = _step(dev, batch, H, W, masks=[1.0 - direct])
    rel = lambda a, b: float((a - b).norm() / a.norm())      # noqa: E731
    assert abs(la[0] - lb[0]) <= 1e-5 * abs(la[0]) and rel(ga, gb) <= 1e-3, (la, lb, rel(ga, gb))
    assert rel(ga, gc) > 0.1, rel(ga, gc)
    # the captured step: the mask is staged into the graph's static buffers on every replay (steps 0, 1 eager, 2
    # captured, 3 replayed; the second run flips the mask at the replayed step).  Training trajectories of separate
    # runs drift apart over the steps (fp atomics; measured 0.14-0.20 relative), so the flip must move the
    # gradients several times further than a repeat of the same run does
    l1, g1, h1 = _step(dev, batch, H, W, use_graph=True, masks=[mm] * 4)
    l2, g2, h2 = _step(dev, batch, H, W, use_graph=True, masks=[mm] * 3 + [1.0 - mm])
    l3, g3, _ = _step(dev, batch, H, W, use_graph=True, masks=[mm] * 4)
    assert h1.graph_replays == h2.graph_replays == 1
    print("graph: same masks %.3g, flipped mask at the replay %.3g" % (rel(g1, g3), rel(g1, g2)))
    assert rel(g1, g2) > 0.5 and rel(g1, g3) < 0.5 * rel(g1, g2), (rel(g1, g3), rel(g1, g2))
