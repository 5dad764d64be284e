"""A patched_mask that is not all ones through both device input pipelines (fs_augment_frames_masked /
fs_resize_frames_masked): the kernels against the vectors of the reference's own classes, the frame path undisturbed,
the plane beside a motion_mask, the C ABI's refusals, and the nuScenes JSON dataset (CAM_BACK) into eager and captured
training steps."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_patched_mask as HM

pytestmark = pytest.mark.gpu


def _build(cfg):
    from fsnet_amd.vision_base.utils.builder import build
    return build(**cfg)


def _run(dev, kind, mirror, inputs, ones=False, gt_image_keys=('patched_mask',), extra=None):
    """the inputs through a freshly built chain (the same seeded draws every time) and one DeviceAugment launch"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, DeviceAugment
    t = _build(HM.train_cfg(kind, mirror, gt_image_keys=gt_image_keys))
    samples = []
    for n, (frames, mask) in enumerate(inputs):
        data = HM.sample_dict(frames, np.ones(mask.shape) if ones else mask)
        if extra is not None:
            data.update(extra[n])
        samples.append(t(data))
    aug = DeviceAugment(HM.FRAME_IDXS)
    host = aug.collate(samples)
    carried = "mask_src" in host[PLAN]
    batch = aug.materialize(host, dev)
    torch.cuda.synchronize()
    return batch, [s[PLAN] for s in samples], carried


@pytest.fixture(scope="module")
def gold():
    return np.load(HM.GOLD)


@pytest.fixture(scope="module")
def runs(dev):
    """every (chain, mirror) batch once, masked and with masks of ones: shared by the tests below, left unchanged"""
    out = {}
    for kind, inputs in (("resize", HM.resize_inputs()), ("warp", HM.warp_inputs())):
        for mirror in (False, True):
            out[kind, mirror] = (_run(dev, kind, mirror, inputs), _run(dev, kind, mirror, inputs, ones=True))
    return out


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_kernels_match_the_reference_vectors(runs, gold, kind, mirror):
    (batch, plans, carried), _ = runs[kind, mirror]
    pm = batch["patched_mask"]
    n = len(plans)
    H, W = (HM.RESIZE_SIZE if kind == "resize" else (HM.WARP_OUT_H, HM.WARP_OUT_W))
    assert carried and pm.dtype == torch.float64 and pm.is_contiguous() and pm.shape == (n, H, W)
    assert all(p["mirror"] == mirror for p in plans)
    for b in range(n):
        want = gold["%s%d_m%d" % (kind, b, mirror)]
        assert (want == 0).any() and (want == 1).any()
        assert np.array_equal(pm[b].cpu().numpy(), want), (kind, mirror, b)
        if kind == "warp":
            assert np.array_equal(plans[b]["warp"]["M"], gold["warp%d_M" % b])


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_the_plane_leaves_the_frames_alone(runs, kind, mirror):
    (masked, _, _), (plain, _, carried) = runs[kind, mirror]
    assert not carried                                    # masks of ones: the launch without a plane
    for i in HM.FRAME_IDXS:
        for fam in ("image", "original_image"):
            assert torch.equal(masked[(fam, i)], plain[(fam, i)]), (fam, i)
    assert torch.equal(masked["P2"], plain["P2"])
    assert not torch.equal(masked["patched_mask"], plain["patched_mask"])


@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_an_explicit_plane_of_ones_equals_the_null_path(dev, runs, kind):
    """the launch without a plane synthesises the mask from coordinates; a uint8 plane of ones (what a mixed batch
    carries for its unmasked samples) read by the masked launch gives the same tensors"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, DeviceAugment
    inputs = HM.resize_inputs() if kind == "resize" else HM.warp_inputs()
    _, (plain, _, _) = runs[kind, True]
    t = _build(HM.train_cfg(kind, True))
    aug = DeviceAugment(HM.FRAME_IDXS)
    host = aug.collate([t(HM.sample_dict(f, np.ones(m.shape))) for f, m in inputs])
    assert "mask_src" not in host[PLAN]
    src = host[PLAN]["src"]
    plane = torch.zeros(src.shape[0], src.shape[2], src.shape[3], dtype=torch.uint8)
    for b, (_, m) in enumerate(inputs):
        plane[b, :m.shape[0], :m.shape[1]] = 1
    host[PLAN]["mask_src"] = plane
    got = aug.materialize(host, dev)
    torch.cuda.synchronize()
    assert torch.equal(got["patched_mask"], plain["patched_mask"])
    for i in HM.FRAME_IDXS:
        assert torch.equal(got[("image", i)], plain[("image", i)])
        assert torch.equal(got[("original_image", i)], plain[("original_image", i)])


@pytest.mark.parametrize("mirror", [False, True])
def test_patched_mask_and_motion_mask_together_on_the_warp_chain(dev, mirror):
    inputs = HM.warp_inputs()
    rs = np.random.RandomState(77)
    motion = [(rs.rand(*m.shape) > 0.5).astype(np.uint8) for _, m in inputs]
    batch, plans, carried = _run(dev, "warp", mirror, inputs, gt_image_keys=('patched_mask', 'motion_mask'),
                                 extra=[dict(motion_mask=m) for m in motion])
    assert carried and batch["motion_mask"].dtype == torch.float32
    for b, (_, mask) in enumerate(inputs):
        M = plans[b]["warp"]["M"]
        assert np.array_equal(batch["patched_mask"][b].cpu().numpy(), HM.expect_warp(mask, M, mirror)), b
        assert np.array_equal(batch["motion_mask"][b].cpu().numpy(),
                              HM.expect_warp(motion[b], M, mirror).astype(np.float32)), b


def test_inconsistent_arguments_are_refused(dev):
    """what the wrappers can see on the host; nothing here launches a read outside a buffer — the per-sample extents
    live in device memory, and there the kernels clamp the mask index to the plane (plans are valid below)"""
    from fsnet_amd.hip.binding import FsAugArgs, FsResizeArgs, lib, stream_ptr
    B, F, Hs, Ws, H, W = 1, 1, 8, 12, 6, 10
    src = torch.zeros(B, F, Hs, Ws, 3, dtype=torch.uint8, device=dev)
    plane = torch.ones(B, Hs, Ws, dtype=torch.uint8, device=dev)
    image = torch.empty(F, B, 3, H, W, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.float64, device=dev)
    dims = torch.tensor([[Hs, Ws, H, W]], dtype=torch.int32, device=dev)
    minv = torch.tensor([[1, 0, 0, 0, 1, 0]], dtype=torch.float64, device=dev)
    iplan = torch.tensor([[3, 3, 3, 0, 0, Hs, Ws, 0]], dtype=torch.int32, device=dev)
    fplan = torch.zeros(B, 4, device=dev)

    def resize_args(**kw):
        r = FsResizeArgs()
        r.src, r.dims, r.image, r.mask = src.data_ptr(), dims.data_ptr(), image.data_ptr(), mask.data_ptr()
        r.B, r.F, r.Hs, r.Ws, r.H, r.W = B, F, Hs, Ws, H, W
        for k in range(3):
            r.std[k] = 1.0
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def warp_args(**kw):
        a = FsAugArgs()
        a.src, a.minv, a.iplan, a.fplan = src.data_ptr(), minv.data_ptr(), iplan.data_ptr(), fplan.data_ptr()
        a.image, a.mask = image.data_ptr(), mask.data_ptr()
        a.B, a.F, a.Hs, a.Ws, a.H, a.W = B, F, Hs, Ws, H, W
        for k in range(3):
            a.std[k] = 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    mp, st = plane.data_ptr(), stream_ptr()
    for bad in (dict(Hs=0), dict(Ws=0), dict(Hs=-3), dict(mask=None)):
        assert lib.fs_resize_frames_masked(C.byref(resize_args(**bad)), mp, st) == 1, bad      # FS_EINVAL
        assert lib.fs_augment_frames_masked(C.byref(warp_args(**bad)), mp, st) == 1, bad
    assert lib.fs_resize_frames_masked(C.byref(resize_args()), None, st) == 1                  # no plane
    assert lib.fs_augment_frames_masked(C.byref(warp_args()), None, st) == 1
    mask.fill_(-1.0)
    assert lib.fs_resize_frames_masked(C.byref(resize_args()), mp, st) == 0
    torch.cuda.synchronize()
    assert bool((mask == 1).all())                        # a plane of ones, 8 x 12 resized to the whole 6 x 10
    mask.fill_(-1.0)
    assert lib.fs_augment_frames_masked(C.byref(warp_args()), mp, st) == 0
    torch.cuda.synchronize()
    assert bool((mask == 1).all())                        # identity warp of a plane of ones, 6 x 10 of 8 x 12


# ---- into training ---------------------------------------------------------------------------------------------------
def _model(dev, H, W, lr):
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    cfg = meta_arch_cfg(H, W, with_pose=False)            # MonoDepthWPose, R18
    cfg["head_cfg"]["overlapped_mask"] = False            # as in configs/nusc_wpose_example
    torch.manual_seed(0)
    m = _build(cfg).to(dev).train()
    tc = training_cfg(lr=lr)
    return m, build_optimizer(m, **tc.optimizer), tc


@pytest.fixture
def fp32():
    from fsnet_amd.engine.runtime import RT
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    yield
    RT.tie_noise = True
    RT.set_compute_dtype(torch.bfloat16)


def test_nusc_json_dataset_into_eager_and_captured_steps(dev, tmp_path, fp32):
    """NusceneJsonDataset (CAM_BACK cut lowered to the tree's frames) -> the nusc config's training augmentation ->
    DeviceAugment -> MonoDepthWPose: one BaseTrainingHook step eager, one from the captured graph"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from tests import helpers_nusc as HN
    H, W = 64, 128
    tree = HN.make_tree(str(tmp_path))
    ds = HM.small_nusc_dataset(tree["json_train"], (H, W))
    np.random.seed(4)
    aug = DeviceAugment(HM.FRAME_IDXS)
    batch = aug.materialize(aug.collate([ds[i] for i in range(6)]), dev)          # six cameras, CAM_BACK among them
    pm = batch["patched_mask"]
    assert pm.dtype == torch.float64 and pm.shape == (6, H, W)
    rows = [int((pm[b].sum(1) > 0).sum()) for b in range(6)]       # 24 x 40 -> 64 x 107, pad_1
    assert rows == [64, 64, 64, 43, 64, 64], rows         # CAM_BACK: floor(d * 0.375) >= 16 from row 43 on
    assert [int(pm[b].sum()) for b in range(6)] == [r * 107 for r in rows]
    m, opt, tc = _model(dev, H, W, lr=1e-4)
    for use_graph, calls in ((False, 1), (True, 3)):      # the third call of a graph hook captures and replays
        hook = _build(dict(use_graph=use_graph, graph_warmup=2, **tc.training_hook))
        for _ in range(calls):
            out = hook(dict(batch), m, opt)
        torch.cuda.synchronize()
        assert hook.graph_captures == (1 if use_graph else 0)
        assert out["loss_dict"] and all(bool(torch.isfinite(v).all()) for v in out["loss_dict"].values())
        assert bool(torch.isfinite(out["loss"]))


def test_the_mask_is_a_live_input_of_the_captured_step(dev, fp32):
    """two batches that differ only in the mask — ones, and the lower third zero — over frames whose lower third is
    noise: the masked loss is the small one.  The captured step, replayed on either batch, lands on that batch's own
    eager value (the learning rate is ~0, so the weights stand still and every step of a batch is the same step)."""
    H, W = 64, 128
    h, w = 48, 96
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:h, 0:w]
    inputs = []
    for b in range(2):
        frames = []
        for k in range(3):
            tex = 128 + 60 * np.sin((xx + 2 * k) / (5.0 + b)) * np.cos(yy / 7.0)          # smooth, shifted per frame
            f = np.repeat(tex[:, :, None], 3, axis=2)
            f[32:] = rs.randint(0, 256, size=(h - 32, w, 3))                              # the car's own body: noise
            frames.append(np.clip(f, 0, 255).astype(np.uint8))
        mask = np.ones((h, w)); mask[32:] = 0
        inputs.append((frames, mask))

    def batch_of(ones):
        from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
        t = _build(HM.train_cfg("resize", False, size=(H, W)))
        aug = DeviceAugment(HM.FRAME_IDXS)
        samples = []
        for frames, mask in inputs:
            d = HM.sample_dict(frames, np.ones(mask.shape) if ones else mask)
            d['P2'] = np.array([[100.0, 0, 48.0, 0], [0, 100.0, 24.0, 0], [0, 0, 1, 0]])
            for i in HM.FRAME_IDXS[1:]:
                d[('relative_pose', i)][2, 3] = -0.3 * i
            samples.append(t(d))
        return aug.materialize(aug.collate(samples), dev)

    plain, masked = batch_of(True), batch_of(False)
    assert set(plain) == set(masked)
    for k in plain:
        same = torch.equal(plain[k], masked[k])
        assert same == (k != "patched_mask"), k
    m, opt, tc = _model(dev, H, W, lr=1e-12)
    eager = _build(dict(use_graph=False, **tc.training_hook))
    l_plain = float(eager(dict(plain), m, opt)["loss_dict"]["loss/0"])
    l_masked = float(eager(dict(masked), m, opt)["loss_dict"]["loss/0"])
    print("eager loss/0: ones %.6f, lower third masked %.6f" % (l_plain, l_masked))
    assert l_masked > 0 and l_plain >= 2 * l_masked, (l_plain, l_masked)          # the test's own precondition
    hook = _build(dict(use_graph=True, graph_warmup=2, **tc.training_hook))
    hook(dict(plain), m, opt)
    hook(dict(plain), m, opt)
    got = []
    for batch, want in ((plain, l_plain), (masked, l_masked), (plain, l_plain), (masked, l_masked)):
        got.append((float(hook(dict(batch), m, opt)["loss_dict"]["loss/0"]), want))
    torch.cuda.synchronize()
    print("replayed loss/0 (got, eager):", got)
    assert hook.graph_captures == 1 and hook.graph_replays == 3
    for g, want in got:
        assert abs(g - want) <= 0.1 * want, got
