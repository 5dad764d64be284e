"""The extended input-pipeline launches (fs_augment_frames_ext / fs_resize_frames_ext / fs_augment_masks_ext) on the GPU:
bit for bit against tests/golden/augment_ext.npz (the reference's own classes), against the launches that existed before
on the plans both can express, and against chains run on frames the test cropped or padded itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_augment_ext as HX

pytestmark = pytest.mark.gpu


def _build(steps, common=None):
    from fsnet_amd.vision_base.utils.builder import build
    return build(**HX.cfg(steps, common))


def _samples(g, tag, steps=None):
    c = HX.case(tag)
    np.random.seed(c["build_seed"])
    transform = _build(steps or c["steps"], c["common"])
    np.random.seed(int(g["%s_global_seed" % tag]))
    return [transform(HX.sample(tag, n, int(g["%s_frame_seed" % tag]))) for n in range(len(HX.SIZES))]


@pytest.fixture(scope="module")
def golden():
    return np.load(HX.GOLD)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("tag", HX.CASES)
def test_cases_match_reference_vectors(dev, golden, tag):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    g = golden
    batch = DeviceAugment(HX.FRAME_IDXS)(_samples(g, tag), dev)
    torch.cuda.synchronize()
    H, W = HX.case(tag)["out_hw"]
    assert batch[("image", 0)].shape == (len(HX.SIZES), 3, H, W) and batch["patched_mask"].dtype == torch.float64
    padded = 0
    for n in range(len(HX.SIZES)):
        pre = "%s%d_" % (tag, n)
        for j, i in enumerate(HX.FRAME_IDXS):
            if pre + "image_%d" % j not in g.files:
                continue                                              # case f stores frame 0: c holds its pixels
            assert torch.equal(batch[("image", i)][n], _t(g[pre + "image_%d" % j], dev)), (tag, n, i)
            assert torch.equal(batch[("original_image", i)][n], _t(g[pre + "orig_%d" % j], dev)), (tag, n, i)
        assert torch.equal(batch["patched_mask"][n], _t(g[pre + "mask"].astype(np.float64), dev)), (tag, n)
        padded += int((g[pre + "mask"] == 0).any())
        if tag == "f":
            assert torch.equal(batch["motion_mask"][n], _t(g[pre + "motion_mask"].astype(np.float32), dev)), n
        assert torch.equal(batch["P2"][n], _t(g[pre + "P2"], dev))
    if tag in ("b", "c", "f"):
        assert padded == len(HX.SIZES)


def _assert_same(got, want):
    for key in [("image", i) for i in HX.FRAME_IDXS] + [("original_image", i) for i in HX.FRAME_IDXS] + ["patched_mask"]:
        assert torch.equal(got[key], want[key]), key


def test_crop_before_the_warp_equals_the_chain_on_sliced_frames(dev, golden):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    c = HX.case("a")
    got = DeviceAugment(HX.FRAME_IDXS)(_samples(golden, "a"), dev)
    plain = [s for s in c["steps"] if s['op'] != 'CropTop']
    np.random.seed(c["build_seed"])
    transform = _build(plain, dict(c["common"], calib_keys=[]))
    np.random.seed(int(golden["a_global_seed"]))
    samples = []
    for n in range(len(HX.SIZES)):
        d = HX.sample("a", n, int(golden["a_frame_seed"]))
        for key in HX.IMGS + HX.ORIGS + ['patched_mask']:
            d[key] = np.ascontiguousarray(d[key][11:])
        samples.append(transform(d))
    want = DeviceAugment(HX.FRAME_IDXS)(samples, dev)
    torch.cuda.synchronize()
    _assert_same(got, want)


def test_pad_before_the_resize_equals_the_chain_on_padded_frames(dev):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    tail = [dict(op='Resize', size=(HX.OUT_H, HX.OUT_W), preserve_aspect_ratio=False),
            dict(op='RandomMirror', mirror_prob=0.5, pose_axis_pairs=HX.POSE_PAIRS)] + HX.case("c")["steps"][-3:]
    common = HX.case("c")["common"]
    first = [dict(op='ConvertToFloat')]
    outs = []
    for pad_on_host in (False, True):
        steps = first + ([] if pad_on_host else [dict(op='Pad2Shape', target_shape=(100, 140))]) + tail
        transform = _build(steps, common)
        np.random.seed(11)
        samples = []
        for n in range(len(HX.SIZES)):
            d = HX.sample("f", n, 77)                       # a holed patched_mask; the motion_mask is not in the keys
            del d['motion_mask']
            if pad_on_host:
                h, w = HX.SIZES[n]
                for key in HX.IMGS + HX.ORIGS + ['patched_mask']:
                    d[key] = np.pad(d[key], [(0, 100 - h), (0, 140 - w)] + [(0, 0)] * (d[key].ndim - 2), 'constant')
            samples.append(transform(d))
        batch = DeviceAugment(HX.FRAME_IDXS).collate(samples)
        assert batch[PLAN]["kind"] == ("resize" if pad_on_host else "ext")
        outs.append(DeviceAugment(HX.FRAME_IDXS).materialize(batch, dev))
    torch.cuda.synchronize()
    _assert_same(outs[0], outs[1])
    assert torch.equal(outs[0]["P2"], outs[1]["P2"])
    assert 0.0 < float(outs[0]["patched_mask"].mean()) < 1.0


def _ext_args(plan, dev, keep):
    """FsAugExtArgs over an old-style collated plan (kind warp / resize): full-canvas window, the same ops, split 0"""
    from fsnet_amd.hip.binding import FsAugExtArgs
    src = plan["src"].to(dev)
    B, F, Hs, Ws, _ = src.shape
    H, W = plan["out_hw"]
    iplan, fplan = plan["iplan"].numpy(), plan["fplan"].numpy()
    if plan["kind"] == "warp":
        dims = np.concatenate([iplan[:, 5:7], np.zeros((B, 2), np.int32)], axis=1).astype(np.int32)
    else:
        dims = plan["dims"].numpy()
    win = np.zeros((B, 8), np.int32)
    codes = np.full((B, 8), 4, np.int32)
    vals = np.zeros((B, 8, 3), np.float64)
    for b in range(B):
        win[b] = [1, W - 1, 0, 0, 0, W, H, 0] if iplan[b, 4] else [0, 0, 0, 0, 0, W, H, 0]
        for q in range(3):
            op, applied = int(iplan[b, q]), int(iplan[b, 3])
            if op == 0 and applied & 1:
                codes[b, q], vals[b, q, 0] = 0, fplan[b, 0]
            elif op == 1 and applied & 2:
                codes[b, q], vals[b, q, 0] = 1, fplan[b, 1]
            elif op == 2 and applied & 8:
                codes[b, q], vals[b, q, 0] = 2 | (1 if applied & 4 else 0) << 4, fplan[b, 2]
    t = dict(src=src, dims=_t(dims, dev), win=_t(win, dev), codes=_t(codes, dev), vals=_t(vals, dev),
             image=torch.empty(F, B, 3, H, W, device=dev), original=torch.empty(F, B, 3, H, W, device=dev),
             mask=torch.empty(B, H, W, dtype=torch.float64, device=dev))
    if plan["kind"] == "warp":
        t["minv"] = plan["minv"].to(dev)
    x = FsAugExtArgs()
    x.src, x.dims, x.win, x.ops, x.opv = (t[k].data_ptr() for k in ("src", "dims", "win", "codes", "vals"))
    x.minv = t["minv"].data_ptr() if "minv" in t else None
    x.image, x.original, x.mask = t["image"].data_ptr(), t["original"].data_ptr(), t["mask"].data_ptr()
    for k in range(3):
        x.mean[k], x.std[k] = float(plan["mean"][k]), float(plan["std"][k])
    x.B, x.F, x.Hs, x.Ws, x.H, x.W, x.n_ops, x.split = B, F, Hs, Ws, H, W, 3, 0
    keep.append(t)
    return x, t


@pytest.mark.parametrize("tag", ["a", "b"])
def test_new_launches_equal_the_old_ones_on_plans_both_express(dev, golden, tag):
    """case a's inputs through the warp pair, case b's through the resize pair"""
    from fsnet_amd.hip.binding import lib, check, stream_ptr
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    aug = DeviceAugment(HX.FRAME_IDXS)
    samples = _samples(golden, tag)
    plan = aug.collate([dict(s) for s in samples])[PLAN]
    assert plan["kind"] == ("warp" if tag == "a" else "resize")
    keep = []
    x, t = _ext_args(plan, dev, keep)
    entry = lib.fs_augment_frames_ext if tag == "a" else lib.fs_resize_frames_ext
    check(entry(C.byref(x), stream_ptr()), "ext")
    want = aug(samples, dev)                                         # the launches that existed before
    torch.cuda.synchronize()
    for f, i in enumerate(HX.FRAME_IDXS):
        assert torch.equal(t["image"][f], want[("image", i)]) and torch.equal(t["original"][f], want[("original_image", i)])
    assert torch.equal(t["mask"], want["patched_mask"])
    # one ground-truth plane through the masks entry point of either family
    from fsnet_amd.hip import ops
    B, _, Hs, Ws, _ = plan["src"].shape
    plane = _t(np.random.RandomState(5).randint(0, 2, size=(B, Hs, Ws)).astype(np.uint8), dev)
    H, W = plan["out_hw"]
    iplan = plan["iplan"].to(dev)
    if tag == "a":
        old = ops.augment_masks(plane, H, W, minv=t["minv"], iplan=iplan)
    else:
        old = ops.augment_masks(plane, H, W, dims=plan["dims"].to(dev), iplan=iplan)
    new = ops.augment_masks_ext(plane, H, W, t["dims"], t["win"], minv=t.get("minv"))
    torch.cuda.synchronize()
    assert torch.equal(old, new) and 0.0 < float(new.mean()) < 1.0
    flips = plan["iplan"][:, 4]
    assert 0 < int(flips.sum()) < len(flips)


def test_an_all_padding_window_gives_normalised_zero(dev):
    from fsnet_amd.hip.binding import lib, check, stream_ptr
    plan = dict(kind="resize", src=torch.full((2, 2, 9, 13, 3), 200, dtype=torch.uint8), out_hw=(7, 11),
                dims=torch.tensor([[9, 13, 9, 13]] * 2, dtype=torch.int32), iplan=torch.zeros(2, 8, dtype=torch.int32),
                fplan=torch.zeros(2, 4), mean=HX.MEAN, std=HX.STD)
    plan["iplan"][:, :3] = 3
    keep = []
    for warp in (False, True):
        if warp:
            plan.update(kind="warp", minv=torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 2, dtype=torch.float64))
            plan["iplan"][:, 5], plan["iplan"][:, 6] = 9, 13
        x, t = _ext_args(plan, dev, keep)
        t["win"][:] = torch.tensor([0, 0, 0, 4, 3, 4, 9, 0], dtype=torch.int32)      # vx0 == vx1: nothing is valid
        t["image"].fill_(7.0); t["original"].fill_(7.0); t["mask"].fill_(7.0)
        x.n_ops = 0
        entry = lib.fs_augment_frames_ext if warp else lib.fs_resize_frames_ext
        check(entry(C.byref(x), stream_ptr()), "ext")
        torch.cuda.synchronize()
        zero = (np.zeros(3, np.float32) / np.float32(255.0) - HX.MEAN.astype(np.float32)) / HX.STD.astype(np.float32)
        assert torch.equal(t["image"], _t(zero, dev).view(1, 1, 3, 1, 1).expand_as(t["image"]))
        assert not t["original"].any() and not t["mask"].any()
        # and the full window returns the frame
        t["win"][:] = torch.tensor([0, 0, 0, 0, 0, 11, 7, 0], dtype=torch.int32)
        check(entry(C.byref(x), stream_ptr()), "ext")
        torch.cuda.synchronize()
        frame = float(np.float32(200.0) / np.float32(255.0))             # numpy's true division, as Normalize's
        assert bool((t["mask"] == 1).all()) and torch.equal(t["original"], torch.full_like(t["original"], frame))


def test_no_resampling_chain_returns_the_cropped_frame_exactly(dev, golden):
    """case d's originals are the crop of the raw frame / 255, mirrored where the mirror was drawn"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    samples = _samples(golden, "d")
    raw = [s[("image", 0)].copy() for s in samples]                  # the uint8 views the crops left
    batch = DeviceAugment(HX.FRAME_IDXS)(samples, dev)
    torch.cuda.synchronize()
    for n, frame in enumerate(raw):
        assert frame.shape == (15, 50, 3)
        if golden["d_mirrors"][n][0]:
            frame = frame[:, ::-1]
        want = frame.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
        assert torch.equal(batch[("original_image", 0)][n], _t(want, dev))


def test_case_a_feeds_a_training_step(dev, golden):
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    H, W = 64, 96
    steps = [dict(s, output_w=W, output_h=H) if s['op'] == 'RandomWarpAffine' else s for s in HX.case("a")["steps"]]
    batch = DeviceAugment(HX.FRAME_IDXS)(_samples(golden, "a", steps), dev)
    assert batch[("image", 0)].shape == (4, 3, H, W) and batch["P2"].shape == (4, 3, 4)
    RT.set_compute_dtype(torch.float32)
    try:
        torch.manual_seed(0)
        m = build(**meta_arch_cfg(H, W, with_pose=False)).to(dev).train()
        tc = training_cfg(clip_gradients=35.0, lr=1e-4)
        opt = build_optimizer(m, **tc.optimizer)
        hook = build(use_graph=False, **tc.training_hook)
        loss = float(hook(batch, m, opt)["loss"].detach())
        torch.cuda.synchronize()
        assert np.isfinite(loss)
    finally:
        RT.set_compute_dtype(torch.bfloat16)


def test_invalid_arguments_return_einval():
    """the host checks of the C ABI; no pointer is followed and nothing is launched"""
    from fsnet_amd.hip.binding import lib, FsAugExtArgs

    def args(**kw):
        x = FsAugExtArgs()
        x.src = x.dims = x.win = x.ops = x.opv = x.image = x.original = x.mask = 64
        for k in range(3):
            x.mean[k], x.std[k] = 0.0, 1.0
        x.B, x.F, x.Hs, x.Ws, x.H, x.W, x.n_ops, x.split = 1, 1, 4, 4, 4, 4, 2, 1
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    for entry, minv in ((lib.fs_augment_frames_ext, 64), (lib.fs_resize_frames_ext, None)):
        assert entry(None, None) == 1
        for bad in (dict(src=None), dict(dims=None), dict(win=None), dict(image=None, original=None), dict(B=0),
                    dict(H=-1), dict(Ws=0), dict(n_ops=9, split=0), dict(n_ops=-1), dict(split=3), dict(split=-1),
                    dict(ops=None), dict(opv=None), dict(mask_src=64, mask=None)):
            assert entry(C.byref(args(minv=minv, **bad)), None) == 1, bad
        assert entry(C.byref(args(minv=None if minv else 64)), None) == 1          # minv on the wrong launch
        x = args(minv=minv)
        x.std[2] = 0.0
        assert entry(C.byref(x), None) == 1
    m = lib.fs_augment_masks_ext
    assert m(None, None, 64, 64, 64, 1, 4, 4, 4, 4, None) == 1 and m(64, None, None, 64, 64, 1, 4, 4, 4, 4, None) == 1
    assert m(64, None, 64, None, 64, 1, 4, 4, 4, 4, None) == 1 and m(64, None, 64, 64, None, 1, 4, 4, 4, 4, None) == 1
    assert m(64, None, 64, 64, 64, 0, 4, 4, 4, 4, None) == 1 and m(64, None, 64, 64, 64, 1, 4, 4, 0, 4, None) == 1
    assert m(64, None, 64, 64, 64, 1, 1 << 16, 1 << 15, 4, 4, None) == 1
