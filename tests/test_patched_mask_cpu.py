"""A patched_mask that is not all ones on the host side of the device input pipeline: the expected-mask composition
against the reference's vectors, what Resize / RandomWarpAffine record and refuse, what collate carries, and the
nuScenes JSON dataset (CAM_BACK zeroes the car's own body) through the nusc config's training augmentation."""
import numpy as np
import pytest

from tests import helpers_patched_mask as HM


@pytest.fixture(scope="module")
def gold():
    return np.load(HM.GOLD)


def _build(cfg):
    from fsnet_amd.vision_base.utils.builder import build
    return build(**cfg)


def _plan(sample):
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    return sample[PLAN]


@pytest.mark.parametrize("mirror", [False, True])
def test_composition_equals_the_reference_vectors(gold, mirror):
    assert str(gold["dtype"]) == "float64"
    for n, (_, mask) in enumerate(HM.resize_inputs()):
        want = gold["resize%d_m%d" % (n, mirror)]
        got = HM.expect_resize(mask, mirror)
        assert got.dtype == np.float64 and got.shape == HM.RESIZE_SIZE
        assert np.array_equal(got, want), n
    inputs = HM.warp_inputs()
    Ms = HM.warp_matrices([m.shape for _, m in inputs])
    for n, (_, mask) in enumerate(inputs):
        assert np.array_equal(Ms[n], gold["warp%d_M" % n])
        got = HM.expect_warp(mask, Ms[n], mirror)
        assert got.dtype == np.float64 and np.array_equal(got, gold["warp%d_m%d" % (n, mirror)]), n


def test_cases_hit_the_branches_they_are_meant_to(gold):
    eff = [tuple(int(v) for v in gold["resize%d_effective" % n]) for n in range(4)]
    assert eff == [(36, 60), (32, 64), (36, 58), (36, 60)]
    m0, m1, m2 = (gold["resize%d_m0" % n] for n in range(3))
    assert not m0[:, 60:].any() and m0[:28, :60].all() and not m0[28:, :60].any()      # 70 / 2.5 = 28 rows of ones
    assert not m1[32:, :].any() and m1[:25].all() and not m1[25:32].any()            # floor(24 * 2.5) = 60 < 62
    assert m2[:, :58].all() and not m2[:, 58:].any()
    assert np.array_equal(gold["resize0_m1"], m0[:, ::-1])
    # the real case: 900 x 1600 with rows 700+ zero -> 288 x 512 keeps the cut exact
    real = np.ones((900, 1600)); real[700:] = 0
    out = HM.expect_resize(real, False, size=(288, 512))
    assert out[:224].all() and not out[224:].any()


@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_masked_samples_are_accepted_and_recorded(kind):
    inputs = HM.resize_inputs() if kind == "resize" else HM.warp_inputs()
    t = _build(HM.train_cfg(kind, False))
    for frames, mask in inputs:
        data = HM.sample_dict(frames, mask)
        s = t(data)
        rec = _plan(s).get("patched_mask")
        if mask.all():
            assert rec is None
        else:
            assert rec.dtype == np.uint8 and np.array_equal(rec, mask)
        assert s['patched_mask'].dtype == np.float64 and np.array_equal(s['patched_mask'], mask)   # the entry stays


@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_a_single_zero_off_the_lattice_is_recorded(kind):
    frames, _ = HM.warp_inputs()[0]
    mask = np.ones(frames[0].shape[:2])
    mask[3, 5] = 0
    s = _build(HM.train_cfg(kind, False))(HM.sample_dict(frames, mask))
    rec = _plan(s).get("patched_mask")
    assert rec is not None and rec[3, 5] == 0 and int(rec.sum()) == rec.size - 1


@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_other_values_and_other_sizes_are_refused(kind):
    frames, _ = HM.warp_inputs()[0]
    h, w = frames[0].shape[:2]
    half = np.ones((h, w)); half[40, 41] = 0.5
    with pytest.raises(NotImplementedError, match="values in"):
        _build(HM.train_cfg(kind, False))(HM.sample_dict(frames, half))
    with pytest.raises(NotImplementedError, match="frame's size"):
        _build(HM.train_cfg(kind, False))(HM.sample_dict(frames, np.ones((h - 1, w))))
    zeros_small = np.zeros((h, w - 2))
    with pytest.raises(NotImplementedError, match="frame's size"):
        _build(HM.train_cfg(kind, False))(HM.sample_dict(frames, zeros_small))


@pytest.mark.parametrize("kind", ["resize", "warp"])
def test_collate_of_ones_carries_no_plane_and_a_mixed_batch_one(kind):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    inputs = HM.resize_inputs() if kind == "resize" else HM.warp_inputs() + [
        (HM.make_frames((84, 150), 7), np.ones((84, 150)))]           # a ragged, unmasked batch-mate
    aug = DeviceAugment(HM.FRAME_IDXS)
    t = _build(HM.train_cfg(kind, False))
    ones = aug.collate([t(HM.sample_dict(f, np.ones(m.shape))) for f, m in inputs])
    assert "mask_src" not in ones[PLAN]
    t = _build(HM.train_cfg(kind, False))
    mixed = aug.collate([t(HM.sample_dict(f, m)) for f, m in inputs])
    plane = mixed[PLAN]["mask_src"]
    src = mixed[PLAN]["src"]
    assert plane.dtype.is_floating_point is False and plane.element_size() == 1
    assert tuple(plane.shape) == (src.shape[0], src.shape[2], src.shape[3])
    for b, (_, m) in enumerate(inputs):
        h, w = m.shape
        assert np.array_equal(plane[b, :h, :w].numpy(), m.astype(np.uint8))          # ones for the unmasked sample
        assert not plane[b, h:].any() and not plane[b, :, w:].any()                  # zero-padded like the frames
    # everything else in the plan is what the all-ones batch carries
    for key, val in ones[PLAN].items():
        got = mixed[PLAN][key]
        same = np.array_equal(np.asarray(val), np.asarray(got)) if hasattr(val, "shape") else val == got
        assert same, key


def test_nusc_json_dataset_plans_a_mask_for_cam_back_only(tmp_path):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    from tests import helpers_nusc as HN
    tree = HN.make_tree(str(tmp_path))
    ds = HM.small_nusc_dataset(tree["json_train"], (64, 128))
    np.random.seed(11)
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) == 12
    back = 0
    for s in samples:
        rec = s[PLAN].get("patched_mask")
        if s['camera_type'] == 'CAM_BACK':
            back += 1
            assert rec is not None and rec[:HM.BACK_ROW].all() and not rec[HM.BACK_ROW:].any()
        else:
            assert rec is None
    assert back == 2
    batch = DeviceAugment(HM.FRAME_IDXS).collate(samples[:6])          # the six cameras of one sample
    plane = batch[PLAN]["mask_src"]
    assert tuple(plane.shape) == (6, HN.H, HN.W) and int(plane[3].sum()) == HM.BACK_ROW * HN.W
    assert all(bool(plane[b].all()) for b in (0, 1, 2, 4, 5))


def test_the_masked_entry_points_refuse_before_any_launch():
    """FS_EINVAL comes back from the wrappers' host checks: nothing is launched, the pointers are never followed"""
    import ctypes as C
    from fsnet_amd.hip.binding import FsAugArgs, FsResizeArgs, lib
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    r = FsResizeArgs()
    r.src = r.dims = r.image = p
    r.B, r.F, r.Hs, r.Ws, r.H, r.W = 1, 1, 2, 2, 2, 2
    a = FsAugArgs()
    a.src = a.minv = a.iplan = a.fplan = a.image = p
    a.B, a.F, a.Hs, a.Ws, a.H, a.W = 1, 1, 2, 2, 2, 2
    for k in range(3):
        r.std[k] = a.std[k] = 1.0
    assert lib.fs_resize_frames_masked(None, p, None) == 1 and lib.fs_augment_frames_masked(None, p, None) == 1
    assert lib.fs_resize_frames_masked(C.byref(r), p, None) == 1          # a plane and no mask output
    assert lib.fs_augment_frames_masked(C.byref(a), p, None) == 1
    r.mask = a.mask = p
    assert lib.fs_resize_frames_masked(C.byref(r), None, None) == 1       # a mask output and no plane
    assert lib.fs_augment_frames_masked(C.byref(a), None, None) == 1
    r.Hs = a.Ws = 0
    assert lib.fs_resize_frames_masked(C.byref(r), p, None) == 1
    assert lib.fs_augment_frames_masked(C.byref(a), p, None) == 1
