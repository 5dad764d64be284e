"""The remaining augmentation classes without a GPU: they build by their reference names, and their draws, P2 / pose
bookkeeping, window composition and refusals are held against tests/golden/augment_ext.npz (the reference's own classes
over the chains of tests/helpers_augment_ext.py) and against numpy."""
import numpy as np
import pytest
import torch

from tests import helpers_augment_ext as HX

AUG = HX.OURS


def _build(steps, common=None):
    from fsnet_amd.vision_base.utils.builder import build
    return build(**HX.cfg(steps, common))


def _samples(g, tag):
    """the case's four samples through fsnet_amd's host classes -> (samples, next value of the global stream)"""
    c = HX.case(tag)
    np.random.seed(c["build_seed"])
    transform = _build(c["steps"], c["common"])
    np.random.seed(int(g["%s_global_seed" % tag]))
    out = [transform(HX.sample(tag, n, int(g["%s_frame_seed" % tag]))) for n in range(len(HX.SIZES))]
    return out, np.random.rand()


@pytest.fixture(scope="module")
def golden():
    return np.load(HX.GOLD)


@pytest.mark.parametrize("name,kwargs", [
    ("CropTop", dict(crop_top_index=3)), ("CropRight", dict(output_width=5)), ("Pad2Shape", dict(target_shape=(4, 4))),
    ("RandomCropToWidth", dict(width=8)), ("RandomHue", dict(distort_prob=1.0)), ("RandomEigenvalueNoise", {}),
    ("PhotometricDistort", {}), ("Copy", dict(from_keys=[('image', 0)], to_keys=[('original_image', 0)]))])
def test_every_new_class_builds_by_its_reference_name(name, kwargs):
    from fsnet_amd.vision_base.utils.builder import build
    obj = build(name=AUG + '.' + name, **kwargs)
    assert type(obj).__name__ == name and callable(obj)


def test_random_crop_to_width_takes_no_unknown_keyword():
    from fsnet_amd.vision_base.utils.builder import build
    with pytest.raises(TypeError):
        build(name=AUG + '.RandomCropToWidth', width=8, object_keys=[])


@pytest.mark.parametrize("tag", HX.CASES)
def test_host_bookkeeping_matches_reference_vectors(golden, tag):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    g = golden
    samples, nxt = _samples(g, tag)
    assert nxt == float(g["%s_next" % tag])                    # the chain consumed the global stream as the reference
    for n, s in enumerate(samples):
        pre = "%s%d_" % (tag, n)
        assert isinstance(s["P2"], torch.Tensor) and np.array_equal(s["P2"].numpy(), g[pre + "P2"]), (tag, n)
        for j, i in enumerate(HX.FRAME_IDXS[1:]):
            assert np.array_equal(np.asarray(s[("relative_pose", i)], dtype=np.float32), g[pre + "pose_%d" % j])
        for key in ("original_shape", "effective_size"):
            assert ((pre + key) in g.files) == (("image_resize", key) in s)
            if ("image_resize", key) in s:
                assert list(s[("image_resize", key)]) == list(g[pre + key])
        assert s[("image", 0)].dtype == np.uint8                # pixels untouched on the host
    batch = DeviceAugment(HX.FRAME_IDXS).collate(samples)
    assert tuple(batch[PLAN]["out_hw"]) == HX.case(tag)["out_hw"] == g["%s0_image_0" % tag].shape[1:]


def _brute_force_window(canvas_hw, steps):
    """index arrays through the post-resampling steps: canvas x / y index of every output pixel, -1 where padded"""
    H, W = canvas_hw
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for kind, arg in steps:
        if kind == "top":
            ys, xs = ys[arg:], xs[arg:]
        elif kind == "cols":
            ys, xs = ys[:, arg[0]:arg[1]], xs[:, arg[0]:arg[1]]
        elif kind == "mirror":
            ys, xs = ys[:, ::-1], xs[:, ::-1]
        elif kind == "pad":
            pads = [(0, arg[0] - ys.shape[0]), (0, arg[1] - ys.shape[1])]
            ys, xs = np.pad(ys, pads, constant_values=-1), np.pad(xs, pads, constant_values=-1)
    return ys, xs


def test_window_rows_equal_a_brute_force_composition(golden):
    """case c: Resize -> CropTop -> RandomCropToWidth -> RandomMirror -> Pad2Shape -> RandomMirror"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    g = golden
    samples, _ = _samples(g, "c")
    # the crop's left edge, from the same point of the global stream
    np.random.seed(int(g["c_global_seed"]))
    seen = set()
    rows = DeviceAugment(HX.FRAME_IDXS).collate([dict(s) for s in samples])[PLAN]["win"].numpy()
    for n, s in enumerate(samples):
        left = np.random.randint(0, HX.OUT_W - 42)
        m1, m2 = bool(np.random.rand() <= 0.5), bool(np.random.rand() <= 0.5)
        assert [m1, m2] == list(g["c_mirrors"][n])
        steps = [("top", 2), ("cols", (left, left + 42))] + [("mirror", None)] * m1 + [("pad", (17, 45))] + [("mirror", None)] * m2
        ys, xs = _brute_force_window((HX.OUT_H, HX.OUT_W), steps)
        flip, x_off, y_off, vx0, vy0, vx1, vy1, _ = (int(v) for v in rows[n])
        yo, xo = np.meshgrid(np.arange(17), np.arange(45), indexing="ij")
        valid = (xo >= vx0) & (xo < vx1) & (yo >= vy0) & (yo < vy1)
        assert np.array_equal(valid, ys >= 0)
        assert np.array_equal(np.where(valid, x_off - xo if flip else x_off + xo, -1), xs)
        assert np.array_equal(np.where(valid, y_off + yo, -1), ys)
        seen.add((m1, m2))
    assert len(seen) >= 3 and any(m2 for _, m2 in seen)          # zeros on the left occur


def _frames(h=20, w=30, seed=0):
    rs = np.random.RandomState(seed)
    d = {('image', 0): rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8), 'P2': np.eye(3, 4)}
    d[('original_image', 0)] = d[('image', 0)].copy()
    return d


K = dict(image_keys=[('image', 0)])


def test_named_refusals():
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    first = [dict(op='ConvertToFloat')]
    bright = dict(op='RandomBrightness', distort_prob=1.0, random_seed=1)
    hsv, rgb = dict(op='ConvertColor', transform='HSV'), dict(op='ConvertColor', current='HSV', transform='RGB')
    with pytest.raises(NotImplementedError, match="after a colour op"):
        _build(first + [bright, dict(op='Pad2Shape', target_shape=(40, 40))], K)(_frames())
    with pytest.raises(ValueError, match="smaller than the 20 x 30 image"):
        _build(first + [dict(op='Pad2Shape', target_shape=(40, 29))], K)(_frames())
    with pytest.raises(ValueError, match="empty image"):
        _build(first + [dict(op='CropTop', crop_top_index=20)], K)(_frames())
    with pytest.raises(ValueError, match="empty image"):       # after a resampling stage too
        _build(first + [dict(op='Resize', size=(8, 12)), dict(op='CropTop', crop_top_index=8)], K)(_frames())
    with pytest.raises(NotImplementedError, match="copies"):
        _build(first + [dict(op='Copy', from_keys=[('image', 0)], to_keys=[('image', 1)])], K)(_frames())
    with pytest.raises(NotImplementedError, match="copies"):
        _build(first + [dict(op='Copy', from_keys=[('image', 0)], to_keys=[('original_image', 1)])], K)(_frames())
    copy = dict(op='Copy', from_keys=[('image', 0)], to_keys=[('original_image', 0)])
    with pytest.raises(NotImplementedError, match="inside an HSV section"):
        _build(first + [hsv, copy, rgb], K)(_frames())
    hue = dict(op='RandomHue', distort_prob=1.0, random_seed=2)
    with pytest.raises(NotImplementedError, match="no RandomHue yet"):
        _build(first + [hsv, hue, dict(hue), rgb], K)(_frames())
    with pytest.raises(NotImplementedError, match="inside an HSV section"):
        _build(first + [hue], K)(_frames())
    nine = _build(first + [dict(bright) for _ in range(9)], K)(_frames())
    with pytest.raises(NotImplementedError, match="more than 8"):
        DeviceAugment([0]).collate([nine])
    noise = dict(op='RandomEigenvalueNoise', random_seed=3)
    with pytest.raises(NotImplementedError, match="8-bit, 16-bit and 32-bit float"):
        _build(first + [noise, hsv, rgb], K)(_frames())
    # a noise op whose draw missed leaves the image float32: the conversion is fine
    _build(first + [dict(noise, distort_prob=-1.0), hsv, rgb], K)(_frames())


def test_random_crop_to_width_edges():
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    with pytest.raises(ValueError):                              # numpy's own: randint(0, 0)
        _build([dict(op='RandomCropToWidth', width=30)], K)(_frames())
    d = _frames()
    before = {k: v.copy() for k, v in d.items()}
    state = np.random.get_state()
    out = _build([dict(op='RandomCropToWidth', width=31)], dict(K, calib_keys=['P2']))(d)
    assert all(np.array_equal(out[k], before[k]) for k in before) and out[('image', 0)].shape == (20, 30, 3)
    assert np.random.get_state()[2] == state[2] and out[PLAN].get("win") is None       # nothing drawn, nothing planned
    np.random.seed(4)
    out = _build([dict(op='RandomCropToWidth', width=12)], dict(K, calib_keys=['P2']))(_frames())
    np.random.seed(4)
    left = np.random.randint(0, 18)
    assert np.array_equal(out[('image', 0)], _frames()[('image', 0)][:, left:left + 12])
    assert np.shares_memory(out[('image', 0)], out[('image', 0)].base)                  # a view, no copy
    assert out['P2'][0, 2] == -left and out['P2'][0, 3] == 0


def test_crop_right_against_numpy_slicing():
    """the reference's CropRight cannot be called (its __init__ drops image_keys): numpy slicing is the yardstick"""
    ref = _frames()[('image', 0)]
    out = _build([dict(op='CropRight', crop_right_index=7)], K)(_frames())
    assert np.array_equal(out[('image', 0)], ref[:, 0:30 - 7]) and np.array_equal(out['P2'], np.eye(3, 4))
    out = _build([dict(op='CropRight', output_width=11)], K)(_frames())
    assert np.array_equal(out[('image', 0)], ref[:, 0:11])
    out = _build([dict(op='CropRight', crop_right_index=4, output_width=11)], K)(_frames())        # the index wins
    assert np.array_equal(out[('image', 0)], ref[:, 0:26])
    out = _build([dict(op='CropRight')], K)(_frames())                                               # crops 0
    assert np.array_equal(out[('image', 0)], ref)
    out = _build([dict(op='CropRight', output_width=31)], K)(_frames())                              # would widen
    assert np.array_equal(out[('image', 0)], ref)
    m = np.arange(600, dtype=np.uint8).reshape(20, 30)
    d = dict(_frames(), motion_mask=m)
    out = _build([dict(op='CropRight', output_width=9)], dict(K, gt_image_keys=['motion_mask']))(d)
    assert np.array_equal(out['motion_mask'], m[:, :9])
    # after a resampling stage it moves the window instead
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, window_row
    out = _build([dict(op='ConvertToFloat'), dict(op='Resize', size=(8, 12), preserve_aspect_ratio=False),
                  dict(op='CropRight', crop_right_index=5)], K)(_frames())
    assert out[('image', 0)].shape == (20, 30, 3) and window_row(out[PLAN]["win"]) == [0, 0, 0, 0, 0, 7, 8, 0]


def test_crop_top_quirks():
    P = np.array([[7.0, 0, 3, 1], [0, 7, 4, 2], [0, 0, 1, 0.5]])
    out = _build([dict(op='CropTop')], dict(K, calib_keys=['P2']))(dict(_frames(), P2=P.copy()))     # crops 0
    assert out[('image', 0)].shape == (20, 30, 3) and np.array_equal(out['P2'], P)
    out = _build([dict(op='CropTop', crop_top_index=3, output_height=5)], dict(K, calib_keys=['P2']))(dict(_frames(), P2=P.copy()))
    assert out[('image', 0)].shape == (17, 30, 3) and out['P2'][1, 2] == 1 and out['P2'][1, 3] == 2 - 3 * 0.5
    out = _build([dict(op='CropTop', output_height=5)], K)(_frames())
    assert np.array_equal(out[('image', 0)], _frames()[('image', 0)][15:])


def test_chains_expressible_before_keep_their_launches(golden):
    """case a (a crop before the warp) and case b (a Copy of the unaugmented frame) collate to the plan kinds of the
    launches that existed before; the others need the extended ones"""
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    from tests import helpers_augment as HA
    from fsnet_amd.vision_base.utils.builder import build
    kinds = {}
    for tag in HX.CASES:
        samples, _ = _samples(golden, tag)
        kinds[tag] = DeviceAugment(HX.FRAME_IDXS).collate(samples)[PLAN]["kind"]
    assert kinds == dict(a="warp", b="resize", c="ext", d="ext", e="ext", f="ext")
    g = HA.golden()
    transform = build(**HA.pipeline_cfg(g))
    np.random.seed(int(g["global_seed"]))
    batch = DeviceAugment(HA.FRAME_IDXS).collate([transform(HA.sample_dict(*HA.sample_inputs(g, n))) for n in range(2)])
    assert batch[PLAN]["kind"] == "warp" and "win" not in batch[PLAN]
    g = np.load(HA.GOLD_RESIZE)
    transform = build(**HA.resize_pipeline_cfg(g))
    batch = DeviceAugment(HA.FRAME_IDXS).collate([transform(HA.sample_dict(*HA.resize_sample_inputs(g, 0)))])
    assert batch[PLAN]["kind"] == "resize" and batch[PLAN]["train"] and "win" not in batch[PLAN]


def test_op_list_and_copy_split_of_case_e(golden):
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment, PLAN
    samples, _ = _samples(golden, "e")
    p = DeviceAugment(HX.FRAME_IDXS).collate(samples)[PLAN]
    assert (p["n_ops"], p["split"]) == (5, 4)
    for row in p["codes"].numpy():
        assert list(row) == [0, 2 | 3 << 4, 3, 1, 0, 4, 4, 4]      # brightness, HSV(sat + hue), noise, contrast | brightness
    assert p["vals"].dtype == torch.float64 and p["minv"].shape == (4, 6)
