"""Motion-mask precompute without a GPU: the Farneback restatement's accuracy (tests/helpers_optflow.py), the
dataset's readers of the precomputed files, the augmentation plans' extra ground-truth keys, the new ABI's refusals
and the new kernels' register budget."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from tests import helpers_kitti as HK
from tests import helpers_optflow as HO

CORRIDOR_EPE = 0.0847 * 1.5      # median EPE of the restatement on corridor_pair(96, 320, seed=1), measured 0.0847


def test_restatement_recovers_subpixel_translation():
    from scipy.ndimage import gaussian_filter, shift, zoom
    rng = np.random.RandomState(3)
    big = gaussian_filter(zoom(rng.rand(27, 43) * 255, 4, order=3), 1.0)
    a = big[:96, :160]
    b = shift(big, (0.3, 0.6), order=3, mode="nearest")[:96, :160]     # content moves +0.6 px in x, +0.3 px in y
    f = HO.farneback(a.astype(np.float32), b.astype(np.float32), **HO.FLOW_CFG)[12:-12, 12:-12]
    epe = np.hypot(f[..., 0] - 0.6, f[..., 1] - 0.3)
    assert epe.max() < 0.05, epe.max()                                  # measured 0.040 (median 0.009)


def test_restatement_corridor_epe():
    img0, img1, P2, T, rigid = HO.corridor_pair(96, 320, seed=1)
    f = HO.farneback(img0, img1, **HO.FLOW_CFG)
    epe = np.median(np.hypot(*(f - rigid).transpose(2, 0, 1)))
    assert epe < CORRIDOR_EPE, epe
    assert np.median(np.hypot(*rigid.transpose(2, 0, 1))) > 10 * CORRIDOR_EPE   # zero flow would be far off


def test_pyramid_plan_levels():
    assert [p[:3] for p in HO.pyramid_plan(96, 320, 0.5, 3)] == [(1, 48, 160), (0, 96, 320)]
    assert [p[0] for p in HO.pyramid_plan(375, 1242, 0.5, 3)] == [3, 2, 1, 0]
    assert HO.pyramid_plan(375, 1242, 0.5, 3)[0][3] == 19                         # ksize of sigma 3.5


def test_png16_round_trip_and_flow_reader(tmp_path):
    from fsnet_amd.monodepth.data.datasets import utils as U
    rng = np.random.RandomState(0)
    img = rng.randint(0, 65536, size=(7, 9, 3)).astype(np.uint16)
    path = str(tmp_path / "f.png")
    U.write_png16(path, img)
    assert np.array_equal(U.read_png16(path), img)
    flow = U.read_flow_png(path)
    assert flow.dtype == np.float32 and flow.shape == (7, 9, 2)
    assert np.array_equal(flow, (img[:, :, [2, 1]].astype(np.float32) - 2 ** 15) / 64.0)


def test_png16_reader_filters(tmp_path):
    """filters 1-4 (what other encoders write) decode like filter 0"""
    import struct
    import zlib
    from fsnet_amd.monodepth.data.datasets import utils as U
    rng = np.random.RandomState(1)
    img = rng.randint(0, 65536, size=(5, 4, 3)).astype(np.uint16)
    rows = img.astype('>u2').reshape(5, -1).view(np.uint8).astype(np.int32)
    enc = []
    for y in range(5):
        ft = y % 5
        prev = rows[y - 1] if y else np.zeros_like(rows[0])
        cur = rows[y]
        left = np.concatenate([np.zeros(6, np.int32), cur[:-6]])
        ul = np.concatenate([np.zeros(6, np.int32), prev[:-6]])
        if ft == 0:
            p = np.zeros_like(cur)
        elif ft == 1:
            p = left
        elif ft == 2:
            p = prev
        elif ft == 3:
            p = (left + prev) >> 1
        else:
            pa, pb, pc = np.abs(prev - ul), np.abs(left - ul), np.abs(left + prev - 2 * ul)
            p = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        enc.append(bytes([ft]) + ((cur - p) & 255).astype(np.uint8).tobytes())

    def chunk(kind, body):
        return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)
    path = str(tmp_path / "g.png")
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 5, 16, 2, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(b''.join(enc))) + chunk(b'IEND', b''))
    assert np.array_equal(U.read_png16(path), img)


def _tree_with_side_products(tmp_path):
    from fsnet_amd.monodepth.data.datasets import utils as U
    raw, split = HK.make_tree(str(tmp_path), seed=5)
    mdir, fdir = tmp_path / "masks", tmp_path / "flow"
    mdir.mkdir()
    fdir.mkdir()
    rng = np.random.RandomState(2)
    masks, flows = [], []
    for i in range(3):                                     # the static filter keeps 3 of the 5 split entries
        m = (rng.rand(HK.H, HK.W) > 0.7).astype(np.uint8)
        Image.fromarray(m).save(str(mdir / ("%08d.png" % i)))
        v = rng.randint(2 ** 15 - 640, 2 ** 15 + 640, size=(HK.H, HK.W, 3)).astype(np.uint16)
        U.write_png16(str(fdir / ("%08d.png" % i)), v)
        masks.append(m)
        flows.append((v[:, :, [2, 1]].astype(np.float32) - 2 ** 15) / 64.0)
    cfg = HK.dataset_cfg(raw, split, prefix='fsnet_amd.')
    cfg.update(is_motion_mask=True, motion_mask_path=str(mdir), is_precompute_flow=True, flow_path=str(fdir))
    return cfg, masks, flows


def test_dataset_reads_motion_mask_and_flow(tmp_path):
    from fsnet_amd.monodepth.data.datasets.mono_dataset import KittiDepthMonoDataset
    cfg, masks, flows = _tree_with_side_products(tmp_path)
    ds = KittiDepthMonoDataset(**cfg)
    assert len(ds) == 3
    for i in range(3):
        s = ds[i]
        assert s["motion_mask"].dtype == np.uint8 and np.array_equal(s["motion_mask"], masks[i])
        assert s["flow"].dtype == np.float32 and np.array_equal(s["flow"], flows[i])


def test_concat_of_several_children_refuses_motion_masks(tmp_path):
    from fsnet_amd.vision_base.data.datasets.dataset_utils import ConcatDataset
    cfg, _, _ = _tree_with_side_products(tmp_path)
    item = dict(cfg, name='fsnet_amd.monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset')
    assert len(ConcatDataset([item])) == 3
    with pytest.raises(ValueError, match="single"):
        ConcatDataset([item, item])


def test_hooks_import():
    from fsnet_amd.monodepth.pipeline_hooks.precomputing_hooks import base_precompute_hooks as P
    from fsnet_amd.vision_base.pipeline_hooks.precomputing_hooks.base_precompute_hooks import BasePrecomputeHook
    assert issubclass(P.MotionMaskPrecomputeHook, BasePrecomputeHook)
    assert issubclass(P.MotionMaskARFlowPrecomputeHook, BasePrecomputeHook)
    assert P.MotionMaskPrecomputeHook.SKIP_EXISTING and not P.MotionMaskARFlowPrecomputeHook.SKIP_EXISTING


def _sample(H=300, W=420, seed=0):
    rng = np.random.RandomState(seed)
    d = {("image", f): rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for f in (0, 1, -1)}
    for f in (0, 1, -1):
        d[("original_image", f)] = d[("image", f)].copy()
    d["patched_mask"] = np.ones([H, W])
    d["motion_mask"] = (rng.rand(H, W) > 0.5).astype(np.uint8)
    d["P2"] = np.array([[300.0, 0, 200, 0], [0, 300, 150, 0], [0, 0, 1, 0]])
    return d


@pytest.mark.parametrize("kind", ["warp", "resize"])
def test_augmentation_plans_carry_extra_gt_key(kind):
    from fsnet_amd.vision_base.data.augmentations import augmentations as A
    keys = [("image", f) for f in (0, 1, -1)] + [("original_image", f) for f in (0, 1, -1)]
    gt = ['patched_mask', 'motion_mask']
    if kind == "warp":
        geo = A.RandomWarpAffine(output_w=256, output_h=96, shift_border=64, image_keys=keys, gt_image_keys=gt,
                                 calib_keys=['P2'], random_seed=1)
    else:
        geo = A.Resize(size=(96, 256), image_keys=keys, gt_image_keys=gt, calib_keys=['P2'])
    chain = [A.ConvertToFloat(image_keys=keys), geo, A.RandomMirror(1.0, image_keys=keys, gt_image_keys=gt),
             A.ConvertToTensor(image_keys=keys, gt_image_keys=gt, calib_keys=['P2'])]
    samples = []
    for seed in (0, 1):
        d = _sample(seed=seed)
        for t in chain:
            d = t(d)
        assert d[A.PLAN]["gt_extra"] == ['motion_mask'] and d["motion_mask"].dtype == np.uint8
        samples.append(d)
    batch = A.DeviceAugment(frame_idxs=(0, 1, -1)).collate(samples)
    src = batch[A.PLAN]["gt"]["motion_mask"]
    assert src.shape == (2, 300, 420) and np.array_equal(src[1].numpy(), samples[1]["motion_mask"])
    assert "motion_mask" not in batch                      # materialize puts the sampled fp32 mask there
    with pytest.raises(TypeError, match="uint8"):
        d = _sample()
        d["motion_mask"] = d["motion_mask"].astype(np.float64)
        for t in chain:
            d = t(d)


def test_flow_parameters_rejected_by_name():
    from fsnet_amd.hip import ops
    good = dict(HO.FLOW_CFG)
    for key, bad in (("poly_n", 6), ("flags", 1), ("flags", 4), ("pyr_scale", 1.0), ("winsize", 0), ("levels", -1),
                     ("iterations", 0), ("poly_sigma", -1.0)):
        with pytest.raises(ValueError, match=key):
            ops._flow_args(1, 64, 64, **dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="mode"):
        ops.motion_mask(None, None, None, 5.0, mode=2)


def test_abi_rejects_invalid_parameters_without_a_gpu():
    import ctypes as C
    from fsnet_amd.hip.binding import FsFlowArgs, FsMotionMaskArgs, lib
    from fsnet_amd.hip import ops
    a = ops._flow_args(2, 96, 320, **HO.FLOW_CFG)
    n = lib.fs_optflow_workspace_bytes(C.byref(a))
    assert n >= 25 * 4 * 2 * 96 * 320 // 2
    for field, bad in (("poly_n", 6), ("flags", 1), ("flags", 512), ("winsize", 200), ("iterations", 0),
                       ("levels", 16), ("pyr_scale", 0.0), ("H", 1), ("poly_sigma", -1.0)):
        b = FsFlowArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.fs_optflow_workspace_bytes(C.byref(b)) == -1, field
        assert lib.fs_optflow_farneback(C.byref(b), None) == 1, field
    a.img0 = a.img1 = a.flow = a.workspace = 16
    a.workspace_bytes = n - 1
    assert lib.fs_optflow_farneback(C.byref(a), None) == 1        # workspace too small
    m = FsMotionMaskArgs()
    m.flow = m.P2 = m.pose = m.mask = 16
    m.B, m.H, m.W, m.mode = 1, 8, 8, 2
    assert lib.fs_motion_mask(C.byref(m), None) == 1
    assert lib.fs_augment_masks(16, None, None, None, 16, 1, 8, 8, 8, 8, None) == 1     # neither warp nor resize
    assert lib.fs_augment_masks(16, 16, 16, 16, 16, 1, 8, 8, 8, 8, None) == 1           # both
    assert lib.fs_augment_masks(16, 16, None, None, 16, 1, 8, 8, 8, 8, None) == 1       # warp without iplan


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_optflow_kernels_do_not_spill():
    """optflow.hip's eight kernels, and the masks kernel that carries their result through the input pipeline beside
    the four frames kernels of augment.hip"""
    from fsnet_amd.csrc import build as B
    for name, count in (("optflow.hip", 8), ("augment.hip", 5)):
        src = os.path.join(os.path.dirname(B.__file__), name)
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            flags = [f for f in B.FLAGS if f != "-fPIC"] + B.extra_flags(src)
            subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", out], check=True,
                           stderr=subprocess.DEVNULL)
            txt = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M)
        assert len(kernels) == count, name
        assert any("masks_kernel" in k for k in kernels) == (name == "augment.hip")
        assert max(int(x) for x in re.findall(r"^\s*\.vgpr_spill_count:\s*(\d+)", txt, re.M)) == 0, name
        assert max(int(x) for x in re.findall(r"^; ScratchSize: (\d+)", txt, re.M)) == 0, name
        assert not re.search(r"^\s*scratch_(load|store)", txt, re.M), name
