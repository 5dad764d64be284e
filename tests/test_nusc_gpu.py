"""nuScenes evaluation on the device: fs_lidar_nusc_depth_u16 against its explicit-order host mirror, bit for bit, at the
smallest shapes that can go wrong and at full size; its determinism under regrouping and graph replay; its refusals;
the device `_precompute` against the host path and the reference's PNGs (tests/golden/nusc_eval.npz); `_single_loss`
against the reference's numbers; FastNuscEvaluationHook with a fixed-weight model against the reference's hook, its
saved folder rescored by NuscenesEvaluator.__call__, and the post-optimising hook against the same steps by hand."""
import os

import numpy as np
import pytest
import torch

from tests import helpers_kitti360 as HK
from tests import helpers_nusc as HN

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "nusc_eval.npz")
PRE = "fsnet_amd."
HOOKS = PRE + "monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks."
VAL_HOOK = PRE + "vision_base.pipeline_hooks.train_val_hooks.base_validation_hooks.BaseValidationHook"
EVALUATOR = PRE + "monodepth.evaluation.nuscenes_unsupervised_eval.NuscenesEvaluator"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HN.make_tree(str(tmp_path_factory.mktemp("nusc")))


def _mirror(scans, M, H, W):
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import nusc_depth_u16
    return np.stack([np.stack([nusc_depth_u16(s, M[g, c], [H, W]) for c in range(M.shape[1])])
                     for g, s in enumerate(scans)])


def _device(scans, M, H, W, dev):
    from fsnet_amd.hip import ops
    out = ops.lidar_nusc_depth_u16(scans, M, H, W, dev)
    assert out.dtype == torch.uint16 and tuple(out.shape) == (len(scans), M.shape[1], H, W)
    return out.cpu().numpy()


def _tiny_matrices(rng, G, C, H, W):
    """camera 0 of every sample is exact (identity rotation, dyadic intrinsics: ties stay ties); the others are
    slightly rotated and shifted"""
    M = np.zeros((G, C, 3, 4))
    for g in range(G):
        for c in range(C):
            K = np.array([[4.0, 0, (W + 1) / 2.0, 0], [0, 4.0, (H + 1) / 2.0, 0], [0, 0, 1.0, 0]])
            if c:
                a = 0.05 * rng.randn(3)
                R = np.eye(4)
                R[:3, :3] += np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                R[:3, 3] = 0.1 * rng.randn(3)
                K = (K * (1 + 0.03 * rng.randn())) @ R
            M[g, c] = K
    return M


def _tiny_scan(rng, H, W, n):
    """camera-frame points (x right, y down, z forward) aimed at the pixels of the exact camera and one ring around
    them, at depths on multiples of 1/256: exact .5 ties in u and v, groups of 2 to 5 on one pixel, row ends paired
    with the next row's start, z <= 0, z = NaN, z below 1/256 (q = 0 hits)"""
    u = rng.randint(0, 2 * (W + 2) + 1, n) / 2.0            # 0, 0.5, ... W + 2: every half pixel, in and out of range
    v = rng.randint(0, 2 * (H + 2) + 1, n) / 2.0
    z = rng.randint(1, 40 * 256, n) / 256.0
    kind = rng.randint(0, 12, n)
    z[kind == 0] = rng.randint(1, 4, (kind == 0).sum()) / 1024.0              # q = 0
    z[kind == 1] = -z[kind == 1]
    z[kind == 2] = 0.0
    x = (u - (W + 1) / 2.0) * z / 4.0
    y = (v - (H + 1) / 2.0) * z / 4.0
    pts = np.stack([x, y, z, rng.rand(n)], 1).astype(np.float32)
    pts[kind == 3, 2] = np.nan
    return pts


@pytest.mark.parametrize("G,C", [(1, 1), (1, 2), (1, 6), (3, 1), (3, 2), (3, 6)])
def test_kernel_equals_the_mirror_at_the_smallest_shapes(dev, G, C):
    seen = dict(ties=0, q0=0, pairs=0, groups=set(), behind=0, nan=0)
    for W in (2, 3):
        for H in range(1, 6):
            rng = np.random.RandomState(1000 * G + 100 * C + 10 * W + H)
            M = _tiny_matrices(rng, G, C, H, W)
            scans = [_tiny_scan(rng, H, W, 12 * H * W + 5) for _ in range(G)]
            if G > 1:
                scans[1] = np.zeros((0, 4), np.float32)                       # one sample without a point
            want, got = _mirror(scans, M, H, W), _device(scans, M, H, W, dev)
            assert np.array_equal(got, want), (G, C, H, W, np.argwhere(got != want)[:5])
            # what this fixture holds, through the exact camera of sample 0
            s = scans[0].astype(np.float64)
            z = s[:, 2]
            seen["behind"] += int((z <= 0).sum())
            seen["nan"] += int(np.isnan(z).sum())
            ok = z > 0
            uu, vv = (4 * s[ok, 0] + (W + 1) / 2.0 * z[ok]) / z[ok], (4 * s[ok, 1] + (H + 1) / 2.0 * z[ok]) / z[ok]
            col, row = np.rint(uu) - 1, np.rint(vv) - 1
            inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
            seen["ties"] += int((inside & ((uu % 1 == 0.5) | (vv % 1 == 0.5))).sum())
            seen["q0"] += int((inside & (z[ok] * 256 < 1)).sum())
            hits = np.bincount((row[inside] * W + col[inside]).astype(int), minlength=H * W).reshape(H, W)
            seen["groups"] |= set(hits.reshape(-1).tolist())
            seen["pairs"] += int(((hits[:-1, W - 1] > 0) & (hits[1:, 0] > 0)).sum())
    assert seen["ties"] > 50 and seen["q0"] > 5 and seen["pairs"] > 5 and seen["behind"] > 50 and seen["nan"] > 20
    assert {2, 3, 4, 5} <= seen["groups"]


def _full_size_case(G=1, n=35000, seed=3):
    """the tree's six cameras at 900 x 1600 (intrinsics x 40, CAM_FRONT still exact) and a ring of points with
    extra returns along some rays, so that thousands of pixels hold more than one"""
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    H, W = 900, 1600
    cams = HN.cameras()
    M = np.zeros((G, len(HN.CAMS), 3, 4))
    for c, cam in enumerate(HN.CAMS):
        t, q, K = cams[cam]
        K = np.array(K) * np.array([[40.0], [37.5], [1.0]])
        M[:, c] = E.projection_matrix(E.camera_extrinsics(dict(rotation=q, translation=t)), K)[:3]
    rng = np.random.RandomState(seed)
    scans = []
    for g in range(G):
        ang = rng.uniform(0, 2 * np.pi, n)
        dist = np.exp(rng.uniform(np.log(2.5), np.log(200.0), n))
        ego = np.stack([dist * np.cos(ang), dist * np.sin(ang), rng.uniform(-1.0, 4.0, n) + 0.02 * dist], 1)
        k = n // 5
        ego[-k:] = ego[:k] * rng.uniform(1.0, 1.002, (k, 1))                  # a second return close to the first
        scans.append(np.concatenate([ego, rng.rand(n, 1)], 1).astype(np.float32))
    return scans, M, H, W


def test_kernel_equals_the_mirror_at_full_size(dev):
    scans, M, H, W = _full_size_case()
    want, got = _mirror(scans, M, H, W), _device(scans, M, H, W, dev)
    hit = int((want != 0).sum())
    assert hit > 20000 and want.max() < 255 * 256
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_regrouping_and_replay_give_the_same_bits(dev, tree):
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    from fsnet_amd.vision_base.data.datasets.nuscenes_utils import NuScenes
    nusc = NuScenes(version=HN.VERSION, dataroot=tree["dataroot"], verbose=False)
    ev = object.__new__(E.NuscenesEvaluator)
    scans, Ms = [], []
    for i in range(HN.NS):
        rec = nusc.get('sample', 'sample_%d' % i)
        data, mask = E.get_lidar(nusc, rec)
        scans.append(np.ascontiguousarray(data[mask == 1, :4]))
        Ms.append(np.stack([j[2] for j in ev._export_jobs(nusc, rec, "gt")]) * (1.0 + 0.01 * i))
    scans[2] = scans[2][:0]                                                   # an empty sample inside the group
    Ms = np.stack(Ms)
    H, W, G = HN.H, HN.W, len(scans)
    a = _device(scans, Ms, H, W, dev)
    assert np.array_equal(a, _mirror(scans, Ms, H, W)) and (a != 0).sum() > 2000 and (a[2] == 0).all()
    assert np.array_equal(_device(scans, Ms, H, W, dev), a)
    singles = np.concatenate([_device(scans[g:g + 1], Ms[g:g + 1], H, W, dev) for g in range(G)])
    threes = np.concatenate([_device(scans[g:g + 3], Ms[g:g + 3], H, W, dev) for g in range(0, G, 3)])
    assert np.array_equal(singles, a) and np.array_equal(threes, a)
    op = ops.LidarNuscDepth(G, len(HN.CAMS), H, W, dev)
    op.stage(scans, Ms)
    HK.run_captured(op, dict(depth=-1))
    assert np.array_equal(op.depth.view(torch.uint16).cpu().numpy(), a)


def test_refusals(dev):
    from fsnet_amd.hip import lib, ops
    ws_fn = lib.fs_lidar_nusc_depth_workspace_bytes
    pts = torch.zeros(4, 4, device=dev)
    offs = torch.tensor([0, 4], dtype=torch.int64, device=dev)
    M = torch.zeros(12, dtype=torch.float64, device=dev)
    out = torch.zeros(64, dtype=torch.int16, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)

    def call(G=1, C=1, H=2, W=2, points=pts, offsets=offs, n=4, m=M, depth=out, work=ws, nbytes=4096):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.fs_lidar_nusc_depth_u16(p(points), p(offsets), n, p(m), G, C, H, W, p(depth), p(work), nbytes, None)
    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(G=0), dict(C=0), dict(H=0), dict(W=1), dict(G=10923, C=6, H=1, W=2), dict(G=65535, C=2, H=1),
                dict(H=32768, W=65536), dict(G=-1), dict(C=-3)):
        shape = dict(dict(G=1, C=1, H=2, W=2), **bad)
        assert ws_fn(shape["G"], shape["C"], shape["H"], shape["W"]) == -1, bad
        assert call(**bad) == 1, bad
    assert ws_fn(1, 1, 2, 2) == 64
    for bad in (dict(offsets=None), dict(m=None), dict(depth=None), dict(work=None), dict(n=-1), dict(points=None),
                dict(nbytes=63), dict(work=ws[1:]), dict(points=pts.view(-1)[1:]), dict(depth=out.view(torch.uint8)[1:])):
        assert call(**bad) == 1, list(bad)
    assert call(points=None, n=0) == 0                                        # an empty cloud needs no points
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.LidarNuscDepth(1, 6, 900, 1, dev)


def test_device_precompute_equals_the_host_path_and_the_golden(dev, gold, tree, tmp_path):
    from fsnet_amd.monodepth.data.datasets.utils import read_png16
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import NuscenesEvaluator
    dirs = dict(device=str(tmp_path / "gt_device"), host=str(tmp_path / "gt_host"))
    ev = NuscenesEvaluator(tree["dataroot"], tree["split"], dirs["device"], nuscenes_version=HN.VERSION, device=dev,
                           group_size=2)
    assert ev.export_on_device and ev._op.G == 2                              # the default where there is a GPU
    NuscenesEvaluator(tree["dataroot"], tree["split"], dirs["host"], nuscenes_version=HN.VERSION,
                      export_on_device=False)
    for j, i in enumerate(HN.EVAL):
        for c, cam in enumerate(HN.CAMS):
            name = 'n015__%s__%d.png' % (cam, 1532402927000000 + 500000 * i)
            a, b = (read_png16(os.path.join(dirs[k], cam, name)) for k in ("device", "host"))
            assert a.dtype == np.uint16 and np.array_equal(a, b) and np.array_equal(a, gold["gt_png"][j, c]), (i, cam)


def test_single_loss_equals_the_reference(dev, gold, tree, tmp_path):
    """the tolerances of tests/test_eval_gpu.py::test_depth_eval_matches_oracle, for the same kernel; the numpy
    restatement of tests/helpers_nusc.py, the oracle of the folder test below, equals the reference's numbers too"""
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import NuscenesEvaluator
    gt_dir = str(tmp_path / "gt")
    os.makedirs(os.path.join(gt_dir, 'CAM_FRONT'))
    ev = NuscenesEvaluator(tree["dataroot"], tree["split"], gt_dir, nuscenes_version=HN.VERSION, device=dev)
    k = 0
    for j in range(len(HN.EVAL)):
        for c in range(len(HN.CAMS)):
            gt = (gold["gt_png"][j, c] / 256.0).astype(np.float32)
            got = ev._single_loss(torch.from_numpy(gold["loss_pred"][k]).to(dev), gt)
            want = gold["loss"][k]
            mine = HN.single_loss(gold["loss_pred"][k].copy(), gt.copy())
            assert np.array_equal(np.concatenate([[mine["ratio"]], mine["error"], mine["abs_error"]]).astype(np.float64),
                                  want), k
            assert abs(float(got["ratio"]) - want[0]) <= 1e-5 * want[0]
            for a, b in ((got["error"], want[1:8]), (got["abs_error"], want[8:15])):
                a = np.array(a, np.float64)
                assert np.abs(a[:4] - b[:4]).max() <= 2e-5 * max(1.0, np.abs(b[:4]).max()), (k, a, b)
                assert np.abs(a[4:] - b[4:]).max() <= 3.0 / max(1, (gt > 1e-3).sum() // 4), (k, a, b)
            k += 1
    with pytest.raises(ValueError):                                           # an empty valid set
        ev._single_loss(torch.ones(13, 21, device=dev), np.zeros((HN.H, HN.W), np.float32))
    write_png16(os.path.join(gt_dir, 'CAM_FRONT', 'empty.png'), np.zeros((HN.H, HN.W), np.uint16))
    with pytest.raises(ValueError):
        ev.single_call(torch.ones(13, 21, device=dev), 'samples/CAM_FRONT/empty.jpg')
    assert float(ev.device_errors(torch.ones(13, 21, device=dev), 'samples/CAM_FRONT/empty.jpg')[15]) == 0


def _model(dev, h, w):
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import fsnet_oracle as O
    m = build(**meta_arch_cfg(h, w, with_pose=False))
    m.load_state_dict(O.init_state(seed=2, with_pose=False), strict=True)
    return m.to(dev)


def _hook(name, tree, gt_dir, dev, **kw):
    from fsnet_amd.vision_base.utils.builder import build
    return build(name=HOOKS + name, test_run_hook_cfg=dict(name=VAL_HOOK),
                 dataset_eval_cfg=dict(name=EVALUATOR, data_path=tree["dataroot"], split_file=tree["split"],
                                       gt_saved_dir=gt_dir, nuscenes_version=HN.VERSION, device=dev),
                 num_workers=0, **kw)


def _close(got, want):
    """tests/test_kitti_eigen_eval_gpu.py's bound on the hook's means against the host pipeline: the same op chain"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.abs(got[:4] - want[:4]).max() <= 1e-4 * max(1.0, np.abs(want[:4]).max())
            and np.abs(got[4:] - want[4:]).max() <= 2e-3)


def test_hook_equals_the_reference_and_its_saved_folder_rescores(dev, gold, tree, tmp_path):
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    from fsnet_amd.monodepth.data.datasets.utils import read_png16
    from fsnet_amd.vision_base.data.augmentations.augmentations import DeviceAugment
    from oracle import eval_oracle as EO
    h, w = (int(v) for v in gold["hook_hw"])
    ds = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                            augmentation=HN.val_augmentation(PRE, h, w))
    gt_dir, save = str(tmp_path / "samples_depth_gt"), str(tmp_path / "result")
    RT.set_compute_dtype(torch.float32)
    try:
        m = _model(dev, h, w)
        plain = _hook("FastNuscEvaluationHook", tree, gt_dir, dev, batch_size=5)
        assert sorted(os.listdir(gt_dir)) == sorted(HN.CAMS)                  # the evaluator exported on construction
        res = plain(m, ds)
        assert not os.path.exists(save) and m.training
        saving = _hook("FastNuscEvaluationHook", tree, gt_dir, dev, save_depth_dir=save)
        assert getattr(saving, 'batch_size', 16) == 16
        res_saving = saving(m, ds)
        # the same network outputs through the host pipeline, one sample at a time: what each saved file must hold
        m.eval()
        host_maps = {}
        with torch.no_grad():
            for i in range(len(ds)):
                sample = ds[i]
                batch = DeviceAugment([0])([sample], dev)
                depth = m(batch, dict(is_training=False))["depth"][0, 0, :h, :w].float().cpu().numpy()
                host_maps[(sample['camera_type'], os.path.basename(sample[('filename', 0)])[:-4] + '.png')] = \
                    EO.cv2_resize_linear(depth, HN.W, HN.H)                    # the depth itself, not its inverse
        m.train()
    finally:
        RT.set_compute_dtype(torch.bfloat16)
    assert len(host_maps) == len(ds) == 12
    assert list(res["per_camera"]) == HN.CAMS                                 # first-seen order
    for key, gkey in (("mean_errors", "hook_errors"), ("mean_abs_errors", "hook_abs_errors")):
        for c, cam in enumerate(HN.CAMS):
            print(key, cam, res["per_camera"][cam][key], "reference", gold[gkey][c])
        print(key, "all mean", res[key], "reference", gold[gkey][-1])
    for key, gkey in (("mean_errors", "hook_errors"), ("mean_abs_errors", "hook_abs_errors")):
        for c, cam in enumerate(HN.CAMS):
            assert _close(res["per_camera"][cam][key], gold[gkey][c]), (key, cam)
            assert np.allclose(res_saving["per_camera"][cam][key], res["per_camera"][cam][key], rtol=1e-12, atol=0)
        assert _close(res[key], gold[gkey][-1]), key
        assert np.allclose(res[key], np.mean([res["per_camera"][cam][key] for cam in HN.CAMS], 0), rtol=1e-12, atol=0)
    # the saved folder: predict_depth/<CAM>/<name>.png beside the ground truth's names; NuscenesEvaluator.__call__
    # over it gives the host metric recomputed on the saved, 1/256 m quantised maps — the bound of the KITTI
    # save-and-rescore test (tests/test_kitti_eigen_eval_gpu.py)
    for cam in HN.CAMS:
        assert sorted(os.listdir(os.path.join(save, 'predict_depth', cam))) == sorted(os.listdir(os.path.join(gt_dir, cam)))
    folder = saving.dataset_eval_func(save)
    host_all, host_all_abs = [], []
    for cam in HN.CAMS:
        host, live = [], []
        for name in os.listdir(os.path.join(save, 'predict_depth', cam)):
            q = read_png16(os.path.join(save, 'predict_depth', cam, name))
            assert q.dtype == np.uint16 and q.shape == (HN.H, HN.W)
            # the file under this camera and name is uint16(depth * 256) of THIS sample's full-resolution prediction:
            # the bound of tests/test_kitti_eigen_eval_gpu.py (the device resize differs from the host's in the last
            # bits, which moves a truncation by one step on a few pixels)
            off = q.astype(np.float64) - np.trunc(host_maps[(cam, name)].astype(np.float64) * 256)
            assert np.abs(off).max() <= 1 and (off != 0).mean() < 0.05, (cam, name, np.abs(off).max())
            live.append(HN.single_loss(host_maps[(cam, name)].copy(),
                                       (read_png16(os.path.join(gt_dir, cam, name)) / 256.0).astype(np.float32)))
        # ... and the hook's means are the host metric of those same predictions
        for key, hkey in (("mean_errors", "error"), ("mean_abs_errors", "abs_error")):
            assert _close(res_saving["per_camera"][cam][key], np.array([r[hkey] for r in live], np.float64).mean(0)), (cam, key)
        for name in os.listdir(os.path.join(save, 'predict_depth', cam)):
            q = read_png16(os.path.join(save, 'predict_depth', cam, name))
            gt = (read_png16(os.path.join(gt_dir, cam, name)) / 256.0).astype(np.float32)
            host.append(HN.single_loss((q / 256.0).astype(np.float32), gt))
        host_err = np.array([r["error"] for r in host], np.float64).mean(0)
        host_abs = np.array([r["abs_error"] for r in host], np.float64).mean(0)
        host_all.append(host_err)
        host_all_abs.append(host_abs)
        got = folder["per_camera"][cam]
        rel = np.abs(got["mean_errors"] - host_err) / np.abs(host_err)
        rel_abs = np.abs(got["mean_abs_errors"] - host_abs) / np.maximum(np.abs(host_abs), 1e-12)
        print("folder", cam, got["mean_errors"], "host on the saved maps", host_err, "relative", rel, rel_abs)
        assert rel.max() <= 1e-5 and rel_abs[host_abs > 0].max() <= 1e-5, cam
        assert np.allclose(got["ratios"], [float(r["ratio"]) for r in host], rtol=1e-6, atol=0)
    for key, want in (("mean_errors", host_all), ("mean_abs_errors", host_all_abs)):
        want = np.mean(want, 0)
        assert (np.abs(folder[key] - want) / np.maximum(np.abs(want), 1e-12))[want > 0].max() <= 1e-5
    # a prediction whose ground truth has no usable point is skipped with the reference's warning
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    victim = sorted(os.listdir(os.path.join(gt_dir, 'CAM_BACK')))[0]
    write_png16(os.path.join(gt_dir, 'CAM_BACK', victim), np.zeros((HN.H, HN.W), np.uint16))
    fresh = _hook("FastNuscEvaluationHook", tree, gt_dir, dev).dataset_eval_func
    with pytest.warns(UserWarning, match="no usable points"):
        again = fresh(save)
    assert len(again["per_camera"]['CAM_BACK']["ratios"]) == 1 and len(again["per_camera"]['CAM_FRONT']["ratios"]) == 2


def test_postopt_hook_equals_the_same_steps_by_hand(dev, tree, tmp_path):
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    from fsnet_amd.monodepth.networks.utils import postopt_utils as PU
    from fsnet_amd.monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks import (
        PostOptFastNuscEvaluationHook, _collate, _materialize)
    h, w = 64, 128
    vo_dir, gt_dir = str(tmp_path / "vo"), str(tmp_path / "samples_depth_gt")
    plain_ds = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                                  augmentation=HN.val_augmentation(PRE, h, w))
    rng = np.random.RandomState(7)
    for i in range(len(plain_ds)):                                            # sparse VO depth at the network's size
        vo = np.zeros((h, w), np.float64)
        mask = rng.rand(h, w) < 0.05
        vo[mask] = rng.uniform(4.0, 60.0, int(mask.sum()))
        name = plain_ds[i][('filename', 0)].replace('samples', vo_dir).replace('.jpg', '.png')
        os.makedirs(os.path.dirname(name), exist_ok=True)
        write_png16(name, np.round(vo / 120.0 * 65535).astype(np.uint16))
    ds = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0], vo_path=vo_dir,
                            augmentation=HN.val_augmentation(PRE, h, w))
    assert ds[0][('vo_depth', 0)].shape == (h, w)
    RT.set_compute_dtype(torch.float32)
    try:
        m = _model(dev, h, w)
        hook = _hook("PostOptFastNuscEvaluationHook", tree, gt_dir, dev, batch_size=6, post_opt_cfg=dict(iter_num=2))
        assert isinstance(hook, PostOptFastNuscEvaluationHook) and hook._post_opt_params()["iter_num"] == 2
        res = hook(m, ds)
        unrefined = _hook("FastNuscEvaluationHook", tree, gt_dir, dev, batch_size=6)(m, ds)
        m.eval()
        rows = {}
        with torch.no_grad():
            for start in (0, 6):
                batch = _materialize(_collate([ds[i] for i in range(start, start + 6)]))
                depth = hook.test_hook(batch, m)["depth"][:, 0, :h, :w].float().contiguous()
                refined = ops.post_optimize(batch[('image', 0)][:, :, :h, :w].float().contiguous(), depth,
                                            batch[('vo_depth', 0)].to(dev, torch.float32), rgb_mean=PU.IMAGENET_MEAN,
                                            rgb_std=PU.IMAGENET_STD, **hook._post_opt_params())
                for i in range(6):
                    depth_0 = ops.resize_linear(refined[i].contiguous(), HN.H, HN.W, invert=False)
                    row = hook.dataset_eval_func.device_errors(depth_0, batch[('filename', 0)][i]).cpu().numpy()
                    rows.setdefault(batch['camera_type'][i], []).append(row)
        m.train()
    finally:
        RT.set_compute_dtype(torch.bfloat16)
    for cam in HN.CAMS:
        want = np.array(rows[cam])[:, 1:8].mean(0)
        assert np.allclose(res["per_camera"][cam]["mean_errors"], want, rtol=1e-12, atol=0), cam
    assert not np.allclose(res["mean_errors"], unrefined["mean_errors"], rtol=1e-3, atol=0)   # the refinement acted
    assert np.isfinite(res["mean_errors"]).all() and np.isfinite(res["mean_abs_errors"]).all()
