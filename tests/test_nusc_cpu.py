"""nuScenes evaluation on the host: the explicit-order mirror of fs_lidar_nusc_depth_u16 and generate_depth_map against
the reference's export of the seeded tree (tests/golden/nusc_eval.npz, tools/gen_golden.py::gen_nusc), the datasets key
for key, the JSON table reader, the host `_precompute`, and the shipped nuScenes configs building their validation
dataset and evaluator.  (`_single_loss` is fs_depth_eval_masked, a device kernel: its golden check is in test_nusc_gpu.py; its numpy restatement
is checked here.)"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from tests import helpers_nusc as HN

GOLD = os.path.join(os.path.dirname(__file__), "golden", "nusc_eval.npz")
PRE = "fsnet_amd."
REF = "/root/reference"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return HN.make_tree(str(tmp_path_factory.mktemp("nusc")))


@pytest.fixture(scope="module")
def nusc(tree):
    from fsnet_amd.vision_base.data.datasets.nuscenes_utils import NuScenesTables
    return NuScenesTables(version=HN.VERSION, dataroot=tree["dataroot"], verbose=False)     # the reader, devkit or not


def _camera(nusc, rec, cam):
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    samp = nusc.get('sample_data', rec['data'][cam])
    sens = nusc.get('calibrated_sensor', samp['calibrated_sensor_token'])
    return samp, E.camera_extrinsics(sens), np.array(sens['camera_intrinsic'])


def test_mirror_and_generate_depth_map_equal_the_reference_export(gold, nusc):
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    for j, i in enumerate(HN.EVAL):
        rec = nusc.get('sample', 'sample_%d' % i)
        lidar_data, lidar_mask = E.get_lidar(nusc, rec)
        assert lidar_data.shape == (81920, 5) and lidar_data.dtype == np.float32 and lidar_mask.dtype == np.float32
        lidar = lidar_data[lidar_mask == 1, :]
        assert 0 < len(lidar) < HN.NPTS + 40 + len(HN.special_points())        # remove_close dropped the near box
        for c, cam in enumerate(HN.CAMS):
            _, T, K = _camera(nusc, rec, cam)
            mine = E.nusc_depth_u16(lidar, E.projection_matrix(T, K)[:3], [HN.H, HN.W])
            assert mine.dtype == np.uint16 and mine.shape == (HN.H, HN.W)
            assert int((mine != gold["gt_png"][j, c]).sum()) == 0, (i, cam)
            f64 = E.generate_depth_map(lidar, T, K, im_shape=[HN.H, HN.W])
            assert f64.dtype == np.float64 and np.array_equal(f64, gold["gt_f64"][j, c]), (i, cam)
            assert np.array_equal((f64 * 256).astype(np.uint16), mine)


def test_mirror_special_cases():
    """the hand-placed points of CAM_FRONT land where their comments say"""
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    t, q, K = HN.cameras()['CAM_FRONT']
    M = E.projection_matrix(E.camera_extrinsics(dict(rotation=q, translation=t)), np.array(K))[:3]
    assert np.array_equal(M, [[20, -32, 0, -30], [12, 0, -32, 30], [1, 0, 0, -1.5]])
    d = E.nusc_depth_u16(HN.special_points().astype(np.float32), M, [HN.H, HN.W])
    assert d[3, 5] == 8 * 256 and d[3, 4] == 0 and d[3, 6] == 0 and d[3, 7] == 4 * 256   # 5.5 -> 6, 6.5 -> 6, 8.5 -> 8 (- 1)
    assert d[7, 10] == 8 * 256 and d[6, 10] == 0 and d[8, 10] == 0                        # 7.5 -> 8, 8.5 -> 8
    assert d[9, 12] == 9 * 256 + 3 and d[9, 13] == 7 * 256 and d[9, 14] == 5 * 256
    assert d[14, HN.W - 1] == 6 * 256 and d[15, 0] == 6 * 256                 # first pixel of the pair takes the minimum
    assert d[17, 0] == 4 * 256 and d[16, HN.W - 1] == 25 * 256                # ... the second keeps its last writer
    assert d[HN.H - 1, HN.W - 1] == 13 * 256 and d[0, 0] == 14 * 256 and d[20, 20] == 100 * 256 + 1
    assert int((d != 0).sum()) == 13
    # behind the camera, NaN, and the saturation beyond 256 m
    pts = np.array([[-5, 0, 1.5, 0], [np.nan, 0, 1.5, 0], [301.5, 0, 1.5, 0], [1.5 + 1 / 512, 0, 1.5, 0]], np.float32)
    d = E.nusc_depth_u16(pts[:3], M, [HN.H, HN.W])
    assert d[11, 19] == 65535 and int((d != 0).sum()) == 1
    assert int((E.nusc_depth_u16(pts, M, [HN.H, HN.W]) != 0).sum()) == 0      # ... and the q = 0 point after it wins
    d = E.nusc_depth_u16(pts[[0, 1, 3]], M, [HN.H, HN.W])
    assert int((d != 0).sum()) == 0                                          # q = 0 hit: a point, yet no depth
    assert E.nusc_depth_u16(np.zeros((0, 4), np.float32), M, [3, 2]).shape == (3, 2)


def test_quaternion_and_transform_matrix():
    from scipy.spatial.transform import Rotation
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E
    rng = np.random.RandomState(0)
    for _ in range(5):
        q = rng.randn(4)
        R = E.quaternion_rotation_matrix(q * 3.0)                              # normalised first
        want = Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()
        assert np.allclose(R, want, atol=1e-14)
        t = rng.randn(3)
        assert np.allclose(E.transform_matrix(t, q, inverse=True) @ E.transform_matrix(t, q), np.eye(4), atol=1e-14)
    assert np.array_equal(E.quaternion_rotation_matrix([0.5, -0.5, 0.5, -0.5]), [[0, 0, 1], [-1, 0, 0], [0, -1, 0]])
    x = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(E.pad_or_trim_to_np(x, [3, 2]), [[0, 1], [3, 4], [0, 0]])


def test_table_reader_resolves_what_the_golden_run_resolved(gold, tree, nusc):
    from fsnet_amd.vision_base.data.datasets import nuscenes_utils as NU
    one = NU.NuScenes(version=HN.VERSION, dataroot=tree["dataroot"], verbose=False)
    assert NU.NuScenes(tree["dataroot"], HN.VERSION) is one                              # the singleton
    assert one.get('sample', 'sample_1')['data'] == nusc.get('sample', 'sample_1')['data']
    assert len(gold["resolved_tokens"]) > 30
    for table, token in zip(gold["resolved_tables"], gold["resolved_tokens"]):
        assert nusc.get(str(table), str(token))['token'] == str(token)
    with pytest.raises(KeyError):
        nusc.get('sample', 'no_such_token')
    assert len(nusc.scene) == 1 and len(nusc.sample) == HN.NS and nusc.dataroot == tree["dataroot"]
    for i, rec in enumerate(nusc.sample):
        assert rec['data'] == {c: 'sd_%s_%d' % (c, i) for c in HN.CAMS + ['LIDAR_TOP']}
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import get_samples
    assert [s['token'] for s in get_samples(nusc)] == ['sample_%d' % i for i in range(HN.NS)]


def _check_sample(sample, gold, prefix, keys, digest=False):
    assert [HN.key_name(k) for k in sample] == [str(k) for k in keys]
    for key, val in sample.items():
        want = gold[prefix + HN.key_name(key)]
        got = np.asarray(val)
        if digest and got.dtype == np.uint8 and got.ndim == 3:
            got = np.array(list(got.shape) + [zlib.crc32(np.ascontiguousarray(got).tobytes())], np.int64)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (prefix, key)


def test_json_dataset_equals_the_reference_samples(gold, tree):
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    ds = NusceneJsonDataset(json_path=tree["json_train"], augmentation=HN.raw_augmentation(PRE))
    assert len(ds) == int(gold["json_n"]) == 12
    for i in range(len(ds)):
        s = ds[i]
        _check_sample(s, gold, "json%d_" % i, gold["json_keys"])
        assert s[('filename', 0)].startswith('samples/' + s['camera_type'] + '/') and s['patched_mask'].dtype == np.float64
        assert s['camera_type'] == HN.CAMS[s['camera_type_index']]
    val = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                             augmentation=HN.raw_augmentation(PRE))
    _check_sample(val[3], gold, "jsonval3_", gold["jsonval_keys"])
    tall = NusceneJsonDataset(json_path=tree["json_tall"], image_keys=['frame0'], frame_ids=[0],
                              augmentation=HN.raw_augmentation(PRE))
    for i in range(2):                       # CAM_BACK: rows 700 and below zeroed; the same frame as CAM_FRONT: ones
        pm = tall[i]['patched_mask']
        assert pm.dtype == np.float64 and pm.shape == (HN.TALL_H, HN.TALL_W)
        assert np.array_equal(pm.min(1), gold["tall%d_mask_rows" % i]) and np.array_equal(pm.max(1), pm.min(1))
    assert tall[0]['patched_mask'][700:].max() == 0 and tall[0]['patched_mask'][:700].min() == 1


def test_json_dataset_reads_vo_depth(tree, tmp_path):
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    plain = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                               augmentation=HN.raw_augmentation(PRE))
    vo_dir = str(tmp_path / "vo")
    name = plain[0][('filename', 0)].replace('samples', vo_dir).replace('.jpg', '.png')
    os.makedirs(os.path.dirname(name))
    vo = np.random.RandomState(0).randint(0, 65536, size=(8, 16)).astype(np.uint16)
    write_png16(name, vo)
    ds = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0], vo_path=vo_dir,
                            augmentation=HN.raw_augmentation(PRE))
    want = vo / 65535.0 * 120
    want[(want < 3) | (want > 80)] = 120
    assert np.array_equal(ds[0][('vo_depth', 0)], want) and ('vo_depth', 0) not in ds[1]
    keys = list(ds[0])
    assert keys.index(('vo_depth', 0)) == keys.index('camera_type') + 1


@pytest.mark.parametrize("tag", ["mono", "sweep"])
@pytest.mark.parametrize("filt", [False, True])
def test_table_datasets_equal_the_reference_samples(gold, tree, tag, filt):
    """is_filter_static with a threshold between the tree's displacements: some samples are redrawn, with the
    reference's np.random.randint call"""
    from fsnet_amd.monodepth.data.datasets import nuscene_dataset as D
    cls = dict(mono=D.NusceneDepthMonoDataset, sweep=D.NusceneSweepDepthMonoDataset)[tag]
    ds = cls(split_file=tree["split"], nuscenes_version=HN.VERSION, nuscenes_dir=tree["dataroot"],
             is_filter_static=filt, filter_threshold=1.1005 if filt else 0.03, augmentation=HN.raw_augmentation(PRE))
    k = "%s%d" % (tag, int(filt))
    assert len(ds) == int(gold[k + "_n"]) == 12
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    for i in range(len(ds)):
        _check_sample(ds[i], gold, "%s_%d_" % (k, i), gold[k + "_keys"], digest=True)
    assert filt == (not np.array_equal(np.random.get_state()[1], state))       # the filter drew, and only the filter


def test_samples_pass_both_collate_functions(tree):
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN, DeviceAugment
    from fsnet_amd.vision_base.data.datasets.dataset_utils import collate_fn
    raw = NusceneJsonDataset(json_path=tree["json_train"], augmentation=HN.raw_augmentation(PRE))
    b = collate_fn([raw[0], raw[3], raw[7]])
    assert b['camera_type'] == ['CAM_FRONT', 'CAM_BACK', 'CAM_FRONT_RIGHT'] and b['camera_type_index'] == [0, 3, 1]
    assert b[('filename', 0)] == [raw[i][('filename', 0)] for i in (0, 3, 7)]
    assert b[('image', 1)].shape == (3, HN.H, HN.W, 3) and b['patched_mask'].dtype == torch.float64
    val = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                             augmentation=HN.val_augmentation(PRE, 64, 128))
    batch = DeviceAugment([0]).collate([val[1], val[9]])
    assert batch['camera_type'] == ['CAM_FRONT_RIGHT', 'CAM_BACK'] and batch[PLAN]["kind"] == "resize"
    assert batch[('filename', 0)] == [val[1][('filename', 0)], val[9][('filename', 0)]]
    assert batch[('image_resize', 'original_shape')].tolist() == [[HN.H, HN.W]] * 2


def test_host_precompute_writes_the_reference_layout(gold, tree, tmp_path):
    from fsnet_amd.monodepth.data.datasets.utils import read_png16
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import NuscenesEvaluator
    gt_dir = str(tmp_path / "samples_depth_gt")
    ev = NuscenesEvaluator(tree["dataroot"], tree["split"], gt_dir, nuscenes_version=HN.VERSION, export_on_device=False,
                           group_size=1)
    assert ev.token_list == ['sample_%d' % i for i in HN.EVAL] and sorted(os.listdir(gt_dir)) == sorted(HN.CAMS)
    for j, i in enumerate(HN.EVAL):
        for c, cam in enumerate(HN.CAMS):
            name = 'n015__%s__%d.png' % (cam, 1532402927000000 + 500000 * i)
            assert ev._gt_path('samples/%s/%s' % (cam, name.replace('.png', '.jpg'))) == os.path.join(gt_dir, cam, name)
            got = read_png16(os.path.join(gt_dir, cam, name))
            assert got.dtype == np.uint16 and np.array_equal(got, gold["gt_png"][j, c]), (i, cam)
    # an existing folder is not exported again; is_force_recompute exports
    os.remove(os.path.join(gt_dir, 'CAM_BACK', name.replace(cam, 'CAM_BACK')))
    NuscenesEvaluator(tree["dataroot"], tree["split"], gt_dir, nuscenes_version=HN.VERSION, export_on_device=False)
    assert len(os.listdir(os.path.join(gt_dir, 'CAM_BACK'))) == 1
    NuscenesEvaluator(tree["dataroot"], tree["split"], gt_dir, nuscenes_version=HN.VERSION, export_on_device=False,
                      is_force_recompute=True)
    assert len(os.listdir(os.path.join(gt_dir, 'CAM_BACK'))) == 2
    text = ev.log(None, 'CAM_BACK', np.arange(7.0), np.arange(7.0) + 1, epoch_num=3, is_print=False)
    head = "  " + "".join("%8s | " % m for m in ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    assert text == ("Epoch 3 for channel CAM_BACK\n" + head + "\n"
                    "&   0.000  &   1.000  &   2.000  &   3.000  &   4.000  &   5.000  &   6.000  \\\\\n"
                    "Epoch 3 for channel CAM_BACK | Abs Error without Scaled\n" + head + "\n"
                    "&   1.000  &   2.000  &   3.000  &   4.000  &   5.000  &   6.000  &   7.000  \\\\")


def test_workspace_refusals_without_a_gpu():
    from fsnet_amd.hip import lib
    ws = lib.fs_lidar_nusc_depth_workspace_bytes
    assert ws(1, 6, 900, 1600) == 6 * 900 * 1600 * 16 and ws(2, 1, 1, 2) == 64
    for G, C, H, W in ((0, 1, 1, 2), (1, 0, 1, 2), (1, 1, 0, 2), (1, 1, 1, 1), (-1, 6, 4, 4), (10923, 6, 1, 2),
                       (65535, 2, 1, 2), (1, 1, 32768, 65536), (4, 6, 9000, 10000)):
        assert ws(G, C, H, W) == -1, (G, C, H, W)
    assert ws(65535, 1, 1, 2) > 0 and ws(10922, 6, 1, 2) > 0 and ws(1, 1, 32768, 65535) > 0
    assert lib.fs_lidar_nusc_depth_u16(None, None, 0, None, 1, 1, 1, 2, None, None, 0, None) == 1


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("name", ["nusc_wpose_example", "distill_nusc_example"])
def test_shipped_nusc_configs_build_dataset_hook_and_evaluator(tmp_path, tree, name):
    """the two shipped nuScenes configs with their `name=` prefixes repointed: the validation dataset and the
    evaluation hook with its NuscenesEvaluator build from the config's own entries (only the paths point at the tmp
    tree, whose gt_saved_dir exists), and a validation sample flows through the config's chain"""
    from tests.test_reference_configs_cpu import _load_cfg
    from fsnet_amd.monodepth.data.datasets.nuscene_dataset import NusceneJsonDataset
    from fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval import NuscenesEvaluator
    from fsnet_amd.monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks import FastNuscEvaluationHook
    from fsnet_amd.vision_base.data.augmentations.augmentations import PLAN
    from fsnet_amd.vision_base.utils.builder import build
    cfg = _load_cfg(tmp_path, name)
    assert cfg.val_dataset.name == "fsnet_amd.monodepth.data.datasets.nuscene_dataset.NusceneJsonDataset"
    cfg.val_dataset.json_path = tree["json_val"]
    ds = build(**cfg.val_dataset)
    assert isinstance(ds, NusceneJsonDataset) and len(ds) == 12
    s = ds[4]
    assert s['camera_type'] == 'CAM_BACK_LEFT' and s[PLAN]["resize"] is not None
    assert tuple(s[('image_resize', 'effective_size')]) == tuple(cfg.data.rgb_shape[:2])
    hook_cfg = cfg.trainer.evaluate_hook
    assert hook_cfg.name.endswith("base_evaluation_hooks.FastNuscEvaluationHook")
    ev_cfg = hook_cfg.dataset_eval_cfg
    assert ev_cfg.name == "fsnet_amd.monodepth.evaluation.nuscenes_unsupervised_eval.NuscenesEvaluator"
    gt_dir = str(tmp_path / "samples_depth_gt")
    os.makedirs(gt_dir)
    ev_cfg.data_path, ev_cfg.split_file, ev_cfg.gt_saved_dir = tree["dataroot"], tree["split"], gt_dir
    hook = build(**hook_cfg)
    assert isinstance(hook, FastNuscEvaluationHook) and isinstance(hook.dataset_eval_func, NuscenesEvaluator)
    assert hook.dataset_eval_func.channels == HN.CAMS and hook.dataset_eval_func.token_list == ['sample_1', 'sample_2']
    assert os.listdir(gt_dir) == [] and hook.save_depth_dir is None and getattr(hook, 'batch_size', 16) == 16
    for sec in ("train_dataset",):
        assert "NusceneJsonDataset" in str(cfg[sec])
    assert "fsnet_amd" in sys.modules


def test_host_restatement_of_single_loss_equals_the_reference(gold):
    """the numpy oracle of the GPU tests (tests/helpers_nusc.single_loss: the nuScenes crop, rows from 0.03594771 H)
    against the reference's `_single_loss`; the evaluator's own `_single_loss` is a device kernel (test_nusc_gpu.py)"""
    for k in range(len(gold["loss"])):
        gt = (gold["gt_png"][k // 6, k % 6] / 256.0).astype(np.float32)
        r = HN.single_loss(gold["loss_pred"][k].copy(), gt.copy())
        got = np.concatenate([[r["ratio"]], r["error"], r["abs_error"]]).astype(np.float64)
        assert np.array_equal(got, gold["loss"][k]), k
    with pytest.raises(ValueError):
        HN.single_loss(np.ones((13, 21), np.float32), np.zeros((HN.H, HN.W), np.float32))
