"""Pins the oracle of the supervised-metrics GPU tests: the vectorised f64 numpy restatement of compute_errors
(tests/helpers_supervised_eval.py) equals the REAL reference function's nine numbers
(tests/golden/supervised_eval.npz, tools/gen_golden.py::gen_supervised_eval) to 1e-12 relative.  Also the host pieces of
the feature that need no GPU: the greyscale path of the 16-bit PNG codec and the argument checks of the entry points."""
import os

import numpy as np
import pytest

from tests import helpers_supervised_eval as HS

GOLD = os.path.join(os.path.dirname(__file__), "golden", "supervised_eval.npz")


@pytest.mark.parametrize("shape", HS.GOLDEN_SHAPES)
def test_numpy_restatement_equals_the_reference(shape):
    g = np.load(GOLD)
    H, W = shape
    gt, pred = HS.u16_pair(H, W, seed=100 + HS.GOLDEN_SHAPES.index(shape))
    assert np.array_equal(gt, g["gt_%dx%d" % shape]) and np.array_equal(pred, g["pred_%dx%d" % shape])
    assert pred.min() >= 256 and 0.15 < float((gt > 0).mean()) < 0.35 and ((gt > 0) & (gt < 3)).any()
    got, n, radicand, _ = HS.sums(gt / 256.0, pred / 256.0)
    want = g["errors_%dx%d" % shape]
    assert n == int((gt > 2).sum())                           # 1 and 2 are <= 0.01 after / 256
    rel = np.abs(got - want) / np.abs(want)
    assert rel.max() <= 1e-12, "restatement vs reference, relative: %s" % rel
    assert radicand >= 1e-3


def test_png16_greyscale_round_trip_and_pil_agreement(tmp_path):
    from PIL import Image
    from fsnet_amd.monodepth.data.datasets import utils as U
    rs = np.random.RandomState(3)
    depth = rs.randint(0, 65536, size=(7, 9)).astype(np.uint16)
    U.write_png16(str(tmp_path / "w.png"), depth)
    assert np.array_equal(U.read_png16(str(tmp_path / "w.png")), depth)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "w.png"))), depth)       # PIL reads what we write
    assert np.array_equal(U.read_depth(str(tmp_path / "w.png")), (depth / 256.0).astype(np.float32))
    Image.fromarray(depth).save(str(tmp_path / "p.png"))                                  # and we read what PIL writes
    got = U.read_png16(str(tmp_path / "p.png"))
    assert got.shape == (7, 9) and got.dtype == np.uint16 and np.array_equal(got, depth)
    rgb = rs.randint(0, 65536, size=(5, 6, 3)).astype(np.uint16)                          # the colour path is unchanged
    U.write_png16(str(tmp_path / "c.png"), rgb)
    assert np.array_equal(U.read_png16(str(tmp_path / "c.png")), rgb)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from fsnet_amd.hip import binding, lib
    assert lib.fs_abi_version() == binding.ABI_VERSION
    # blocks per image depend on H*W alone: one per 8192 pixels, at most 64; ten f64 per block
    assert lib.fs_depth_errors9_workspace_bytes(1, 3, 5) == 80
    assert lib.fs_depth_errors9_workspace_bytes(3, 96, 320) == 3 * 4 * 80
    assert lib.fs_depth_errors9_workspace_bytes(32, 375, 1242) == 32 * 57 * 80
    assert lib.fs_depth_errors9_workspace_bytes(2, 2000, 2000) == 2 * 64 * 80
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.fs_depth_errors9_workspace_bytes(*bad) == -1
    assert lib.fs_depth_errors9(None, None, 1, 1, 256.0, 1, 4, 4, None, 0, None, None) == 1          # FS_EINVAL
    assert lib.fs_depth_quantize_u16(None, None, 256.0, 4, 4, None) == 1


def test_new_kernels_do_not_spill():
    from tests.test_no_spills_cpu import test_no_scratch
    test_no_scratch("eval_supervised.hip")


def test_module_has_the_reference_names():
    import inspect
    from fsnet_amd.monodepth.evaluation import kitti_supervised_eval as M
    assert list(inspect.signature(M.compute_errors).parameters) == ["image_gt", "image_pred"]
    for fn in (M.evaluate_depth, M.evaluate_depth_unsupervised_aligned):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["label_path", "result_path", "scale"] and sig.parameters["scale"].default == 256.0
    assert M.METRIC_NAMES == HS.NAMES
