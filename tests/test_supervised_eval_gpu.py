"""fs_depth_errors9 / fs_depth_quantize_u16 and the kitti_supervised_eval module on the device, against the f64 numpy
restatement of the reference's compute_errors that tests/test_supervised_eval_cpu.py pins to the real function.

Bounds.  Every sum has at most 375 * 1242 = 4.7e5 non-negative f64 terms, so any two summation orders differ by at most
(n - 1) * eps ~ 1e-10 relative; device and host log differ by a few ulp.  Slots 0-5, 7, 8: 1e-9 relative.  Slot 6 is the
root of a difference, so its square is compared with the oracle's radicand to 1e-9 of the normalised squared log (the
minuend); the inputs keep the radicand >= 1e-3.  Slot 9 (the count) is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_supervised_eval as HS

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5), (7, 9), (37, 123), (96, 320), (375, 1242)]


def _as_dev(a, dev):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev)
    return torch.from_numpy(a).to(dev)


@pytest.fixture(scope="module")
def cases():
    """per shape: three uint16 pairs (the third with a single valid pixel) and their oracle rows, computed once"""
    out = {}
    for H, W in SHAPES:
        valid = 0.6 if H * W < 100 else 0.25
        pairs = [HS.u16_pair(H, W, seed=7 * H + W + k, valid=valid) for k in range(3)]
        gt2 = np.zeros((H, W), np.uint16)
        gt2[H // 2, W // 3] = 2563
        pairs[2] = (gt2, pairs[2][1])
        gt = np.stack([p[0] for p in pairs])
        pred = np.stack([p[1] for p in pairs])
        out[(H, W)] = (gt, pred, [HS.sums(g / 256.0, p / 256.0) for g, p in zip(gt, pred)])
    return out


def _check(got, oracle, tag):
    want, n, radicand, nsl = oracle
    assert int(got[9]) == n, "%s: count %d, oracle %d" % (tag, int(got[9]), n)
    for s in (0, 1, 2, 3, 4, 5, 7, 8):
        dev = abs(got[s] - want[s]) / abs(want[s]) if want[s] != 0 else abs(got[s])
        assert dev <= 1e-9, "%s: slot %d (%s) deviates %.3e relative (got %r, oracle %r)" % (tag, s, HS.NAMES[s], dev,
                                                                                          got[s], want[s])
    if n > 1:
        assert radicand >= 1e-3, "%s: oracle radicand %.3e" % (tag, radicand)
        dev = abs(got[6] ** 2 - radicand) / nsl
        assert dev <= 1e-9, "%s: slot 6 squared deviates %.3e of the normalised squared log" % (tag, dev)
    else:       # one pixel: the radicand is the rounding residue of x^2/1 - x^2/1, zero on both sides or NaN from a negative
        assert got[6] == 0.0 or np.isnan(got[6]) or got[6] ** 2 <= 1e-9 * nsl, "%s: slot 6 %r" % (tag, got[6])


@pytest.mark.parametrize("kind", ["u16_u16", "u16_f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_errors9_matches_restatement(dev, cases, shape, kind):
    from fsnet_amd.hip import ops
    gt, pred, oracle = cases[shape]
    assert shape[0] * shape[1] % 8 != 0 or shape == (96, 320)       # images 1 and 2 of the odd sizes start misaligned
    g = gt if kind == "u16_u16" else (gt / 256.0).astype(np.float32)            # exact: 16 significant bits
    got = ops.depth_errors9(_as_dev(pred, dev), _as_dev(g, dev)).cpu().numpy()
    assert got.shape == (3, 10) and got.dtype == np.float64
    assert int(got[2, 9]) == 1
    for k in range(3):
        _check(got[k], oracle[k], "%dx%d %s image %d" % (shape + (kind, k)))


@pytest.mark.parametrize("shape", SHAPES)
def test_same_bits_for_any_run_and_any_grouping(dev, cases, shape):
    from fsnet_amd.hip import ops
    gt, pred, _ = cases[shape]
    for g in (gt, (gt / 256.0).astype(np.float32)):
        p_d, g_d = _as_dev(pred, dev), _as_dev(g, dev)
        a = ops.depth_errors9(p_d, g_d).clone()
        b = ops.depth_errors9(p_d, g_d).clone()
        single = torch.cat([ops.depth_errors9(p_d[k:k + 1].clone(), g_d[k:k + 1].clone()) for k in range(3)])
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two runs differ"
        assert torch.equal(a.view(torch.int64), single.view(torch.int64)), "one per call differs from three per call"


def test_float_prediction_and_uint16_storage(dev, cases):
    """float32 / float32 and float32-pred / u16-gt run the same arithmetic; torch.uint16 storage equals int16 storage"""
    from fsnet_amd.hip import ops
    gt, pred, oracle = cases[(37, 123)]
    pf, gf = (pred / 256.0).astype(np.float32), (gt / 256.0).astype(np.float32)
    ref = ops.depth_errors9(_as_dev(pred, dev), _as_dev(gt, dev))
    for p, g in ((pf, gf), (pf, gt)):
        got = ops.depth_errors9(_as_dev(p, dev), _as_dev(g, dev))
        assert torch.equal(got.view(torch.int64), ref.view(torch.int64))
    u = ops.depth_errors9(_as_dev(pred, dev).view(torch.uint16), _as_dev(gt, dev).view(torch.uint16))
    assert torch.equal(u.view(torch.int64), ref.view(torch.int64))
    half = ops.depth_errors9(_as_dev(pred, dev), _as_dev(gt, dev), scale=128.0).cpu().numpy()
    for k in range(3):       # scale 128: every depth doubles, and a ground truth of 2 (0.0156) now counts
        _check(half[k], HS.sums(gt[k] / 128.0, pred[k] / 128.0), "scale 128 image %d" % k)
    assert half[0, 9] > ref.cpu().numpy()[0, 9]


def test_empty_valid_set(dev):
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.evaluation.kitti_supervised_eval import compute_errors
    gt = np.zeros((1, 7, 9), np.uint16)
    gt[0, 1, 1], gt[0, 2, 2] = 1, 2                        # <= 0.01 after / 256
    pred = np.full((1, 7, 9), 2560, np.uint16)
    out = ops.depth_errors9(_as_dev(pred, dev), _as_dev(gt, dev)).cpu().numpy()
    assert out[0, 9] == 0
    with pytest.raises(ValueError):
        compute_errors(gt[0] / 256.0, pred[0] / 256.0)
    with pytest.raises(ValueError):
        compute_errors(_as_dev(gt[0], dev), _as_dev(pred[0], dev))


def test_compute_errors_takes_numpy_or_device_input(dev, cases):
    from fsnet_amd.monodepth.evaluation.kitti_supervised_eval import compute_errors
    gt, pred, oracle = cases[(7, 9)]
    a = compute_errors(gt[0] / 256.0, pred[0] / 256.0)
    b = compute_errors(torch.from_numpy((gt[0] / 256.0).astype(np.float32)).to(dev), _as_dev(pred[0], dev))
    assert a.shape == (9,) and np.array_equal(a, b)
    _check(np.concatenate([a, [oracle[0][1]]]), oracle[0], "compute_errors 7x9")


def test_invalid_arguments_through_the_c_abi(dev):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import stream_ptr
    N, H, W = 2, 7, 9
    pred = torch.full((N, H, W), 2560, dtype=torch.int16, device=dev)
    gt = torch.full((N, H, W), 2000, dtype=torch.int16, device=dev)
    need = lib.fs_depth_errors9_workspace_bytes(N, H, W)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    out = torch.full((N, 10), -1.0, dtype=torch.float64, device=dev)

    def call(scale, n, h, w, nbytes):
        return lib.fs_depth_errors9(pred.data_ptr(), gt.data_ptr(), 1, 1, C.c_double(scale), n, h, w, ws.data_ptr(),
                                    nbytes, out.data_ptr(), stream_ptr())
    assert call(0.0, N, H, W, need) == 1 and call(-1.0, N, H, W, need) == 1            # FS_EINVAL
    assert call(256.0, N, H, W, need - 1) == 1                                          # short workspace
    assert call(256.0, 0, H, W, need) == 1 and call(256.0, N, 0, W, need) == 1 and call(256.0, N, H, 0, need) == 1
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())                                                    # nothing was launched
    assert call(256.0, N, H, W, need) == 0
    assert int(out.cpu()[0, 9]) == H * W


def test_depth_quantize_u16(dev):
    from fsnet_amd.hip import ops
    rng = np.random.RandomState(4)
    d = (rng.rand(7, 9) * 90).astype(np.float32)
    d.flat[:6] = [0.0, 255.999, 256.0, 1e9, -1.0, np.nan]
    d.flat[6:9] = [np.inf, -np.inf, 0.999 / 256]
    with np.errstate(invalid="ignore"):
        want = np.clip(np.trunc(d * np.float32(256)), 0, 65535)
    want[np.isnan(d)] = 0
    got = ops.depth_quantize_u16(torch.from_numpy(d).to(dev))
    assert got.dtype == torch.uint16 and tuple(got.shape) == (7, 9)
    got = got.cpu().numpy()
    assert got.dtype == np.uint16 and np.array_equal(got, want.astype(np.uint16)), (got, want)
    assert got.flat[1] == 65535 and got.flat[3] == 65535 and got.flat[4] == 0 and got.flat[5] == 0
    big = (rng.rand(96, 320) * 90).astype(np.float32)                  # the 16-byte path, more than one block
    assert np.array_equal(ops.depth_quantize_u16(torch.from_numpy(big).to(dev)).cpu().numpy(),
                          np.trunc(big * np.float32(256)).astype(np.uint16))


def test_folder_evaluation(dev, tmp_path, capsys):
    """five PNG pairs of two sizes (groups of 2, 2 and 1 consecutive equal sizes) through evaluate_depth and, with the
    ground truth as an .npz cache, evaluate_depth_unsupervised_aligned: the per-image oracle means, in the reference's
    strings"""
    from PIL import Image
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    from fsnet_amd.monodepth.evaluation import kitti_supervised_eval as M
    from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import stack_maps
    sizes = [(37, 123), (37, 123), (30, 101), (30, 101), (37, 123)]
    label, result = tmp_path / "label", tmp_path / "result"
    label.mkdir(), result.mkdir()
    rows, gts = [], []
    for k, (H, W) in enumerate(sizes):
        gt, pred = HS.u16_pair(H, W, seed=300 + k)
        Image.fromarray(gt).save(str(label / ("%010d.png" % k)))              # written by PIL, read by read_png16
        write_png16(str(result / ("%010d.png" % k)), pred)
        rows.append(HS.compute_errors(gt / 256.0, pred / 256.0))
        gts.append((gt / 256.0).astype(np.float32))
    (result / "notes.txt").write_text("not a png\n")
    want = np.array(rows).mean(0)
    np.savez_compressed(str(tmp_path / "gt.npz"), data=stack_maps(gts))
    for fn, lab in ((M.evaluate_depth, str(label)), (M.evaluate_depth_unsupervised_aligned, str(tmp_path / "gt.npz"))):
        texts = fn(lab, str(result))
        printed = capsys.readouterr().out
        assert "totally found 5 images in %s and %s" % (lab, str(result)) in printed and "Notice" not in printed
        assert len(texts) == 9
        for i, text in enumerate(texts):
            head, value = text.rsplit(" : ", 1)
            assert head == "mean " + HS.NAMES[i] and text.endswith("\n")
            dev_rel = abs(float(value) - want[i]) / want[i]
            assert dev_rel <= 1e-9, "%s %s: %.3e relative" % (fn.__name__, HS.NAMES[i], dev_rel)
    M.main([str(label), str(result)])
    assert capsys.readouterr().out.splitlines()[-9].startswith("mean mae : ")
