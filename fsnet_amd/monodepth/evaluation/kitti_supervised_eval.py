"""The KITTI depth-benchmark metrics with the reference's names and signatures (monodepth/evaluation/
kitti_supervised_eval.py): compute_errors, evaluate_depth over two folders of 16-bit PNGs, and
evaluate_depth_unsupervised_aligned over an `.npz` ground-truth cache and a folder of PNGs.  The reference walks every
pixel in a Python double loop under numba; here the raw uint16 planes are uploaded as they are and the division by
`scale`, the valid test and the nine f64 sums are one fs_depth_errors9 call for up to 32 images of one size
(ops.depth_errors9).  The PNGs are decoded by read_png16 on the host.

    python -m fsnet_amd.monodepth.evaluation.kitti_supervised_eval LABEL RESULT
"""
import os

import numpy as np
import torch

from fsnet_amd.hip import ops
from fsnet_amd.monodepth.data.datasets.utils import read_png16

METRIC_NAMES = ["mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log",
                "abs relative", "squared relative"]
MAX_GROUP = 32        # images per fs_depth_errors9 call


def _to_device(a, device):
    """a device tensor as it is; a host array as float32 or, for a 16-bit plane, as its raw bits"""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a
    a = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    if a.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(device)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def compute_errors(image_gt, image_pred):
    """The nine errors of two depth images [H, W] (reference :7-81): mae, rmse, inverse mae, inverse rmse, log mae,
    log rmse, scale invariant log, abs relative, squared relative, over the pixels with image_gt > 0.01, as a float64
    array [9].  Inputs are numpy arrays or device tensors, in metres; a host array that is not uint16 is taken as
    float32 (the arithmetic after that is f64, as in the reference), a uint16 one as a raw PNG plane over 256.

    Deliberate deviation: raises ValueError when no pixel is valid.  The reference divides by the zero pixel count
    there: NaN from plain numpy, a ZeroDivisionError under numba."""
    gt, pred = _to_device(image_gt, _device()), _to_device(image_pred, _device())
    out = ops.depth_errors9(pred[None], gt[None])[0].cpu().numpy()
    if out[9] == 0:
        raise ValueError("compute_errors: no pixel with ground truth > 0.01")
    return out[:9]


def _errors_of_pairs(gts, preds, scale):
    """gts, preds: equally long lists of host arrays [H, W] (uint16 planes, or float32 metres for a cached ground
    truth).  Consecutive pairs of one size and kind go to the device together, at most MAX_GROUP per call.  -> [n, 9]"""
    dev = _device()
    rows, start = [], 0
    while start < len(preds):
        key = (gts[start].shape, gts[start].dtype, preds[start].shape)
        stop = start
        while stop < len(preds) and stop - start < MAX_GROUP and \
                (gts[stop].shape, gts[stop].dtype, preds[stop].shape) == key:
            stop += 1
        out = ops.depth_errors9(_to_device(np.stack(preds[start:stop]), dev), _to_device(np.stack(gts[start:stop]), dev),
                                scale).cpu().numpy()
        if (out[:, 9] == 0).any():
            raise ValueError("image %d has no pixel with ground truth > 0.01" % (start + int(np.argmin(out[:, 9]))))
        rows.append(out[:, :9])
        start = stop
    return np.concatenate(rows)


def _texts(error_vectors):
    return ["mean {} : {}\n".format(name, np.mean(error_vectors[:, i])) for i, name in enumerate(METRIC_NAMES)]


def _png_list(path):
    return [os.path.join(path, name) for name in sorted(os.listdir(path)) if name.endswith(".png")]


def evaluate_depth_unsupervised_aligned(label_path, result_path, scale=256.0):
    """label_path: the `.npz` ground-truth cache of the evaluators (key `data`, metres); result_path: a folder of
    16-bit PNGs.  Despite the name no alignment (median scaling) is done: the reference (:83-120) does none."""
    gt_depths = np.load(label_path, fix_imports=True, encoding='latin1', allow_pickle=True)["data"]
    result_list = _png_list(result_path)
    if not len(gt_depths) == len(result_list):
        print("Notice: the lenght of gt_list {} is not the same as the result_list {}".format(len(gt_depths),
                                                                                              len(result_list)))
    print("totally found {} images in {} and {}".format(len(gt_depths), label_path, result_path))
    gts = [np.asarray(gt_depths[i], dtype=np.float32) for i in range(len(gt_depths))]
    preds = [read_png16(result_list[i]) for i in range(len(gt_depths))]
    return _texts(_errors_of_pairs(gts, preds, scale))


def evaluate_depth(label_path, result_path, scale=256.0):
    """label_path, result_path: folders of 16-bit PNGs, paired in sorted order (reference :122-157)"""
    gt_list = _png_list(label_path)
    result_list = _png_list(result_path)
    if not len(gt_list) == len(result_list):
        print("Notice: the lenght of gt_list {} is not the same as the result_list {}".format(len(gt_list),
                                                                                              len(result_list)))
    print("totally found {} images in {} and {}".format(len(gt_list), label_path, result_path))
    gts = [read_png16(p) for p in gt_list]
    preds = [read_png16(result_list[i]) for i in range(len(gt_list))]
    return _texts(_errors_of_pairs(gts, preds, scale))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="KITTI depth-benchmark metrics of a folder of 16-bit depth PNGs")
    ap.add_argument("label_path", help="folder of ground-truth PNGs, or the .npz ground-truth cache of an evaluator")
    ap.add_argument("result_path", help="folder of predicted depth PNGs (uint16(depth * scale))")
    ap.add_argument("--scale", type=float, default=256.0)
    args = ap.parse_args(argv)
    fn = evaluate_depth if os.path.isdir(args.label_path) else evaluate_depth_unsupervised_aligned
    for text in fn(args.label_path, args.result_path, args.scale):
        print(text, end="")


if __name__ == "__main__":
    main()
