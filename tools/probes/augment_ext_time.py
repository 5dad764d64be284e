"""Time of the extended input-pipeline launch beside the one it stands next to, at the reference's training shape:
batch 12 x 3 frames of 375x1242 uint8 -> 192x640.  HIP events around each launch, median of --iters after warm-up:
  old    fs_augment_frames, three colour ops
  ext    fs_augment_frames_ext on the same plan (full-canvas window, the same three ops, split 0)
  ext_e  fs_augment_frames_ext with the op list of the tests' case e (brightness, HSV with hue and saturation,
         eigenvalue noise, contrast | Copy | brightness: five slots, split 4, an f64 tail)
  resize      fs_resize_frames in its training form (plan rows, original, mask), the frames resized to the output
  resize_ext  fs_resize_frames_ext on the same plan
  masks       fs_augment_masks, one uint8 plane per sample through the warp's plan
Prints one JSON line.
    python tools/probes/augment_ext_time.py [--iters 50]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from fsnet_amd.hip.binding import lib, check, stream_ptr, FsAugArgs, FsAugExtArgs, FsResizeArgs  # noqa: E402


def median_us(launch, iters):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, F, Hs, Ws, H, W = 12, 3, 375, 1242, 192, 640
    rs = np.random.RandomState(0)
    src = torch.from_numpy(rs.randint(0, 256, size=(B, F, Hs, Ws, 3)).astype(np.uint8)).to(dev)
    scale = rs.uniform(0.45, 0.75, size=B)                       # forward scale of RandomWarpAffine at this shape
    minv = np.zeros((B, 6))
    minv[:, 0] = minv[:, 4] = 1.0 / scale
    minv[:, 2], minv[:, 5] = rs.uniform(0, 100, size=B), rs.uniform(0, 40, size=B)
    mirror = (np.arange(B) % 2).astype(np.int32)
    iplan = np.zeros((B, 8), np.int32)
    iplan[:, 0:3], iplan[:, 3], iplan[:, 4], iplan[:, 5], iplan[:, 6] = [0, 1, 2], 15, mirror, Hs, Ws
    fplan = np.tile(np.array([12.5, 1.2, 0.8, 0.0], np.float32), (B, 1))
    dims = np.tile(np.array([Hs, Ws, 0, 0], np.int32), (B, 1))
    win = np.array([[1, W - 1, 0, 0, 0, W, H, 0] if m else [0, 0, 0, 0, 0, W, H, 0] for m in mirror], np.int32)
    codes3 = np.tile(np.array([0, 1, 2 | 1 << 4, 4, 4, 4, 4, 4], np.int32), (B, 1))
    vals3 = np.zeros((B, 8, 3))
    vals3[:, 0, 0], vals3[:, 1, 0], vals3[:, 2, 0] = fplan[0, 0], fplan[0, 1], fplan[0, 2]
    codes_e = np.tile(np.array([0, 2 | 3 << 4, 3, 1, 0, 4, 4, 4], np.int32), (B, 1))
    vals_e = np.zeros((B, 8, 3))
    vals_e[:, 0, 0], vals_e[:, 1, :2], vals_e[:, 2], vals_e[:, 3, 0], vals_e[:, 4, 0] = 12.5, [0.8, 95.0], [3.1, -2.2, 0.7], 1.2, -9.0
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(minv=minv, iplan=iplan, fplan=fplan, dims=dims, win=win,
                                                         codes3=codes3, vals3=vals3, codes_e=codes_e, vals_e=vals_e).items()}
    image = torch.empty(F, B, 3, H, W, device=dev)
    orig = torch.empty_like(image)
    mask = torch.empty(B, H, W, dtype=torch.float64, device=dev)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    a = FsAugArgs()
    a.src, a.minv, a.iplan, a.fplan = src.data_ptr(), t["minv"].data_ptr(), t["iplan"].data_ptr(), t["fplan"].data_ptr()
    a.image, a.original, a.mask = image.data_ptr(), orig.data_ptr(), mask.data_ptr()
    x = FsAugExtArgs()
    x.src, x.minv, x.dims, x.win = src.data_ptr(), t["minv"].data_ptr(), t["dims"].data_ptr(), t["win"].data_ptr()
    x.image, x.original, x.mask = image.data_ptr(), orig.data_ptr(), mask.data_ptr()
    for k in range(3):
        a.mean[k], a.std[k], x.mean[k], x.std[k] = mean[k], std[k], mean[k], std[k]
    a.B, a.F, a.Hs, a.Ws, a.H, a.W = B, F, Hs, Ws, H, W
    x.B, x.F, x.Hs, x.Ws, x.H, x.W = B, F, Hs, Ws, H, W
    out = {"old_us": median_us(lambda: check(lib.fs_augment_frames(C.byref(a), stream_ptr()), "old"), args.iters)}
    want = image.clone()
    x.ops, x.opv, x.n_ops, x.split = t["codes3"].data_ptr(), t["vals3"].data_ptr(), 3, 0
    out["ext_us"] = median_us(lambda: check(lib.fs_augment_frames_ext(C.byref(x), stream_ptr()), "ext"), args.iters)
    out["ext_equals_old"] = bool(torch.equal(image, want))
    x.ops, x.opv, x.n_ops, x.split = t["codes_e"].data_ptr(), t["vals_e"].data_ptr(), 5, 4
    out["ext_e_us"] = median_us(lambda: check(lib.fs_augment_frames_ext(C.byref(x), stream_ptr()), "ext_e"), args.iters)
    rdims = torch.from_numpy(np.tile(np.array([Hs, Ws, H, W], np.int32), (B, 1))).to(dev)
    r = FsResizeArgs()
    r.src, r.dims, r.iplan, r.fplan = src.data_ptr(), rdims.data_ptr(), t["iplan"].data_ptr(), t["fplan"].data_ptr()
    r.image, r.original, r.mask = image.data_ptr(), orig.data_ptr(), mask.data_ptr()
    for k in range(3):
        r.mean[k], r.std[k] = mean[k], std[k]
    r.B, r.F, r.Hs, r.Ws, r.H, r.W = B, F, Hs, Ws, H, W
    out["resize_us"] = median_us(lambda: check(lib.fs_resize_frames(C.byref(r), stream_ptr()), "resize"), args.iters)
    want = image.clone()
    x.minv, x.dims = None, rdims.data_ptr()
    x.ops, x.opv, x.n_ops, x.split = t["codes3"].data_ptr(), t["vals3"].data_ptr(), 3, 0
    out["resize_ext_us"] = median_us(lambda: check(lib.fs_resize_frames_ext(C.byref(x), stream_ptr()), "resize_ext"),
                                     args.iters)
    out["resize_ext_equals_old"] = bool(torch.equal(image, want))
    plane = torch.from_numpy(rs.randint(0, 2, size=(B, Hs, Ws)).astype(np.uint8)).to(dev)
    warped = torch.empty(B, H, W, device=dev)
    out["masks_us"] = median_us(lambda: check(lib.fs_augment_masks(
        plane.data_ptr(), t["minv"].data_ptr(), None, t["iplan"].data_ptr(), warped.data_ptr(), B, Hs, Ws, H, W,
        stream_ptr()), "masks"), args.iters)
    out = {k: round(v, 1) if isinstance(v, float) else v for k, v in out.items()}
    out["workload"] = "B=%d x %d frames %dx%d u8 -> %dx%d, median of %d" % (B, F, Hs, Ws, H, W, args.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
