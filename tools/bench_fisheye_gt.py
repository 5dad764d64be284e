"""Timing of the KITTI-360 fisheye ground truth and metric on the device (informational, no threshold):
fs_lidar_mei_depth per frame at G = 1 and G = 8 frames per call, fs_depth_eval_masked per image, at 1400 x 1400 with
about 120k points per scan, and tests/helpers_kitti360.py's numpy restatement of the reference's ground truth on the
host for context.  Writes profiles/fisheye_gt_bench.json.

    python tools/bench_fisheye_gt.py [--iters 20]
    rocprofv3 --kernel-trace --stats -d <dir> -o fisheye_gt -- python tools/bench_fisheye_gt.py --iters 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fsnet_amd.hip import ops  # noqa: E402
from tests import helpers_kitti360 as HK  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisheye_gt_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    H = W = 1400
    from fsnet_amd.vision_base.data.datasets.synthetic import synthetic_mei_calib
    P32, calib = synthetic_mei_calib(H, W, 0)
    P = P32.astype(np.float64)
    T00, _, T02, _, T_cam2velo = HK.extrinsics()
    T = np.linalg.inv(T02) @ T00 @ np.linalg.inv(T_cam2velo)
    mei = np.array([P[0, 0], P[1, 1], P[0, 2], P[1, 2], calib["distortion_parameters"]["k1"],
                    calib["distortion_parameters"]["k2"], calib["mirror_parameters"]["xi"]])
    rng = np.random.RandomState(0)
    scans = [HK.scene(rng, a.points) for _ in range(8)]
    res = dict(H=H, W=W, points_per_scan=a.points, iters=a.iters)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for G in (1, 8):
        op = ops.LidarMeiDepth(G, H, W, dev)
        op.stage(scans[:G], np.stack([T] * G), np.stack([mei] * G))
        res["lidar_mei_depth_ms_per_frame_G%d" % G] = timed(op.run, a.iters) / G
    gt = op.depth.clone()
    mask = op.close_mask.clone()
    pred = torch.rand(8, 700, 700, device=dev) * 30 + 0.5
    res["depth_eval_masked_ms_per_image_B1"] = timed(lambda: ops.depth_eval_masked(pred[:1], gt[:1], mask[:1]), a.iters)
    res["depth_eval_masked_ms_per_image_B8"] = timed(lambda: ops.depth_eval_masked(pred, gt, mask), a.iters) / 8
    t0 = time.perf_counter()
    for s in scans[:2]:
        HK.ground_truth(s, T, P, calib, H=H, W=W)
    res["host_numpy_ms_per_frame"] = (time.perf_counter() - t0) / 2 * 1e3
    res["gt_pixels_per_frame"] = float((gt > 0).sum().item()) / 8
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
