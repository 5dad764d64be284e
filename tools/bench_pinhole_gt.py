"""Timing of Kitti360Evaluator._precompute (informational, no threshold): the validation split of the synthetic
KITTI-360 tree of tests/helpers_kitti360_persp.py with its scans scaled to --points points each, exported

  - on the device: Kitti360Evaluator._precompute as it ships (split and image sizes read on the host, scans read from
    disk, fs_lidar_pinhole_depth per group, maps copied back; no cache file written), and the kernels alone per frame;
  - on the host: the same loop with monodepth_utils.project_depth_map per frame (the vectorised mirror of the
    reference's export; the reference's own Counter loop is slower still and is not timed here).

Each is warmed up once and repeated --repeats times; the median and the min-max spread are reported.  The two exports
are compared pixel by pixel at the timed size.  Writes profiles/pinhole_gt_bench.json.

    python tools/bench_pinhole_gt.py [--repeats 7] [--points 120000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fsnet_amd.hip import ops  # noqa: E402
from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import Kitti360Evaluator  # noqa: E402
from fsnet_amd.monodepth.networks.utils.monodepth_utils import project_depth_map  # noqa: E402
from tests import helpers_kitti360_persp as HP  # noqa: E402


def stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--group-size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinhole_gt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinhole_gt.py needs the GPU")
    dev = torch.device("cuda", 0)
    res = dict(H=HP.H, W=HP.W, frames=len(HP.EVAL_FRAMES), points_per_scan=a.points, group_size=a.group_size)
    with tempfile.TemporaryDirectory() as d:
        raw, _, val = HP.make_tree(d, npts=a.points)
        ev = Kitti360Evaluator(gt_depths=[np.zeros((2, 2), np.float32)], device=dev, group_size=a.group_size)

        def device_export():
            ev._precompute(raw, val, None)
            return ev.gt_depths

        def host_export():
            from PIL import Image
            from fsnet_amd.monodepth.data.datasets.utils import read_pc_from_bin
            ev._load_calib(os.path.join(raw, "calibration"))
            P = ev.velo_to_image()
            out = []
            for line in open(val).readlines():
                seq, _, img_index, _, _ = line.strip().split(',')
                velo = read_pc_from_bin(os.path.join(raw, "data_3d_raw", seq, "velodyne_points/data",
                                                     "%010d.bin" % int(img_index)))
                with Image.open(os.path.join(raw, "data_2d_raw", seq, "image_00", "data_rect",
                                             "%010d.png" % int(img_index))) as im:
                    shape = np.array(im.size)[::-1].astype(np.int32)
                out.append(project_depth_map(velo, P, shape).astype(np.float32))
            return out

        for tag, fn in (("device_precompute", device_export), ("host_precompute", host_export)):
            fn()                                                        # warm-up: code objects, file cache
            ts = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                maps = fn()                                             # the device path ends in a copy to the host
                ts.append(time.perf_counter() - t0)
            res[tag] = stats(ts)
            res[tag + "_pixels_hit"] = [int((m > 0).sum()) for m in maps]
        got, want = device_export(), host_export()
        res["mismatching_pixels"] = [int((g != w).sum()) for g, w in zip(got, want)]
        # the kernels alone: inputs staged once, events around `inner` back-to-back calls
        scans = [HP.scan(raw, i) for i in HP.EVAL_FRAMES]
        G = len(scans)
        op = ops.LidarPinholeDepth(G, HP.H, HP.W, dev)
        op.stage(scans, np.stack([ev.velo_to_image()] * G))
        inner = 200
        for _ in range(20):
            op.run()
        ts = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                op.run()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3 / inner / G)
        res["kernels_per_frame_G%d" % G] = stats(ts)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
