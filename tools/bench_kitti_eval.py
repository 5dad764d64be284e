"""Timing of the KITTI evaluation paths that moved to the device (informational, no threshold):

  - the Eigen ground-truth export: KittiEigenEvaluator over --frames split lines of the synthetic KITTI-raw tree of
    tests/helpers_kitti.py at 375x1242 with --points points per scan, with export_on_device (scans read from disk,
    fs_lidar_pinhole_depth per group, maps copied back) and without (generate_depth_map per scan on the host); no cache
    file is written, and the two exports are compared pixel by pixel;
  - the supervised metrics: evaluate_depth over --frames pairs of 375x1242 16-bit PNGs (decode on the host, upload,
    fs_depth_errors9 per group of 32) against the same files through the vectorised numpy restatement of compute_errors
    (tests/helpers_supervised_eval.py; the reference's per-pixel loop is slower still), and the kernels alone.

Each is warmed up once and repeated --repeats times; the median and the min-max spread are reported.  Writes
profiles/kitti_eval_bench.json.

    python tools/bench_kitti_eval.py [--repeats 5] [--frames 64] [--points 120000]
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
from fsnet_amd.monodepth.data.datasets.utils import read_png16, write_png16  # noqa: E402
from fsnet_amd.monodepth.evaluation import kitti_supervised_eval as SE  # noqa: E402
from fsnet_amd.monodepth.evaluation.kitti_unsupervised_eval import KittiEigenEvaluator  # noqa: E402
from tests import helpers_kitti as HK  # noqa: E402
from tests import helpers_supervised_eval as HS  # noqa: E402

H, W = 375, 1242


def stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=len(ts))


def timed(fn, repeats):
    fn()                                                        # warm-up: code objects, file cache
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()                                              # every path ends with its result on the host
        ts.append(time.perf_counter() - t0)
    return stats(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--group-size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kitti_eval.py needs the GPU")
    dev = torch.device("cuda", 0)
    res = dict(H=H, W=W, frames=a.frames, points_per_scan=a.points, group_size=a.group_size)
    with tempfile.TemporaryDirectory() as d:
        raw, _ = HK.make_tree(d, H=H, W=W)
        HK.add_velodyne(raw, H=H, W=W, npts=a.points)
        split = os.path.join(d, "bench_split.txt")
        with open(split, "w") as f:
            for i in range(a.frames):
                f.write("%s/%s %d l\n" % (HK.DATE, HK.DRIVE, i % HK.NFRAMES))

        def export(on_device):
            return KittiEigenEvaluator(data_path=raw, split_file=split, gt_saved_file=None, device=dev,
                                       export_on_device=on_device, group_size=a.group_size).gt_depths
        res["device_export"], got = timed(lambda: export(True), a.repeats)
        res["host_export"], want = timed(lambda: export(False), a.repeats)
        res["export_mismatching_pixels"] = int(sum(int((g != w).sum()) for g, w in zip(got, want)))
        res["export_pixels_hit_frame0"] = int((got[0] > 0).sum())

        label, result = os.path.join(d, "label"), os.path.join(d, "result")
        os.makedirs(label), os.makedirs(result)
        for i in range(a.frames):
            gt, pred = HS.u16_pair(H, W, seed=i)
            write_png16(os.path.join(label, "%010d.png" % i), gt)
            write_png16(os.path.join(result, "%010d.png" % i), pred)

        def numpy_eval():
            rows = [HS.compute_errors(read_png16(os.path.join(label, n)) / 256.0, read_png16(os.path.join(result, n)) / 256.0)
                    for n in sorted(os.listdir(label))]
            return np.array(rows).mean(0)

        def device_eval():
            return np.array([float(t.rsplit(" : ", 1)[1]) for t in SE.evaluate_depth(label, result)])
        res["device_evaluate_depth"], got = timed(device_eval, a.repeats)
        res["numpy_evaluate_depth"], want = timed(numpy_eval, a.repeats)
        res["evaluate_depth_max_relative_deviation"] = float((np.abs(got - want) / np.abs(want)).max())
        t0 = time.perf_counter()
        planes = [read_png16(os.path.join(label, n)) for n in sorted(os.listdir(label))]
        res["png_decode_ms_per_file"] = (time.perf_counter() - t0) * 1e3 / len(planes)
        # the kernels alone: a group of 32 staged once, events around `inner` back-to-back calls
        G = min(32, a.frames)
        g_d = torch.from_numpy(np.stack(planes[:G]).view(np.int16)).to(dev)
        p_d = torch.from_numpy(np.stack([read_png16(os.path.join(result, "%010d.png" % i)) for i in range(G)])
                               .view(np.int16)).to(dev)
        inner = 50
        for _ in range(5):
            ops.depth_errors9(p_d, g_d)
        ts = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                ops.depth_errors9(p_d, g_d)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3 / inner / G)
        res["errors9_kernels_per_image_G%d" % G] = stats(ts)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
