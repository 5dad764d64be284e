"""Timing of the nuScenes ground-truth export (informational, no threshold): --samples samples x 6 cameras x 900 x 1600
with --points points each (the shapes of NuscenesEvaluator._precompute on the real data), three stages timed apart:

  - device: the inputs staged once, then fs_lidar_nusc_depth_u16 (init, scatter, gather) for all samples in one call —
    device events around `inner` back-to-back calls — and the same call followed by the copy of the uint16 planes to
    the host, a host clock around work that ends in that copy;
  - host mirror: nuscenes_unsupervised_eval.nusc_depth_u16 per sample and camera (vectorised numpy; the reference's own
    Counter loop is slower still and is not timed here);
  - PNG encode: write_png16 of the planes (zlib, host), which either path pays.

Each is warmed up once and repeated --repeats times, the device and host stages alternating; the median and the min-max
spread are reported.  The two exports are compared pixel by pixel at the timed size.  Bytes the device stage must move:
16 B written (init) + 16 B read (gather) + 2 B written per pixel, plus the points once per camera.
Writes profiles/nusc_gt_bench.json.

    python tools/bench_nusc_gt.py [--repeats 7] [--samples 4] [--points 34720]
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
from fsnet_amd.monodepth.data.datasets.utils import write_png16  # noqa: E402
from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as E  # noqa: E402
from tests import helpers_nusc as HN  # noqa: E402

H, W = 900, 1600


def stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=len(ts))


def case(samples, points, seed=3):
    """the six cameras of tests/helpers_nusc.py at 900 x 1600 and a ring of points around the car per sample"""
    cams = HN.cameras()
    M = np.zeros((samples, len(HN.CAMS), 3, 4))
    for c, cam in enumerate(HN.CAMS):
        t, q, K = cams[cam]
        K = np.array(K) * np.array([[40.0], [37.5], [1.0]])
        M[:, c] = E.projection_matrix(E.camera_extrinsics(dict(rotation=q, translation=t)), K)[:3]
    rng = np.random.RandomState(seed)
    scans = []
    for _ in range(samples):
        ang = rng.uniform(0, 2 * np.pi, points)
        dist = np.exp(rng.uniform(np.log(2.5), np.log(100.0), points))
        ego = np.stack([dist * np.cos(ang), dist * np.sin(ang), rng.uniform(-1.0, 4.0, points) + 0.02 * dist], 1)
        k = points // 5
        ego[-k:] = ego[:k] * rng.uniform(1.0, 1.002, (k, 1))                  # second returns: duplicate pixels
        scans.append(np.concatenate([ego, rng.rand(points, 1)], 1).astype(np.float32))
    return scans, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--points", type=int, default=34720)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nusc_gt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nusc_gt.py needs the GPU")
    dev = torch.device("cuda", 0)
    G, C = a.samples, len(HN.CAMS)
    scans, M = case(G, a.points)
    res = dict(H=H, W=W, samples=G, cameras=C, points_per_sample=a.points)
    res["device_bytes_per_call"] = int(G * C * H * W * 34 + G * C * a.points * 16)
    op = ops.LidarNuscDepth(G, C, H, W, dev)
    op.stage(scans, M)

    def device_export():
        return op.run().cpu().numpy()

    def host_export():
        return np.stack([np.stack([E.nusc_depth_u16(s, M[g, c], [H, W]) for c in range(C)])
                         for g, s in enumerate(scans)])

    got, want = device_export(), host_export()                                # warm-up: code objects, allocations
    res["mismatching_pixels"] = int((got != want).sum())
    res["pixels_hit"] = int((want != 0).sum())
    ts = dict(device_export=[], host_mirror=[])
    for _ in range(a.repeats):                                                # alternating: the host is shared
        for tag, fn in (("device_export", device_export), ("host_mirror", host_export)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                              # the device path ends in a copy to the host
            ts[tag].append(time.perf_counter() - t0)
    for tag in ts:
        res[tag] = stats(ts[tag])
    # the kernels alone: events around `inner` back-to-back calls of all samples
    inner = 20
    for _ in range(3):
        op.run()
    ks = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            op.run()
        e1.record()
        torch.cuda.synchronize()
        ks.append(e0.elapsed_time(e1) / 1e3 / inner)
    res["device_kernels"] = stats(ks)
    res["device_kernels_GB_per_s"] = res["device_bytes_per_call"] / (res["device_kernels"]["median_ms"] * 1e-3) / 1e9
    with tempfile.TemporaryDirectory() as d:
        es = []
        for r in range(a.repeats + 1):
            t0 = time.perf_counter()
            for g in range(G):
                for c in range(C):
                    write_png16(os.path.join(d, "%d_%d.png" % (g, c)), want[g, c])
            if r:                                                             # the first round is the warm-up
                es.append(time.perf_counter() - t0)
        res["png_encode"] = stats(es)
    for tag in ("device_export", "host_mirror", "device_kernels", "png_encode"):
        res[tag]["per_sample_ms"] = res[tag]["median_ms"] / G
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
