"""Timing of the motion-mask precompute on one MI355X: ops.optical_flow_farneback + ops.motion_mask per frame pair at
375x1242 with pyr_scale 0.5, levels 3, winsize 15, iterations 3, poly_n 5, poly_sigma 1.2, flags 0 (B = 1 and
B = 8; device events around `--steps` calls after `--warmup`), and MotionMaskPrecomputeHook end to end (frames/s over a
generated KITTI-raw tree of 375x1242 PNGs, PNG decode and encode included).  Prints one JSON line.
    python tools/bench_motion_mask.py > profiles/motion_mask_bench.json"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fsnet_amd.hip import ops  # noqa: E402
from tests import helpers_kitti as HK  # noqa: E402
from tests import helpers_optflow as HO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-hook", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, W = 375, 1242
    pairs = [HO.corridor_pair(H, W, seed=s) for s in range(8)]
    i0 = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    i1 = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    P2 = torch.from_numpy(np.stack([p[2] for p in pairs])).to(dev)
    T = torch.from_numpy(np.stack([p[3] for p in pairs])).to(dev)
    res = {"params": dict(HO.FLOW_CFG), "size": [H, W], "steps": args.steps, "warmup": args.warmup, "gpu": {}}
    for B in (1, 8):
        ws = torch.empty(ops.optflow_workspace_bytes(B, H, W, **HO.FLOW_CFG), dtype=torch.uint8, device=dev)
        out = torch.empty(B, H, W, 2, device=dev)

        def call():
            ops.optical_flow_farneback(i0[:B], i1[:B], workspace=ws, out=out, **HO.FLOW_CFG)
            ops.motion_mask(out, P2[:B], T[:B], 5.0, 0)
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        res["gpu"]["B%d" % B] = {"ms_per_call": round(ms, 4), "ms_per_pair": round(ms / B, 4),
                                 "workspace_MB": round(ws.numel() / 2 ** 20, 1)}
    if not args.no_hook:
        from fsnet_amd.monodepth.pipeline_hooks.precomputing_hooks.base_precompute_hooks import MotionMaskPrecomputeHook
        with tempfile.TemporaryDirectory() as d:
            raw, split = HK.make_tree(d, seed=5, H=H, W=W)
            cfg = dict(HK.dataset_cfg(raw, split, prefix='fsnet_amd.'),
                       name='fsnet_amd.monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset', is_filter_static=False)
            for kw in (dict(), dict(batch_size=5, num_workers=4)):
                hook = MotionMaskPrecomputeHook(cfg, HO.FLOW_CFG, output_dir=os.path.join(d, "m%d" % len(kw)), **kw)
                n = len(hook.dataset)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(sys.stderr):       # the hook's progress line: stdout is the JSON
                    hook()
                torch.cuda.synchronize()
                res["hook_frames_per_s" + ("_batched" if kw else "")] = round(n / (time.perf_counter() - t0), 2)
            res["hook_frames"] = n
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
