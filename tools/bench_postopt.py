"""Timing of the sparse-VO depth post-optimisation (ops.post_optimize -> fs_postopt) on one MI355X at the hook
defaults (h_seg 10, w_seg 18, 3 SLIC iterations, max_points 800): 192x640 and 320x1024 at B = 1 and B = 8, device
events around `--steps` calls after `--warmup`, all launches included.  Prints one JSON line; the CPU restatement's
time per image (tests/helpers_postopt.py, torch on the host) is printed beside it as context, not as a target.
    python tools/bench_postopt.py > profiles/<name>.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fsnet_amd.hip import ops  # noqa: E402
from tests import helpers_postopt as HP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement's timing")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"params": "hook defaults", "steps": args.steps, "warmup": args.warmup, "gpu": {}}
    for H, W in ((192, 640), (320, 1024)):
        scenes = [HP.synthetic_scene(H, W, 300 + i, vo_frac=0.02, vo_noise=0.05) for i in range(8)]
        image, pred, vo = [torch.from_numpy(np.stack([s[j] for s in scenes])).to(dev) for j in (0, 2, 3)]
        for B in (1, 8):
            call = lambda: ops.post_optimize(image[:B], pred[:B], vo[:B], rgb_mean=HP.IMAGENET_MEAN,   # noqa: E731
                                             rgb_std=HP.IMAGENET_STD, **HP.HOOK_DEFAULTS)
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
            res["gpu"]["%dx%d_B%d" % (H, W, B)] = {"ms_per_call": round(ms, 4), "ms_per_image": round(ms / B, 4)}
    if not args.no_cpu:
        image, _, pred, vo = HP.synthetic_scene(192, 640, 300, vo_frac=0.02, vo_noise=0.05)
        t0 = time.perf_counter()
        HP.post_optimize(image, pred, vo, **HP.HOOK_DEFAULTS)
        res["cpu_restatement_ms_per_image_192x640"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
