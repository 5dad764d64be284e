"""Timing of the matching cost volume (informational, no threshold): ops.cost_volume (fs_cost_volume, one launch) against
the host form of ResnetEncoderMatching.match_features — plain torch ops, vectorised over batch and frames — run on the
same GPU, at the matching resolution of a 192 x 640 input: 48 x 160, C = 64, D = 96 bins, F = 2 lookup frames, B = 12.

Both compute the filled fp32 cost volume and the missing mask; the kernel also writes the masked volume into the concat
buffer, the confidence and the lowest-cost map in the same launch (the host form is not charged for those).  Each side
is warmed up, then timed --repeats times with device events around `inner` back-to-back calls; median and min-max
spread are reported, and the two results are compared at the timed size.  Writes profiles/cost_volume_bench.json.

    python tools/bench_cost_volume.py [--repeats 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fsnet_amd.hip import ops  # noqa: E402
from fsnet_amd.monodepth.networks.models.backbone.resnet_matching import intrinsics_4x4, match_features_host  # noqa: E402
from tests import helpers_matching as HM  # noqa: E402


def stats(ts):
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=len(ts))


def timed(fn, warmup, inner, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_volume_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cost_volume.py needs the GPU")
    dev = torch.device("cuda", 0)
    h, w, C, D, F, B = 48, 160, 64, 96, 2, a.batch
    g = torch.Generator().manual_seed(7)
    field = torch.nn.functional.avg_pool2d(torch.rand(B, C, h + 8, w + 8, generator=g), 5, 1, 2) * 2.0
    cur = field[:, :, 4:4 + h, 4:4 + w].contiguous().to(dev)
    look = torch.stack([field[:, :, 4:4 + h, 2:2 + w], field[:, :, 5:5 + h, 7:7 + w]], 1).contiguous().to(dev)
    poses, P2 = HM.poses_and_P2(B, F, h, w)
    K, inv_K = intrinsics_4x4(P2)
    K, inv_K = torch.from_numpy(K).float().to(dev), torch.from_numpy(inv_K).float().to(dev)
    poses = poses.to(dev)
    bins = torch.from_numpy(np.linspace(HM.MIN_BIN, HM.MAX_BIN, D)).float().to(dev)
    res = dict(h=h, w=w, C=C, D=D, F=F, B=B, bins="linear %.1f..%.1f" % (HM.MIN_BIN, HM.MAX_BIN))

    host = lambda: match_features_host(cur, look, poses, K, inv_K, bins)
    res["host_form_fp32"] = timed(host, 2, 1, a.repeats)
    want, want_missing = host()
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        cn = cur.permute(0, 2, 3, 1).contiguous().to(dtype)
        ln = look.reshape(B * F, C, h, w).permute(0, 2, 3, 1).contiguous().to(dtype)
        cat = torch.zeros(B, h, w, C + D, dtype=dtype, device=dev)
        res["kernel_%s" % tag] = timed(lambda: ops.cost_volume(cn, ln, K, inv_K, poses, bins, cat), 20, 50, a.repeats)
        res["kernel_%s_with_volume" % tag] = timed(
            lambda: ops.cost_volume(cn, ln, K, inv_K, poses, bins, cat, want_volume=True), 20, 50, a.repeats)
        if dtype == torch.float32:
            _, _, vol, missing = ops.cost_volume(cn, ln, K, inv_K, poses, bins, cat, want_volume=True)
            differ = missing != want_missing
            res["cells"] = int(differ.numel())
            res["missing_share"] = float(want_missing.mean())
            res["cells_with_another_missing_flag"] = int(differ.sum())
            res["max_abs_deviation_from_host_form"] = float((vol - want)[~differ].abs().max())
    res["host_over_kernel_fp32"] = res["host_form_fp32"]["median_ms"] / res["kernel_fp32_with_volume"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
