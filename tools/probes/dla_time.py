"""Time forward + backward of DLA-34 at 12 x 3 x 192 x 640 (the headline batch) in bf16 and fp32:
  (a) the HIP runner (fsnet_amd/engine/dla_net.py), and
  (b) the module's own torch path (DLA.forward_torch) on the device in the same dtype — fp32 parameters, or the module
      cast to bf16 — the baseline the runner has to beat.
Both run the whole training-mode call: forward on an fp32 NCHW image batch, backward from one cotangent per feature of
out_indices (1, 2, 3, 4, 5), parameter gradients accumulated.  Device events around `--steps` calls after `--warmup`,
`--repeat` windows with the two variants alternating inside every window, the median window reported (and the best).
Then one more profiled call of the runner with the launch profile on and the weight gradients inline: per level the sum
of its forward and backward launch times (the launches alone, without the gaps between them).
One JSON line per dtype.  Nothing is asserted.

    python tools/probes/dla_time.py --steps 10 --warmup 3 --repeat 5

Compare within one job only: boxes differ by +-2 % (README)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def per_level(runner, records):
    """{level: {"fwd": ms, "bwd": ms, "launches": n}} from the runner's marks into the launch-profile records"""
    out = {}
    marks = runner.marks
    for (lo, phase, name), (hi, _, _) in zip(marks, marks[1:]):
        if name == "end":
            continue
        ent = out.setdefault(name, {"fwd": 0.0, "bwd": 0.0, "launches": 0})
        ent[phase] += sum(r[2] for r in records[lo:hi]) * 1e3
        ent["launches"] += hi - lo
    return {k: {a: (round(b, 3) if a != "launches" else b) for a, b in v.items()} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fsnet_amd.engine.handover import HO
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip.conv import LaunchProfile
    from fsnet_amd.vision_base.networks.models.backbone.dla import dla34
    dev = torch.device("cuda", 0)
    N, H, W = args.batch, args.height, args.width
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=gen).to(dev)
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        RT.set_compute_dtype(tag)
        torch.manual_seed(2)
        hip = dla34(pretrained=None, out_indices=(1, 2, 3, 4, 5)).to(dev).train()
        ref = dla34(pretrained=None, out_indices=(1, 2, 3, 4, 5)).to(dev).train()
        ref.load_state_dict(hip.state_dict())
        ref = ref.to(dtype)
        xr = x.to(dtype)
        cots = [torch.randn(N, c, H >> i, W >> i, generator=gen).to(dev, dtype) for i, c in zip(range(1, 6), hip.channels[1:])]

        def run_hip():
            torch.autograd.backward(hip(x), cots)
            HO.join_companions_final()

        def run_torch():
            torch.autograd.backward(ref.forward_torch(xr), cots)

        times = {"hip": [], "torch": []}
        for _ in range(args.repeat):
            times["hip"].append(timed(run_hip, args.steps, args.warmup))
            times["torch"].append(timed(run_torch, args.steps, args.warmup))
        # one profiled call: weight gradients inline so that every launch lands between its level's marks
        streams, RT.wgrad_streams = RT.wgrad_streams, 0
        runner = hip._runner
        runner.marks = []
        LaunchProfile.begin()
        run_hip()
        records = LaunchProfile.end()
        RT.wgrad_streams = streams
        levels = per_level(runner, records)
        runner.marks = []
        line = dict(net="dla34", batch=N, height=H, width=W, dtype=tag,
                    hip_ms=round(statistics.median(times["hip"]), 3), hip_best_ms=round(min(times["hip"]), 3),
                    torch_ms=round(statistics.median(times["torch"]), 3), torch_best_ms=round(min(times["torch"]), 3),
                    launches=len(records), launch_sum_ms=round(sum(r[2] for r in records) * 1e3, 3), levels=levels)
        kinds = {}
        for k, _, t in records:
            kinds[k] = kinds.get(k, 0.0) + t * 1e3
        line["kinds_ms"] = {k: round(v, 3) for k, v in sorted(kinds.items(), key=lambda kv: -kv[1])}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
