"""Where the ConvNeXt runner's time goes: ConvNeXt-T, in_chans=6, 12 x 192 x 640, forward + backward, the HIP runner against
the module's own forward_torch on the same device and dtype.  Medians of five windows of ten calls, then a per-launch sum
from one profiled call (LaunchProfile).  Nothing is asserted on time: the table is what the next change to convnext.hip is
measured against.

    python tools/probes/convnext_time.py [--dtype bf16|fp32]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from fsnet_amd.engine.handover import HO  # noqa: E402
from fsnet_amd.engine.runtime import RT  # noqa: E402
from fsnet_amd.hip.conv import LaunchProfile  # noqa: E402
from fsnet_amd.vision_base.networks.models.backbone import convnext  # noqa: E402


def one_call(fwd, model, x, cots):
    for p in model.parameters():
        p.grad = None
    feats = fwd(x)
    torch.autograd.backward(feats, [c.to(f.dtype) for c, f in zip(cots, feats)])
    HO.join_companions_final()


def windows(fwd, model, x, cots, n_windows=5, calls=10):
    for _ in range(3):
        one_call(fwd, model, x, cots)
    out = []
    for _ in range(n_windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            one_call(fwd, model, x, cots)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    RT.set_compute_dtype(args.dtype)
    dt = RT.compute_dtype
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = convnext.convnext_tiny(in_chans=6).to(dev).train()
    for blk in (b for s in model.stages for b in s):
        blk.gamma.data.fill_(0.1)
    x = torch.randn(12, 6, 192, 640, device=dev)
    dims = [96, 192, 384, 768]
    cots = [torch.randn(12, c, 48 >> i, 160 >> i, device=dev) for i, c in enumerate(dims)]
    med, all_ = windows(model, model, x, cots)
    print("runner        %s  fwd+bwd median %.3f ms   windows %s" % (args.dtype, med, " ".join("%.3f" % v for v in all_)))
    ref = convnext.convnext_tiny(in_chans=6).to(dev).train()
    ref.load_state_dict(model.state_dict())
    ref = ref.to(dt)
    med_t, all_t = windows(ref.forward_torch, ref, x.to(dt), cots)
    print("forward_torch %s  fwd+bwd median %.3f ms   windows %s" % (args.dtype, med_t, " ".join("%.3f" % v for v in all_t)))
    LaunchProfile.begin()
    one_call(model, model, x, cots)
    recs = LaunchProfile.end()
    by = {}
    for kind, _, sec in recs:
        n, t = by.get(kind, (0, 0.0))
        by[kind] = (n + 1, t + sec)
    total = sum(t for _, t in by.values())
    print("per-launch sum of one profiled call: %.3f ms over %d launches" % (total * 1e3, len(recs)))
    for kind, (n, t) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print("  %-22s %4d launches  %8.3f ms  %5.1f %%" % (kind, n, t * 1e3, 100.0 * t / total))


if __name__ == "__main__":
    main()
