"""Time the deformable convolution (dcn.hip) forward and backward at the DLA upsampler's shapes for a 192 x 640 batch of
12 — 48x160x64, 24x80x128, 12x40x256, 6x20x512 (H x W x channels, 3x3 / stride 1 / padding 1, modulated, one deformable
group, Ci = Co) — against
  (a) the same arithmetic as torch gather ops on the device (the restatement of tests/helpers_dcn.py, fp32), and
  (b) the project's plain 3x3 convolution at the same shape (ConvOp forward, data gradient, weight gradient): the floor,
      a deformable convolution cannot beat it.
The dcn_* and conv_* variants time the launches alone, on operands that are already NHWC and packed.  `module_fwd_bwd` is
what a module call costs: modulated_deform_conv forward + backward on NCHW fp32 tensors, with the layout conversions and
the two weight packs of every call.
Device events around `--steps` launches after `--warmup`, `--repeat` windows, best window reported; the three variants
alternate inside every window.  One JSON line per shape and compute dtype.  Nothing is asserted.

    python tools/probes/dcn_time.py --steps 20 --warmup 5 --repeat 3

Compare within one job only: boxes differ by +-2 % (README)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = [(48, 160, 64), (24, 80, 128), (12, 40, 256), (6, 20, 512)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--no-gather", action="store_true", help="skip the torch gather variant (it is slow at 48x160)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fsnet_amd.hip import ops
    from fsnet_amd.hip.conv import ConvOp
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import modulated_deform_conv
    from tests import helpers_dcn as HD
    dev = torch.device("cuda", 0)
    N = args.batch
    for H, W, Cc in SHAPES:
        g = torch.Generator().manual_seed(H)
        x32 = torch.randn(N, Cc, H, W, generator=g).to(dev)
        off = (1.5 * torch.randn(N, 18, H, W, generator=g)).to(dev)
        mask = torch.rand(N, 9, H, W, generator=g).to(dev)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) / (3.0 * Cc ** 0.5)).to(dev)
        bias = torch.zeros(Cc, device=dev)
        dy32 = torch.randn(N, Cc, H, W, generator=g).to(dev)
        for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            geo = ops.DcnGeometry(x32.shape, w.shape, 1, 1, 1, 1, 1, dtype)
            x = ops.nchw_to_nhwc(x32, None, geo.Ci_p, dtype)
            dy = ops.nchw_to_nhwc(dy32, None, geo.Co_p, dtype)
            w_f, w_d = ops.dcn_pack(geo, w, 0), ops.dcn_pack(geo, w, 1)
            conv = ConvOp(Cc, Cc, 3, 3, 1, 1, dtype, dev)
            conv.pack(w)
            dw = torch.zeros_like(w)
            xg = x32.clone().requires_grad_()
            og, mg, wg = off.clone().requires_grad_(), mask.clone().requires_grad_(), w.clone().requires_grad_()
            bg = bias.clone().requires_grad_()

            def gather_fwd():
                return HD.dcn_ref(xg, og, mg, wg, bias, 1, 1, 1, 1)

            def gather_all():
                torch.autograd.grad(gather_fwd(), [xg, og, mg, wg], dy32)

            def module_all(tag=tag):
                RT.set_compute_dtype(tag)
                out = modulated_deform_conv(xg, og, mg, wg, bg, 1, 1, 1, 1, 1)
                torch.autograd.grad(out, [xg, og, mg, wg, bg], dy32)

            variants = {
                "module_fwd_bwd": module_all,
                "dcn_fwd": lambda: ops.dcn_forward(geo, x, off, mask, w_f, bias),
                "dcn_bwd_data": lambda: ops.dcn_backward_data(geo, x, off, mask, w_d, dy),
                "dcn_bwd_weight": lambda: ops.dcn_backward_weight(geo, x, off, mask, dy, want_bias=True),
                "conv_fwd": lambda: conv.forward(x),
                "conv_dgrad": lambda: conv.dgrad(dy, H, W),
                "conv_wgrad": lambda: conv.wgrad(dy, x, dw),
            }
            if tag == "fp32" and not args.no_gather:
                variants["gather_fwd"] = gather_fwd
                variants["gather_fwd_bwd"] = gather_all
            best = {k: float("inf") for k in variants}
            for _ in range(args.repeat):
                for k, fn in variants.items():
                    best[k] = min(best[k], timed(fn, args.steps, args.warmup))
            line = dict(shape="%dx%dx%d" % (H, W, Cc), batch=N, dtype=tag)
            line.update({k + "_us": round(v, 1) for k, v in best.items()})
            line["dcn_total_us"] = round(best["dcn_fwd"] + best["dcn_bwd_data"] + best["dcn_bwd_weight"], 1)
            line["conv_total_us"] = round(best["conv_fwd"] + best["conv_dgrad"] + best["conv_wgrad"], 1)
            line["atomic_MB"] = round(N * H * W * 9 * 4 * Cc * 4 / 1e6, 1)      # d_x adds of the data backward, upper bound
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
