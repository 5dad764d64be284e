"""Time the photometric loss chain over N = 1, 2, 3, 4 source frames (photo_multi.hip: identity planes + forward +
backward + pose gradient) at the benchmark's geometry — 192 x 640, batch 12, four scales — and, in the same process on
the same box, the existing two-source launches (fs_photo_identity_rows + fs_photo_fused_fwd + fs_photo_fused_bwd +
fs_photo_pose_grad).  Method of tools/probes/optim_step_time.py: warm-up calls, then a host clock around `--steps`
calls that ends in a device synchronise, `--repeat` windows, the variants alternated inside every window round.  Each
phase is also timed alone with device events.  One JSON line per variant.

    python tools/probes/photo_multi_time.py --steps 200 --warmup 20 --repeat 3

Compare within one job only: boxes differ by +-2 % (README)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_inputs(B, H, W, N, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    ys = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xs = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.rand(B, 3, 1, 1, generator=g) * 6.28
    frames = []
    for f in range(N + 1):
        sh = 3.0 * f / W
        img = 0.5 + 0.25 * torch.sin(23.0 * (xs + sh) + ph) * torch.cos(11.0 * ys + ph) + 0.2 * torch.rand(B, 3, H, W, generator=g)
        frames.append(img.clamp(0, 1).float().to(dev).contiguous())
    P2 = torch.zeros(B, 3, 4)
    P2[:, 0, 0], P2[:, 0, 2], P2[:, 1, 1], P2[:, 1, 2], P2[:, 2, 2] = 0.58 * W, 0.5 * W, 1.92 * H, 0.5 * H, 1
    Ts = []
    for f in range(N):
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, 0, 3], T[:, 2, 3] = 0.01 * (f + 1), (-0.8 if f % 2 == 0 else 0.8)
        Ts.append(T.to(dev).contiguous())
    depths = [(4 + 25 * torch.rand(B, 1, H >> s, W >> s, generator=g)).to(dev).contiguous() for s in range(4)]
    disps = [(1.0 / d).contiguous() for d in depths]
    pm = torch.ones(B, H, W, dtype=torch.float64, device=dev)
    return frames[0], frames[1:], P2.to(dev).contiguous(), Ts, pm, depths, disps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fsnet_amd.hip import ops
    from fsnet_amd.engine.runtime import RT
    dev = torch.device("cuda", 0)
    RT.overlap = False                     # the smoothness kernels on the same stream: the same for every variant
    B, H, W = 12, 192, 640
    variants = {}
    for name, N, multi in (("two-source", 2, False), ("multi-1", 1, True), ("multi-2", 2, True), ("multi-3", 3, True),
                           ("multi-4", 4, True)):
        inp = make_inputs(B, H, W, N, dev)
        if multi:
            pl = ops.PhotometricLoss(B, H, W, [0, 1, 2, 3], dev, 0.5, 100.0, nsrc=N, force_multi=True, want_pred=False)
        else:
            pl = ops.PhotometricLoss(B, H, W, [0, 1, 2, 3], dev, 0.5, 100.0, want_pred=False)
        variants[name] = (pl, inp, N)

    def chain(name):
        pl, (img0, srcs, P2, Ts, pm, depths, disps), N = variants[name]
        pl.forward(img0, srcs, P2, Ts, pm, depths, disps, noise_seed=3)
        pl.backward(None)

    def phases(name):
        """device-event times of identity / forward / backward+pose-grad, launched alone (ms)"""
        import ctypes as C
        from fsnet_amd.hip import lib
        from fsnet_amd.hip.binding import stream_ptr
        pl, _, N = variants[name]
        chain(name)                           # fills the argument struct
        pa, st = C.byref(pl._pa), stream_ptr()
        multi = pl.multi
        calls = {
            "identity": (lambda: lib.fs_photo_multi_identity(pa, st)) if multi else (lambda: lib.fs_photo_identity_rows(pa, st)),
            "forward": (lambda: lib.fs_photo_multi_fwd(pa, st)) if multi else (lambda: lib.fs_photo_fused_fwd(pa, st)),
            "backward": (lambda: lib.fs_photo_multi_bwd(pa, st)) if multi else (lambda: lib.fs_photo_fused_bwd(pa, st)),
        }
        out = {}
        for k, fn in calls.items():
            for _ in range(5):
                assert fn() == 0
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(50):
                fn()
            e.record()
            torch.cuda.synchronize()
            out[k + "_us"] = round(s.elapsed_time(e) * 1000.0 / 50, 1)
        return out

    for name in variants:
        for _ in range(args.warmup):
            chain(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.repeat):
        for name in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                chain(name)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1000.0 / args.steps)
    base = min(ms["two-source"])
    for name in variants:
        line = dict(variant=name, nsrc=variants[name][2], chain_ms=[round(v, 4) for v in ms[name]],
                    best_ms=round(min(ms[name]), 4), ratio_to_two_source=round(min(ms[name]) / base, 3))
        line.update(phases(name))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
