"""Time the fisheye (Mei ray-table) photometric loss chain over N = 1, 2, 3, 4 source frames (fs_photo_mei_multi_*:
identity planes + forward + backward + pose gradient) at the fisheye workload's geometry — 384 x 384, batch 16, four
scales — and, in the same process on the same box, the two-source fisheye launches (fs_photo_identity_rows +
fs_photo_fused_fwd + fs_photo_fused_bwd + fs_photo_pose_grad with the ray tables).  Then the training step of
MonoDepthWPose + FishEyeDecoder for frame_ids of each length ([0, 1, -1] runs what it ran before this path existed).
Method of tools/probes/photo_multi_time.py / optim_step_time.py: warm-up calls, then a host clock around `--steps` calls
that ends in a device synchronise, `--repeat` windows, the variants alternated inside every window round; each phase also
alone with device events.  One JSON line per variant.

    python tools/probes/photo_mei_multi_time.py --steps 100 --warmup 10 --repeat 3

Compare within one job only: boxes differ by +-2 % (README)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAME_LISTS = {1: [0, -1], 2: [0, 1, -1], 3: [0, -2, -1, 1], 4: [0, -2, -1, 1, 2]}


def make_inputs(B, H, W, N, dev, seed=0):
    from fsnet_amd.vision_base.data.datasets.synthetic import synthetic_mei_calib
    g = torch.Generator().manual_seed(seed)
    ys = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xs = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.rand(B, 3, 1, 1, generator=g) * 6.28
    frames = []
    for f in range(N + 1):
        sh = 3.0 * f / W
        img = 0.5 + 0.25 * torch.sin(23.0 * (xs + sh) + ph) * torch.cos(11.0 * ys + ph) + 0.2 * torch.rand(B, 3, H, W, generator=g)
        frames.append(img.clamp(0, 1).float().to(dev).contiguous())
    Ps, calibs = zip(*[synthetic_mei_calib(H, W, b % 2) for b in range(B)])
    P2 = torch.stack([torch.as_tensor(p, dtype=torch.float32) for p in Ps], 0)
    Ts = []
    for f in range(N):
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, 0, 3], T[:, 2, 3] = (0.6 if f % 2 == 0 else -0.6) * (1 + f // 2), 0.03
        Ts.append(T.to(dev).contiguous())
    depths = [(5 + 20 * torch.rand(B, 1, H >> s, W >> s, generator=g)).to(dev).contiguous() for s in range(4)]
    disps = [(1.0 / d).contiguous() for d in depths]
    pm = torch.ones(B, H, W, dtype=torch.float64, device=dev)
    return (frames[0], frames[1:], P2.to(dev).contiguous(), Ts, pm, depths, disps), (P2, list(calibs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--model-steps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip import lib, ops
    from fsnet_amd.hip.binding import stream_ptr
    from fsnet_amd.monodepth.networks.utils.mei_fisheye_utils import MeiCameraProjection
    dev = torch.device("cuda", 0)
    RT.overlap = False                     # the smoothness kernels on the same stream: the same for every variant
    B, H, W = 16, 384, 384
    proj = MeiCameraProjection()
    variants = {}
    for name, N, multi in (("two-source", 2, False), ("multi-1", 1, True), ("multi-2", 2, True), ("multi-3", 3, True),
                           ("multi-4", 4, True)):
        inp, (P2, calibs) = make_inputs(B, H, W, N, dev)
        pl = ops.PhotometricLoss(B, H, W, [0, 1, 2, 3], dev, 0.5, 150.0, nsrc=N, force_multi=multi, want_pred=False)
        tabs, rows = proj.tables(H, W, P2, calibs, dev)
        pl.stage_fisheye(tabs, rows)
        variants[name] = (pl, inp, N)

    def chain(name):
        pl, (img0, srcs, P2, Ts, pm, depths, disps), N = variants[name]
        pl.forward(img0, srcs, P2, Ts, pm, depths, disps, noise_seed=3)
        pl.backward(None)

    def phases(name):
        """device-event times of identity / forward / backward, launched alone (us)"""
        pl, _, N = variants[name]
        chain(name)                           # fills the argument struct
        pa, st = C.byref(pl._pa), stream_ptr()
        be = pl._be
        calls = {"identity": lambda: be.identity(pa, st), "forward": lambda: be.fwd(pa, st), "backward": lambda: be.bwd(pa, st)}
        out = {"kernels": be.name}
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
    variants.clear()

    # ---- the model's training step per frame list (bf16, the benchmark's fisheye configuration)
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.vision_base.data.datasets.dataset_utils import collate_fn
    from fsnet_amd.vision_base.data.datasets.synthetic import SyntheticTripletDataset
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    from fsnet_amd.vision_base.utils.utils import set_random_seed
    RT.overlap = True
    RT.set_compute_dtype("bf16")
    steps = {}
    runs = {}
    for N, fids in FRAME_LISTS.items():
        set_random_seed(123)
        model = build(**meta_arch_cfg(H, W, with_pose=False, depth=18, num_output_channels=64, max_depth=150.0,
                                      fisheye=True, frame_ids=fids)).to(dev).train()
        tc = training_cfg(clip_gradients=35.0, lr=1e-4, weight_decay=1e-5)
        opt = build_optimizer(model, **tc.optimizer)
        hook = build(**tc.training_hook)
        ds = SyntheticTripletDataset(size=4 * B, height=H, width=W, seed=1000, fisheye=True, frame_idxs=tuple(fids))
        batches = []
        for i in range(4):
            d = collate_fn([ds[i * B + j] for j in range(B)])
            batches.append({k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()})
        runs[N] = (hook, model, opt, batches)
        for i in range(args.warmup):
            hook(dict(batches[i % 4]), model, opt, global_step=i)
        torch.cuda.synchronize()
        steps[N] = []
    for _ in range(args.repeat):
        for N, (hook, model, opt, batches) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.model_steps):
                hook(dict(batches[i % 4]), model, opt, global_step=args.warmup + i)
            torch.cuda.synchronize()
            steps[N].append((time.perf_counter() - t0) * 1000.0 / args.model_steps)
    for N in runs:
        print(json.dumps(dict(variant="model-step", frame_ids=FRAME_LISTS[N], step_ms=[round(v, 3) for v in steps[N]],
                              best_ms=round(min(steps[N]), 3), ratio_to_two_source=round(min(steps[N]) / min(steps[2]), 3),
                              graph_replays=int(getattr(runs[N][0], "graph_replays", 0)))), flush=True)


if __name__ == "__main__":
    main()
