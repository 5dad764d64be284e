"""Time the training step of the benchmark workload (BASELINE configs[1]: 192x640, batch 12, bf16, depth + pose) with a
given optimizer name, the way bench.py times it: warm-up calls of the training hook, then a host clock around `--steps`
calls that ends in a device synchronise.  One JSON line per run; `graph_replays` says whether the timed steps were
hipGraph replays or eager launches.  Works on any commit that has bench.py (an `sgd` / `adamw` step is eager before the
fused optimizers existed).

    python tools/probes/optim_step_time.py --optimizer sgd --steps 200 --warmup 20 --repeat 3

Alternate the optimizers (and the commits) in ONE job and repeat: other people's work shares the host."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OPTIMIZERS = {"adam": dict(name="adam", lr=1e-4),
              "adamw": dict(name="adamw", lr=1e-4, weight_decay=1e-2),
              "sgd": dict(name="sgd", lr=1e-3, momentum=0.9, weight_decay=1e-4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", default="adam", choices=sorted(OPTIMIZERS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3, help="timed windows in this process")
    ap.add_argument("--tag", default="", help="copied into the output line (which commit this is)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from bench import synthetic_device_batches
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    from fsnet_amd.vision_base.utils.utils import set_random_seed
    dev = torch.device("cuda", 0)
    set_random_seed(123)
    RT.set_compute_dtype("bf16")
    B, H, W = 12, 192, 640
    model = build(**meta_arch_cfg(H, W, with_pose=True)).to(dev).train()
    optimizer = build_optimizer(model, **OPTIMIZERS[args.optimizer])
    hook = build(**training_cfg(clip_gradients=35.0).training_hook)
    batches = synthetic_device_batches(B, H, W, dev, 0)
    step = 0

    def run(n):
        nonlocal step
        for _ in range(n):
            hook(dict(batches[step % len(batches)]), model, optimizer, global_step=step)
            step += 1

    run(args.warmup)
    ms = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
    loss = float(model.head._pl.out[-1])
    assert loss == loss and abs(loss) < 1e3, "training diverged (loss=%r)" % loss
    print(json.dumps(dict(tag=args.tag, optimizer=args.optimizer, optimizer_class=type(optimizer).__name__,
                          ms_per_step=ms, steps=args.steps, graph_replays=hook.graph_replays, loss=loss)))


if __name__ == "__main__":
    main()
