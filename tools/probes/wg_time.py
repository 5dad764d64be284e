"""stand-alone time of the weight-gradient launches, one shape per kernel family (graph replay of 20 launches, HIP events):
us per launch (main kernel + reduce), median of 15 replays.  The last row is a 3x3 forward launch — code of another file,
timed the same way: what it scatters by between runs and trees is what a difference in the rows above is worth."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from fsnet_amd.hip.conv import ConvOp
dev = torch.device('cuda:0'); dt = torch.bfloat16
SHAPES = [  # family, Ci, Co, k, stride, pad, H, W, B
    ("halo", 64, 64, 3, 1, 1, 48, 160, 12), ("halo", 64, 64, 3, 1, 1, 48, 160, 24), ("halo", 128, 128, 3, 1, 1, 24, 80, 12),
    ("halo", 256, 256, 3, 1, 1, 12, 40, 12), ("halo", 512, 512, 3, 1, 1, 6, 20, 12), ("halo", 64, 64, 3, 1, 1, 80, 256, 8),
    ("stem", 3, 64, 7, 2, 3, 192, 640, 12), ("narrow", 16, 16, 3, 1, 1, 192, 640, 12),
    ("1x1 lds-dma", 256, 64, 1, 1, 0, 80, 256, 8),       # ResNet-50 layer 1 reduce at 320x1024
    ("generic tile", 512, 512, 3, 1, 1, 6, 20, 4),       # 480 pixels, wide dW: 128x128 tiles
    ("conv3x3 forward", 64, 64, 3, 1, 1, 48, 160, 12),
]


def replay_us(fn, launches=20, replays=15):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches): fn()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000 / launches)
    return sorted(ts)[len(ts) // 2]


for fam, Ci, Co, k, stride, pad, H, W, B in SHAPES:
    op = ConvOp(Ci, Co, k, k, stride, pad, dt, dev)
    Ho, Wo = op.out_hw(H, W)
    x = torch.randn(B, H, W, op.Ci_p, device=dev).to(dt)
    if fam == "conv3x3 forward":
        op.pack(torch.randn(Co, Ci, k, k, device=dev) / (Ci * k * k) ** 0.5)
        y = torch.empty(B, Ho, Wo, op.Co_p, dtype=dt, device=dev)
        us = replay_us(lambda: op.forward(x, out=y))
    else:
        gy = torch.randn(B, Ho, Wo, op.Co_p, device=dev).to(dt)
        dw = torch.zeros(Co, Ci, k, k, device=dev)
        us = replay_us(lambda: op.wgrad(gy, x, dw))
    print(f"{fam:16s} {Ci}->{Co} {k}x{k}/s{stride} @{H}x{W} B={B}: {us:.1f} us")
