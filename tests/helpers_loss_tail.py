"""Plain torch / numpy restatements of the loss tail — the edge-aware smoothness loss and its gradient, the loss
assembly (loss_finalize), the gradient square sum (sumsq), the depth-bin head and the pose tail — with the inputs and
the host arithmetic the GPU cases of tests/test_loss_tail_gpu.py are built from.  No GPU here:
tests/test_loss_tail_restatement_cpu.py holds the restatements against the oracle and asserts which branch each case
reaches.

Every restatement takes a dtype: torch.float64 is the reference, torch.float32 the yardstick (the same formula in
torch's float32 on the CPU; how far it strays from float64 is the unit the kernels' deviation is measured in, see
`bound`)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fsnet_oracle as O

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------- tolerances
def yardstick(ref64, ref32):
    """largest absolute deviation of the float32 restatement from the float64 one"""
    return float((ref32.double() - ref64).abs().max())


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def bound(ref64, ref32):
    """what a float32 kernel may deviate from float64: 8 x yardstick + 4 float32 ulps of the largest reference
    magnitude.  8, because the kernels' expf, their reciprocal rounded once to float and their summation order are not
    torch's; nothing here is taken from what a kernel returns."""
    return 8.0 * yardstick(ref64, ref32) + 4.0 * ulp32(ref64.abs().max())


# ---------------------------------------------------------------------------------------------- smoothness
def smooth_terms(disps, colors, scale_ids, gout, dtype=F64):
    """per scale: disp_sum[b], (sx_sum[b], sy_sum[b]) as the kernel accumulates them before the means, the loss
    `smooth_loss/s` and d_disp by autograd.  The formula is the oracle's (photometric_loss): nd = disp / (mean_hw(disp)
    + 1e-7), smooth_loss(nd, color) * 1e-5 / 2**scale_id, gradient weight gout / S."""
    S = len(disps)
    g = 1.0 if gout is None else float(gout)
    out = []
    for d, c, sid in zip(disps, colors, scale_ids):
        d = d.detach().to(dtype).clone().requires_grad_(True)
        c = c.detach().to(dtype)
        B, _, h, w = d.shape
        nd = d / (d.mean(2, True).mean(3, True) + 1e-7)
        ex = torch.exp(-(c[..., :-1] - c[..., 1:]).abs().mean(1, True))
        ey = torch.exp(-(c[:, :, :-1] - c[:, :, 1:]).abs().mean(1, True))
        sx = ((nd[..., :-1] - nd[..., 1:]).abs() * ex).sum((1, 2, 3))
        sy = ((nd[:, :, :-1] - nd[:, :, 1:]).abs() * ey).sum((1, 2, 3))
        loss = (sx.sum() / (B * h * (w - 1)) + sy.sum() / (B * (h - 1) * w)) * 1e-5 / (2 ** sid)
        (loss * g / S).backward()
        out.append({"disp_sum": d.detach().sum((1, 2, 3)), "sx_sum": sx.detach(), "sy_sum": sy.detach(),
                    "loss": loss.detach(), "d_disp": d.grad})
    return out


def neighbour_gaps(disp):
    """float64 |nd_i - nd_j| over all horizontal and vertical neighbour pairs of disp [B,1,h,w], per batch element"""
    d = disp.double()
    nd = d / (d.mean(2, True).mean(3, True) + 1e-7)
    gx = (nd[..., :-1] - nd[..., 1:]).abs().flatten(1)
    gy = (nd[:, :, :-1] - nd[:, :, 1:]).abs().flatten(1)
    return torch.cat([gx, gy], 1)


def smooth_grid(hw):
    """smooth_grid of csrc/smooth_optim.hip: blocks per (scale, batch element), shared by all scales.  Returns (blocks,
    per scale: (rounds of the grid-stride loop, pixels in the last round, blocks that hold no pixel at all))"""
    big = max(h * w for h, w in hw)
    blocks = min((big + 255) // 256, 32)
    per = blocks * 256
    info = []
    for h, w in hw:
        n = h * w
        rounds = (n + per - 1) // per
        info.append((rounds, n - (rounds - 1) * per, max(0, blocks - (n + 255) // 256)))
    return blocks, info


# (name, B, [(h, w)], scale_id, seed) — the cases of the direct smoothness test
SMOOTH_CASES = [
    ("a", 1, [(2, 2)], [0], 0),
    ("b", 2, [(3, 5)], [0], 5),
    ("c", 2, [(37, 53), (18, 26), (9, 13)], [0, 1, 2], 2),
    ("d", 3, [(96, 100), (2, 300)], [1, 3], 3),
]


def grid_disp(g, B, h, w, const_b):
    """disparities on the grid k/64 * 0.9 + 0.01, k in 1..64: about a quarter of the pixels copy their left
    neighbour, a tenth their upper one, so neighbouring normalised disparities are exactly equal (sign 0 in the kernel,
    gradient 0 in torch.abs) or at least a grid step apart (no sign can differ between float32 and float64).
    const_b: that batch element is constant (None: no such element)."""
    k = torch.randint(1, 65, (B, 1, h, w), generator=g)
    left = torch.rand(B, 1, h, w - 1, generator=g) < 0.25
    k[..., 1:] = torch.where(left, k[..., :-1].clone(), k[..., 1:])
    up = torch.rand(B, 1, h - 1, w, generator=g) < 0.10
    k[:, :, 1:] = torch.where(up, k[:, :, :-1].clone(), k[:, :, 1:])
    if const_b is not None:
        k[const_b] = 17
    return (k.double() / 64 * 0.9 + 0.01).float()


def mixed_color(g, B, h, w):
    """flat 4x4 regions, noise on about a third of the pixels, and pixels forced to 0 or 1 in all channels: the edge
    weight exp(-mean|dc|) spans e^-1 .. 1"""
    c = torch.rand(B, 3, (h + 3) // 4, (w + 3) // 4, generator=g)
    c = c.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :h, :w].clone()
    noisy = (torch.rand(B, 1, h, w, generator=g) < 0.3).float()
    c = (c + noisy * 0.1 * torch.rand(B, 3, h, w, generator=g)).clamp(0, 1)
    step = torch.rand(B, 1, h, w, generator=g) < 0.15
    level = (torch.rand(B, 1, h, w, generator=g) < 0.5).float()
    return torch.where(step, level.expand(B, 3, h, w), c).float().contiguous()


def smooth_case(name):
    """-> (B, hw, scale_ids, disps, colors, const_b).  Case a is written out: a 2x2 image has four neighbour pairs, one of
    them equal.  B = 1 cannot hold a constant element beside a varying one, so case a has none."""
    _, B, hw, sids, seed = next(c for c in SMOOTH_CASES if c[0] == name)
    g = torch.Generator().manual_seed(100 + seed)
    const_b = B - 1 if B > 1 else None
    if name == "a":
        k = torch.tensor([[5.0, 5.0], [40.0, 23.0]], dtype=F64).view(1, 1, 2, 2)
        disps = [(k / 64 * 0.9 + 0.01).float()]
    else:
        disps = [grid_disp(g, B, h, w, const_b) for h, w in hw]
    colors = [mixed_color(g, B, h, w) for h, w in hw]
    return B, hw, sids, disps, colors, const_b


def chain_batch():
    """the B=2, 32x64 oracle batch of test_photometric_chain_vs_oracle_no_mask with grid disparities at the four scales
    (element 1 constant), the depths that belong to them, and the float64 colour pyramid"""
    B, H, W = 2, 32, 64
    data = O.synthetic_batch(B, H, W, seed=8)
    g = torch.Generator().manual_seed(4)
    disps = [grid_disp(g, B, H >> s, W >> s, 1) for s in range(4)]
    depths = [(1.0 / (1.0 / 100.0 + (1.0 / 0.5 - 1.0 / 100.0) * d.double())).float() for d in disps]
    return data, depths, disps


def color_pyramid(img, hw, dtype=F64):
    return [img.to(dtype) if (h, w) == tuple(img.shape[2:]) else F.adaptive_avg_pool2d(img.to(dtype), (h, w))
            for h, w in hw]


# ---------------------------------------------------------------------------------------------- loss_finalize
FINALIZE_CASES = [          # (B, hw per scale, scale_id)
    (1, [(4, 6)], [2]),
    (3, [(32, 64), (16, 32), (8, 16), (4, 8)], [0, 1, 2, 3]),
    (64, [(16, 32), (8, 16), (4, 8), (2, 4)], [0, 1, 2, 3]),
    (65, [(12, 20), (6, 10), (3, 5)], [0, 2, 3]),
    (130, [(10, 14), (5, 7)], [1, 3]),
]


def finalize_sums(B, hw, seed):
    """positive float64 sums of the size the step produces: per-element photometric sums, mask sums, smoothness sums"""
    rng = np.random.default_rng(seed)
    S = len(hw)
    loss_sums = rng.uniform(0.05, 0.2, (S, B)) * hw[0][0] * hw[0][1]
    mask_sum = rng.uniform(0.5, 1.0, B) * hw[0][0] * hw[0][1]
    sm_sums = np.stack([rng.uniform(0.1, 0.9, (B, 2)) * h * w for h, w in hw])
    return loss_sums, mask_sum, sm_sums


def finalize(loss_sums, mask_sum, sm_sums, B, hs, ws, scale_ids):
    """loss_finalize_kernel with its casts: sx, sy and sm are float32, everything else float64.
    loss_sums [S,B], mask_sum [B], sm_sums [S,B,2] -> out [2S+1] float64 (loss/s, smooth_loss/s, total)"""
    S = len(hs)
    out = np.zeros(2 * S + 1)
    msum = float(np.sum(mask_sum))
    total = 0.0
    for s in range(S):
        h, w = hs[s], ws[s]
        ax, ay, ls = float(sm_sums[s, :, 0].sum()), float(sm_sums[s, :, 1].sum()), float(loss_sums[s].sum())
        sx = np.float32(ax / float(B * h * (w - 1)))
        sy = np.float32(ay / float(B * (h - 1) * w))
        sm = np.float32(np.float32(np.float32(sx + sy) * np.float32(1e-5)) / np.float32(1 << scale_ids[s]))
        l = ls / (msum + 1e-6) + float(sm)
        out[s], out[S + s] = l, float(sm)
        total += l
    out[2 * S] = total / S
    return out


# ---------------------------------------------------------------------------------------------- sumsq
SUMSQ_NS = [1, 3, 4, 5, 1023, 4101, 524292, 2 * 524288 + 5, 3 * 524288 + 1027]


def sumsq_walk(n):
    """fs_sumsq's host grid and, thread by thread, which loop of sumsq_kernel takes each element: the loop with two
    16-byte loads in flight, the single-load loop, the scalar tail"""
    blocks = min((n // 4 + 255) // 256 + 1, 512)
    stride = blocks * 1024
    i = np.arange(blocks * 256, dtype=np.int64) * 4
    it2 = np.maximum(0, -((-(n - 3 - stride - i)) // (2 * stride)))        # i + 3 + stride < n, step 2 * stride
    i = i + it2 * 2 * stride
    it1 = np.maximum(0, -((-(n - 3 - i)) // stride))                       # i + 3 < n, step stride
    i = i + it1 * stride
    tail = np.where(i < n, np.minimum(n, i + 4) - i, 0)
    return {"blocks": blocks, "threads": blocks * 256, "two": int(8 * it2.sum()), "one": int(4 * it1.sum()),
            "tail": int(tail.sum()), "threads_two": int((it2 > 0).sum()), "threads_one": int((it1 > 0).sum()),
            "threads_tail": int((tail > 0).sum())}


# ---------------------------------------------------------------------------------------------- depth-bin head
HEAD_KS = [16, 32, 64]
HEAD_SINGLE = (2, 5, 7)
HEAD_MULTI = [(3, 5, 7), (3, 3, 4), (3, 2, 2)]
HEAD_FX = (0.7, 1.0, 1.9)          # x base_fx, one per image
HEAD_BASE_FX = 37.0
MIN_D, MAX_D = 0.5, 100.0


def head_blocks(Ms):
    """grid_for / head_blocks of csrc/heads.hip: first block of every scale, and the total"""
    start, total = [], 0
    for M in Ms:
        start.append(total)
        total += max(1, min((M + 255) // 256, 8192))
    return start + [total]


def head_logits(g, M, K, Cl):
    """[M, Cl] float32.  Rows 0..3 are written out: entries exactly at +-10 (the clamp passes the gradient there) next to
    entries beyond it, an all-equal row, a one-hot-dominant row; the rest is 6 * randn with a few more +-10 / beyond.
    Channels >= K are 1000 + noise: nothing may read them."""
    x = torch.randn(M, Cl, generator=g) * 6
    edge = torch.tensor([10.0, -10.0, 10.5, -10.5, 30.0, -30.0, 9.5, -9.5])
    x[0, :K] = edge.repeat(K // 8)
    if M > 1:
        x[1, :K] = 2.5
    if M > 2:
        x[2, :K] = -8.0
        x[2, K // 3] = 9.0
    if M > 3:
        x[3, :K] = torch.randn(K, generator=g)
        x[3, 0], x[3, K - 1] = 10.0, -10.0
    pick = torch.rand(M, Cl, generator=g) < 0.04
    pick[:4] = False
    x = torch.where(pick, edge[torch.randint(0, 6, (M, Cl), generator=g)], x)
    x[:, K:] = 1000.0 + x[:, K:]
    return x.float().contiguous()


def head(logits, bins, sc, min_d, max_d, d_depth=None, d_disp=None, dtype=F64):
    """logits [M, K], bins [K], sc [M] (the focal scale P2[b,0,0] / base_fx of the row's image) or None ->
    depth [M], disp [M], dlogits [M, K] by autograd from d_depth / d_disp (None: no such term; both None: zeros)"""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    p = torch.softmax(torch.clamp(x, -10.0, 10.0), dim=1)
    d = (p * bins.to(dtype).view(1, -1)).sum(1)
    if sc is None:
        depth = d
        disp = (1 / depth - 1 / max_d) / (1 / min_d - 1 / max_d)
    else:
        sc = sc.to(dtype)
        depth = d * sc
        disp = (1 / depth - 1 / (max_d * sc)) / (1 / (min_d * sc) - 1 / (max_d * sc))
    obj = x.sum() * 0
    if d_depth is not None:
        obj = obj + (depth * d_depth.to(dtype)).sum()
    if d_disp is not None:
        obj = obj + (disp * d_disp.to(dtype)).sum()
    obj.backward()
    return depth.detach(), disp.detach(), x.grad


def head_scale(P2, base_fx, rows_img, dtype=F64):
    """per-row focal scale as the kernel indexes it: image m // rows_img, P2[b, 0, 0] / base_fx"""
    return (P2[:, 0, 0].to(dtype) / torch.tensor(base_fx, dtype=F32).to(dtype)).repeat_interleave(rows_img)


def head_P2(nimg):
    P2 = torch.zeros(nimg, 3, 4)
    P2[:, 0, 0] = torch.tensor([f * HEAD_BASE_FX for f in HEAD_FX[:nimg]])
    P2[:, 1, 1], P2[:, 0, 2], P2[:, 1, 2], P2[:, 2, 2] = 50.0, 20.0, 10.0, 1.0
    return P2.float().contiguous()


# ---------------------------------------------------------------------------------------------- pose tail
POSE_HW = [1, 63, 64, 65, 120]


def pose_features(g, B, hw, Cx):
    """[B, hw, Cx] float32, scaled as test_pose_tail scales them (3 * randn): means of a few tenths, angles of a few
    1e-3 after the 0.01.  Never a zero rotation: channel 0's mean is pushed away from 0."""
    x = torch.randn(B, hw, Cx, generator=g) * 3
    x[:, :, 0] += 0.5
    return x.float().contiguous()


def pose_tail(x, nframes, invert, scale, dT=None, dtype=F64):
    """x [B, hw, Cx] -> axisangle [B,nframes,1,3], translation [B,nframes,1,3], T [B,4,4] of frame 0
    (O.transformation_from_parameters) and, with dT, dx [B, hw, Cx] by autograd of sum(T * dT)"""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    B = x.shape[0]
    m = x[:, :, :6 * nframes].mean(1)
    o = scale * m.view(B, nframes, 1, 6)
    aa, tr = o[..., :3], o[..., 3:]
    T = O.transformation_from_parameters(aa[:, 0], tr[:, 0], invert=invert)
    dx = None
    if dT is not None:
        (T * dT.to(dtype)).sum().backward()
        dx = x.grad
    return aa.detach(), tr.detach(), T.detach(), dx
