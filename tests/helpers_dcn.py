"""The yardstick of the deformable-convolution tests: a plain-torch restatement of the sampling rule, differentiable by
autograd, in any floating dtype — plus the seeded cases the CPU and GPU tests share.

The reference's extension (vision_base/networks/ops/dcn/src/cuda/deform_conv_cuda_kernel.cu) is CUDA only and cannot
run here, so this restatement is held against that text BY READING, not by execution:
  * sample position h = ho * stride_h - pad_h + r * dil_h + offset, offset channel 2 (rS + s) for h and 2 (rS + s) + 1 for
    w inside deformable group g, mask channel rS + s                      (:211-228 v1, :600-616 v2)
  * the value is 0 unless h > -1 and w > -1 and h < H and w < W            (:229, :618)
  * bilinear around floor(h), floor(w); a corner contributes only when it lies inside [0, H-1] x [0, W-1]   (:89-113)
  * v2 multiplies the sampled value by the mask                            (:627)
  * the column GEMM with the OIHW weight flattened over (ci, r, s), plus the bias in v2
Autograd of this expression is what the col2im kernels (:280-333 and :636-693 with the corner weights of :118-143) and
the col2im_coord kernels (:374-436 and :696-767 with the coordinate weights of :146-188, the mask gradient at :764-765)
compute: floor() has a zero derivative, so d/dh reaches only the blend weights, and a sample outside the open range has
no gradient at all (:423, :747).
"""
import functools

import torch


def bf16_round(t):
    """the GEMM-operand hook of the bf16 yardstick: the value rounded to bf16, the gradient passed through"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, hook):
        ctx.hook = hook
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.hook(g).detach(), None


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_hw(H, W, R, S, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    return (H + 2 * ph - (dh * (R - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (S - 1) + 1)) // sw + 1


def sample_coords(offset, H, W, R, S, stride, padding, dilation, dg):
    """h, w [N][dg][R*S][Ho][Wo] in offset's dtype"""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    N, _, Ho, Wo = offset.shape
    dt = offset.dtype
    off = offset.reshape(N, dg, R * S, 2, Ho, Wo)
    dev = offset.device
    r = torch.arange(R * S, device=dev) // S
    s = torch.arange(R * S, device=dev) % S
    bh = (torch.arange(Ho, device=dev)[None, :, None] * sh - ph + (r * dh)[:, None, None]).to(dt)       # [RS][Ho][1]
    bw = (torch.arange(Wo, device=dev)[None, None, :] * sw - pw + (s * dw)[:, None, None]).to(dt)       # [RS][1][Wo]
    return bh + off[:, :, :, 0], bw + off[:, :, :, 1]


def dcn_columns(x, offset, mask, R, S, stride, padding, dilation, dg):
    """col [N][Ci][R*S][Ho][Wo]"""
    N, Ci, H, W = x.shape
    Ho, Wo = offset.shape[2:]
    h, w = sample_coords(offset, H, W, R, S, stride, padding, dilation, dg)
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    hli, wli = hl.long(), wl.long()
    cpg = Ci // dg
    xg = x.reshape(N, dg, cpg, H * W)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    col = 0
    for hi, wi, wt in ((hli, wli, hh * hw), (hli, wli + 1, hh * lw), (hli + 1, wli, lh * hw), (hli + 1, wli + 1, lh * lw)):
        ok = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)).reshape(N, dg, 1, -1).expand(N, dg, cpg, -1)
        v = torch.gather(xg, 3, idx).reshape(N, dg, cpg, R * S, Ho, Wo)
        col = col + torch.where(ok, wt, zero)[:, :, None] * v
    if mask is not None:
        col = col * mask.reshape(N, dg, 1, R * S, Ho, Wo)
    return col.reshape(N, Ci, R * S, Ho, Wo)


def dcn_ref(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, dg=1, hook=None):
    """out [N][Co][Ho][Wo]; hook (e.g. bf16_round) rounds the GEMM operands: columns, weights and, in backward, dY"""
    Co, Ci, R, S = weight.shape
    col = dcn_columns(x, offset, mask, R, S, stride, padding, dilation, dg)
    wk = weight.reshape(Co, Ci, R * S)
    if hook is not None:
        col, wk = hook(col), hook(wk)
    out = torch.einsum("nckhw,ock->nohw", col, wk)
    if bias is not None:
        out = out + bias[None, :, None, None]
    if hook is not None:
        out = _RoundGrad.apply(out, hook)      # dY is rounded once, for every gradient (d_bias included)
    return out


QUANTITIES = ("out", "d_x", "d_offset", "d_mask", "dW", "d_bias")


def run_ref(case, dtype, hook=None):
    """forward and backward of the restatement on the CPU -> {quantity: tensor in `dtype`}"""
    t = {k: (v.detach().to(dtype).requires_grad_(k != "dy") if torch.is_tensor(v) else v) for k, v in case.items()}
    out = dcn_ref(t["x"], t["offset"], t["mask"], t["weight"], t["bias"], t["stride"], t["padding"], t["dilation"],
                  t["dg"], hook)
    leaves = [t[k] for k in ("x", "offset", "mask", "weight", "bias") if t[k] is not None]
    grads = iter(torch.autograd.grad(out, leaves, t["dy"]))
    res = {"out": out.detach(), "d_x": next(grads), "d_offset": next(grads)}
    res["d_mask"] = next(grads) if t["mask"] is not None else None
    res["dW"] = next(grads)
    res["d_bias"] = next(grads) if t["bias"] is not None else None
    return res


# ------------------------------------------------------------------------------------------------------------ cases
def _coords(gen, n, size):
    """n sample coordinates along an axis of `size` cells in three classes: 0 fully inside (both neighbours are cells),
    1 inside the open range (-1, size) with one neighbour outside, 2 outside.  Fractions in [0.05, 0.95]: never within
    1e-3 of an integer."""
    frac = 0.05 + 0.9 * torch.rand(n, generator=gen, dtype=torch.float64)
    u = torch.rand(n, generator=gen, dtype=torch.float64)
    pick = torch.rand(n, generator=gen, dtype=torch.float64)
    full = torch.floor(u * max(size - 1, 1)).clamp(max=max(size - 2, 0))
    edge = torch.where(u < 0.5, torch.full_like(u, -1.0), torch.full_like(u, float(size - 1)))
    outer = torch.tensor([-3.0, -2.0, float(size), float(size + 1)], dtype=torch.float64)[(u * 4).long().clamp(max=3)]
    anyin = torch.floor(pick * (size + 1)) - 1          # any cell of the open range: -1 .. size - 1
    return {"full": full + frac, "edge": edge + frac, "outer": outer + frac, "anyin": anyin + frac}


def make_case(seed, N, Ci, H, W, Co, R, S, stride=1, padding=0, dilation=1, dg=1, v2=True, bias=True):
    """seeded inputs whose samples are ~12 % wholly outside, ~15 % partly outside and the rest fully inside"""
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, R, S, stride, padding, dilation)
    assert Ho >= 1 and Wo >= 1 and H >= 2 and W >= 2
    n = N * dg * R * S * Ho * Wo
    ch, cw = _coords(gen, n, H), _coords(gen, n, W)
    cls = torch.rand(n, generator=gen, dtype=torch.float64)
    axis = torch.rand(n, generator=gen, dtype=torch.float64) < 0.5
    h = torch.where(cls < 0.12, torch.where(axis, ch["outer"], ch["anyin"]),
                    torch.where(cls < 0.27, torch.where(axis, ch["edge"], ch["anyin"]), ch["full"]))
    w = torch.where(cls < 0.12, torch.where(axis, cw["anyin"], cw["outer"]),
                    torch.where(cls < 0.27, torch.where(axis, cw["anyin"], cw["edge"]), cw["full"]))
    zero = torch.zeros(N, dg * 2 * R * S, Ho, Wo, dtype=torch.float64)
    bh, bw = sample_coords(zero, H, W, R, S, stride, padding, dilation, dg)
    off = torch.stack([h.reshape(bh.shape) - bh, w.reshape(bw.shape) - bw], dim=3)     # [N][dg][RS][2][Ho][Wo]
    fan = Ci * R * S
    case = {
        "x": torch.randn(N, Ci, H, W, generator=gen, dtype=torch.float64).float(),
        "offset": off.reshape(N, dg * 2 * R * S, Ho, Wo).float(),
        "mask": (0.1 + 0.8 * torch.rand(N, dg * R * S, Ho, Wo, generator=gen, dtype=torch.float64)).float() if v2 else None,
        "weight": ((torch.rand(Co, Ci, R, S, generator=gen, dtype=torch.float64) * 2 - 1) / fan ** 0.5).float(),
        "bias": torch.randn(Co, generator=gen, dtype=torch.float64).float() if bias else None,
        "dy": torch.randn(N, Co, Ho, Wo, generator=gen, dtype=torch.float64).float(),
        "stride": stride, "padding": padding, "dilation": dilation, "dg": dg,
    }
    return case


def sample_statistics(case):
    """fractions of the case's samples (in f64, from the fp32 offsets): outside, partial, full; the smallest distance of
    a coordinate from an integer; the mask's range"""
    Co, Ci, R, S = case["weight"].shape
    H, W = case["x"].shape[2:]
    h, w = sample_coords(case["offset"].double(), H, W, R, S, case["stride"], case["padding"], case["dilation"], case["dg"])
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    full = (h >= 0) & (h < H - 1) & (w >= 0) & (w < W - 1)
    n = float(h.numel())
    dist = torch.minimum((h - torch.round(h)).abs().min(), (w - torch.round(w)).abs().min())
    m = case["mask"]
    return {"outside": float((~inside).sum()) / n, "partial": float((inside & ~full).sum()) / n,
            "full": float(full.sum()) / n, "min_int_dist": float(dist),
            "mask_min": float(m.min()) if m is not None else 0.5, "mask_max": float(m.max()) if m is not None else 0.5}


def _case(name, **kw):
    return name, kw


def gpu_cases(P=64, C=256):
    """The seam shapes of the GPU tests, from the kernels' pixel tile P and the forward's channel tile C (fs_dcn_tile(0)):
    M in {1, P-1, P, P+1, 2P+3} output pixels; Ci, Co in {16, 24, 64, 72, 128} and the padded 3 -> 5; stride 1 / 2,
    padding 0 / 1 / 2, dilation 1 / 2, 3x3 and 1x1, deformable_groups 1 / 2, v1 / v2, with and without bias; and the
    forward's channel tile: a forward block owns C output channels only where at least 256 blocks run without
    splitting them (C / 2 or C / 4 = 64 otherwise; every case above runs at 64), so three 1x1 cases with 128 P and 256 P
    pixels and Co = C / 2 + 8 and C + 8 reach C / 2 and C channels per block with a part-filled last 64-channel tile and,
    at Co = C + 8, a second block along the channels.  -> {name: make_case keywords}"""
    assert P == 64, "the pixel shapes below are written for a 64-pixel tile: re-derive them from fs_dcn_tile"
    cases = [
        # M = 1: 3x3 input, 3x3 kernel, no padding
        _case("m1_c16_k3", seed=1, N=1, Ci=16, H=3, W=3, Co=16, R=3, S=3, padding=0),
        # M = P - 1 = 63 = 7 x 9
        _case("m63_c24_k3_p1", seed=2, N=1, Ci=24, H=7, W=9, Co=24, R=3, S=3, padding=1),
        # M = P = 64 = 8 x 8, from 15 x 15 at stride 2 with dilation 2 and padding 2: (15 + 4 - 5) / 2 + 1 = 8
        _case("m64_c64_k3_s2_d2", seed=3, N=1, Ci=64, H=15, W=15, Co=64, R=3, S=3, stride=2, padding=2, dilation=2),
        # M = P + 1 = 65 = 5 x 13
        _case("m65_c72_k3_v1", seed=4, N=1, Ci=72, H=5, W=13, Co=72, R=3, S=3, padding=1, v2=False, bias=False),
        # M = 2P + 3 = 131 = 131 x 1 (13 x 29 and 33 x 20 below exceed it: several blocks, N = 3)
        _case("m131_c128_k1", seed=5, N=1, Ci=128, H=131, W=2, Co=128, R=1, S=1, stride=(1, 2), padding=0),
        _case("n3_13x29_c64_c16_dg2", seed=6, N=3, Ci=64, H=13, W=29, Co=16, R=3, S=3, padding=1, dg=2),
        _case("n3_33x20_c16_c128_s2", seed=7, N=3, Ci=16, H=33, W=20, Co=128, R=3, S=3, stride=2, padding=1, bias=False),
        _case("5x7_c3_c5_padded", seed=8, N=1, Ci=3, H=5, W=7, Co=5, R=3, S=3, padding=1),
        _case("5x7_c128_c72_d2_p2_v1_dg2", seed=9, N=3, Ci=128, H=5, W=7, Co=72, R=3, S=3, padding=2, dilation=2, dg=2,
              v2=False, bias=False),
        _case("13x29_c24_c64_k1_s2", seed=10, N=1, Ci=24, H=13, W=29, Co=64, R=1, S=1, stride=2, padding=0),
        # the forward's channel tile (1x1 keeps the restatement cheap): 128 P pixels x (C / 2 + 8) channels -> C / 2 per
        # block, two tiles then one; 256 P pixels x (C / 2 + 8) -> C per block, three tiles; 256 P x (C + 8) -> C per block,
        # four tiles, and a second block with one
        _case("co_half_tile", seed=11, N=1, Ci=16, H=2 * P, W=P, Co=C // 2 + 8, R=1, S=1),
        _case("co_full_tile_part", seed=12, N=1, Ci=16, H=2 * P, W=2 * P, Co=C // 2 + 8, R=1, S=1),
        _case("co_full_tile_two_blocks", seed=13, N=1, Ci=16, H=2 * P, W=2 * P, Co=C + 8, R=1, S=1),
    ]
    return dict(cases)


@functools.lru_cache(maxsize=None)
def case_and_refs(name):
    """(case, f64 reference, fp32 CPU run, bf16-hook run): computed once per process and shared; do not modify"""
    case = make_case(**gpu_cases()[name])
    return case, run_ref(case, torch.float64), run_ref(case, torch.float32), run_ref(case, torch.float64, bf16_round)


def deviation(a, ref):
    """(max abs, rms) of a - ref in f64"""
    d = a.double() - ref.double()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------- the DLA upsampler fixture (dla_up.npz)
DLA_UP = dict(input_channels=[16, 32, 64, 128, 256, 512], down_ratio=4, last_level=5)
DLA_UP_MIN_OFFSET = 0.3          # mean |offset| in pixels every DCN layer must reach: below it the fixture tests a plain conv


def dla_up_inputs(N=2, base=64, seed=71):
    """(seeded pyramid from a base x base image: level i is [N][C_i][base / 2^i][base / 2^i], the output's cotangent)"""
    gen = torch.Generator().manual_seed(seed)
    chans = DLA_UP["input_channels"]
    pyramid = [torch.randn(N, c, base >> i, base >> i, generator=gen, dtype=torch.float64) for i, c in enumerate(chans)]
    first = {2: 1, 4: 2, 8: 3, 16: 4}[DLA_UP["down_ratio"]]
    cot = torch.randn(N, chans[first], base >> first, base >> first, generator=gen, dtype=torch.float64)
    return pyramid, cot


def dla_up_state(module, seed=72):
    """the project's seeded formula (tests/helpers_matching.init_state) over the module's own keys and shapes: every
    convolution, the zero-initialised conv_offset included, gets weights of He scale"""
    from tests.helpers_matching import init_state
    return init_state(module.state_dict(), seed)


def dla_up_run(module, pyramid, cot, dtype, device="cpu"):
    """training-mode forward and backward -> (out, {parameter or 'input<i>': gradient}); unused inputs have no entry"""
    module = module.to(device=device, dtype=dtype).train()
    xs = [p.to(device=device, dtype=dtype).requires_grad_() for p in pyramid]
    out = module(list(xs))
    names = [k for k, _ in module.named_parameters()] + ["input%d" % i for i in range(len(xs))]
    leaves = [p for _, p in module.named_parameters()] + xs
    grads = torch.autograd.grad(out, leaves, cot.to(device=device, dtype=dtype), allow_unused=True)
    return out.detach(), {k: g.detach() for k, g in zip(names, grads) if g is not None}
