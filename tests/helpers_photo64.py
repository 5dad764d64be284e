"""A plain float64 restatement, with autograd, of what photo_fused_fwd_kernel / photo_fused_bwd_kernel compute for the
pinhole model, plus the seeded inputs and the shape lists of the strip-seam sweep (tests/test_photo64_cpu.py pins this
file on the CPU, tests/test_photo_fused_seams_gpu.py compares the kernels with it).

The chain is the one of oracle/fsnet_oracle.py (backproject, project, bilinear / border / align_corners=True sampling,
SSIM on reflection padding, 0.85 / 0.15 mix, overlap test, the constant 100, per-pixel minimum against the identity
terms) with three differences: every intermediate is float64 (K, K^-1 and the pixel grid included) unless another
dtype is asked for, the per-scale depth maps have any size, and the bilinear sampler is written out so that it can take
a coordinate shift sigma: every DECISION on a sample coordinate (cell index, border clamp, the inside test and the
nearest index of the overlap mask) is taken on coordinate + sigma, the interpolation itself on the coordinate.  With
sigma = 0 it is F.grid_sample.  A prescribed selection map (values 0..4 as the forward kernel writes them) replaces the
chain's own argmin: 0 / 1 the identity terms, 2 / 3 the reprojection terms, 4 the constant 100."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _f32(v):
    return float(np.float32(v))


# the kernels' constants are fp32 literals: the same values here, so that only the arithmetic differs
C1, C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))
W_SSIM, W_L1 = _f32(0.85), _f32(0.15)

# --------------------------------------------------------------------------------------------- shapes of the sweep
# forward strips: 62 columns x 16 rows; backward strips: 60 columns x 32 rows
SHAPES_A = ((24, 56, 2), (16, 64, 2), (32, 120, 3), (40, 128, 2))            # (H, W, B), scales 0..3 (sides % 8 == 0)
HS_B = (2, 3, 15, 16, 17, 31, 32, 33, 34)
WS_B = (2, 3, 59, 60, 61, 62, 63, 64, 119, 120, 121, 123, 124, 125)
SHAPES_B = tuple([(HS_B[i % 9], w) for i, w in enumerate(WS_B)] + [(HS_B[(i + 4) % 9], w) for i, w in enumerate(WS_B)]
                 + [(33, 61), (33, 125)])                                     # scale 0 only; B alternates 1, 2
CASES_C = ((33, 61, ((33, 61), (16, 30), (9, 17), (4, 7))),                   # free depth-map sizes, C ABI, B = 2
           (34, 125, ((17, 62), (31, 120))),
           (20, 70, ((1, 1), (1, 9), (7, 1))))
SHAPES_D = ((32, 120, 2), (40, 128, 2))                                       # option runs
OPTIONS_D = ("no_patched_mask", "no_overlap_mask", "motion_mask", "gout")


def multi_strip(H, W):
    return H > 16 and W > 62


# --------------------------------------------------------------------------------------------- inputs
def _rot(v):
    """Rodrigues, f64: v [3] -> [3,3]"""
    th = float(np.linalg.norm(v))
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


_cases = {}


def blob_mask(H, W):
    """8 x 8 patches on the two frame corners that have the virtual rows / columns and the last strips, and one across
    the first strip seams of both kernels (columns 60 and 62, rows 16 or 32)"""
    m = np.zeros((H, W), bool)
    m[:8, :8] = True
    m[max(H - 8, 0):, max(W - 8, 0):] = True
    cy = 32 if H > 32 else (16 if H > 16 else H // 2)
    cx = 61 if W > 62 else W // 2
    m[max(cy - 4, 0):cy + 4, max(cx - 4, 0):cx + 4] = True
    return m


def make_case(B, H, W, maps=None, seed=0, blobs=False):
    """Seeded host inputs (fp32 arrays as the kernels read them, the patched mask f64): frames in [0, 1] cut from one
    canvas of smooth structure + per-pixel texture at different offsets (+ a little independent noise), depths 3..23,
    a non-integer principal point, and per (sample, frame) a small rotation about all three axes and a translation
    with three non-zero components, sized so that a tenth to a fifth of the samples leave the source frame.
    blobs: outside blob_mask() the source frames are the target + a little noise (more of it in the second), so that the
    identity terms win there and the gradient lives on the patches (and the motion mask is 1 outside them).  A coarse depth map has so few cells
    that a handful of samples next to a sampler cell boundary anywhere in the frame puts more than 2 % of its cells
    under the allowance A; with the gradient confined to the patches a seed exists at which none does."""
    maps = tuple(maps) if maps is not None else ((H, W),)
    key = (B, H, W, maps, seed, blobs)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(7919 * seed + 1000003 * B + 1009 * H + W)
    P = 12
    yy, xx = np.meshgrid(np.arange(H + 2 * P) / max(H, 8), np.arange(W + 2 * P) / max(W, 8), indexing="ij")
    fr, ph = 2 + 5 * rng.random((B, 3, 1, 1)), 6.28 * rng.random((B, 3, 1, 1))
    canvas = 0.5 + 0.22 * np.sin(fr * 6.28 * xx + ph) * np.cos(fr * 3.1 * yy + 0.5 * ph) \
        + 0.12 * np.sin(23.0 * xx * yy + ph) + 0.30 * (rng.random((B, 3, H + 2 * P, W + 2 * P)) - 0.5)
    imgs = []
    for oy, ox in ((0, 0), (1, -3), (-2, 4)):
        im = canvas[:, :, P + oy:P + oy + H, P + ox:P + ox + W] + 0.06 * (rng.random((B, 3, H, W)) - 0.5)
        if blobs and (oy, ox) != (0, 0):
            amp = 0.03 if len(imgs) == 1 else 0.12
            im = np.where(blob_mask(H, W), im, imgs[0] + amp * (rng.random((B, 3, H, W)) - 0.5))
        imgs.append(np.clip(im, 0.0, 1.0).astype(np.float32))
    depths = [(3 + 20 * rng.random((B, 1, h, w))).astype(np.float32) for h, w in maps]
    P2 = np.zeros((B, 3, 4), np.float32)
    P2[:, 0, 0], P2[:, 0, 2] = 0.58 * W, 0.5 * W + 0.37
    P2[:, 1, 1], P2[:, 1, 2] = 1.92 * H, 0.5 * H - 0.21
    P2[:, 2, 2] = 1
    Ts = []
    for f in range(2):
        T = np.zeros((B, 4, 4))
        for b in range(B):
            sg = 1.0 if f == 0 else -1.0
            j = 1 + 0.25 * rng.random(6)
            aa = np.array([sg * 0.024 * j[0], -sg * 0.10 * j[1], sg * 0.03 * j[2] * (1 if b % 2 else -1)])
            T[b, :3, :3] = _rot(aa)
            T[b, :3, 3] = [sg * 0.25 * j[3], -0.07 * j[4], -sg * 0.6 * j[5]]
            T[b, 3, 3] = 1
        Ts.append(T.astype(np.float32))
    mm = rng.random((B, H, W)) < 0.3
    if blobs:
        mm = np.where(blob_mask(H, W), mm, True)
    case = dict(B=B, H=H, W=W, maps=maps, img0=imgs[0], src=[imgs[1], imgs[2]], depths=depths, P2=P2, T=Ts,
                patched_mask=(rng.random((B, H, W)) < 0.7).astype(np.float64), motion_mask=mm.astype(np.float32))
    _cases[key] = case
    return case


# seeds per input: the smallest one (from 1) at which the input meets the conditions of check_conditions(); the
# coarse maps have so few cells that the 2 % cap on cells next to a sampler cell boundary tolerates none or one
SEEDS = {"a-32x120-B3": 2, "b-20-3x63": 2, "c-20x70": 4, "d-40x128-motion_mask": 3}         # (every other input: seed 1)


def case_named(name):
    """'a-HxW-Bn', 'b-<index>-HxW', 'c-HxW', 'd-HxW-<option>' -> (case, options)"""
    kind, rest = name.split("-", 1)
    seed = SEEDS.get(name, 1)
    if kind == "a":
        H, W, B = [s_ for s_ in SHAPES_A if "%dx%d-B%d" % s_ == rest][0]
        return make_case(B, H, W, [(H >> s, W >> s) for s in range(4)], seed, True), {}
    if kind == "b":
        i = int(rest.split("-")[0])
        H, W = SHAPES_B[i]
        return make_case(1 + i % 2, H, W, None, seed), {}
    if kind == "c":
        H, W, maps = [c for c in CASES_C if "%dx%d" % c[:2] == rest][0]
        return make_case(2, H, W, maps, seed, True), {}
    hw, opt = rest.split("-", 1)
    H, W, B = [s_ for s_ in SHAPES_D if "%dx%d" % s_[:2] == hw][0]
    return make_case(B, H, W, [(H >> s, W >> s) for s in range(4)], seed, True), options(opt)


NAMES_A = tuple("a-%dx%d-B%d" % s_ for s_ in SHAPES_A)
NAMES_B = tuple("b-%d-%dx%d" % ((i,) + SHAPES_B[i]) for i in range(len(SHAPES_B)))
NAMES_C = tuple("c-%dx%d" % c[:2] for c in CASES_C)
NAMES_D = tuple("d-%dx%d-%s" % (s_[0], s_[1], o) for s_ in SHAPES_D for o in OPTIONS_D)
ALL_NAMES = NAMES_A + NAMES_B + NAMES_C + NAMES_D


def options(name):
    return {"no_patched_mask": dict(use_patched_mask=False), "no_overlap_mask": dict(overlapped_mask=False),
            "motion_mask": dict(use_motion_mask=True), "gout": dict(gout=0.37)}[name]


# --------------------------------------------------------------------------------------------- the chain
def sample_bilinear_border(src, ix, iy, sigma=0.0):
    """src [B,C,H,W], ix / iy [B,H,W] in pixels -> (pred [B,C,H,W], d pred / d ix, d pred / d iy of the cell).
    bilinear, border padding, align_corners=True; decisions on (ix + sigma, iy + sigma)."""
    B, C, H, W = src.shape

    def axis(c, n):
        cs = c.detach() + sigma
        cc = torch.where(cs <= 0, torch.zeros_like(c), torch.where(cs >= n - 1, torch.full_like(c, n - 1), c))
        i0 = cs.clamp(0, n - 1).floor().clamp(max=n - 2)
        return cc - i0, i0.long()

    wx, x0 = axis(ix, W)
    wy, y0 = axis(iy, H)
    flat = src.reshape(B, C, H * W)

    def tap(dy, dx):
        idx = ((y0 + dy) * W + x0 + dx).reshape(B, 1, H * W).expand(B, C, H * W)
        return flat.gather(2, idx).reshape(B, C, H, W)

    t00, t01, t10, t11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    wx, wy = wx.unsqueeze(1), wy.unsqueeze(1)
    pred = (1 - wy) * ((1 - wx) * t00 + wx * t01) + wy * ((1 - wx) * t10 + wx * t11)
    jx = (1 - wy) * (t01 - t00) + wy * (t11 - t10)
    jy = (1 - wx) * (t10 - t00) + wx * (t11 - t01)
    return pred, jx.detach(), jy.detach()


def sample_nearest_zeros(mask, ix, iy, sigma=0.0):
    """mask [B,H,W] or None (= ones); -> bool [B,H,W]: the nearest sample (round half to even, zeros padding) == 1"""
    B, H, W = ix.shape
    xn, yn = torch.round(ix.detach() + sigma), torch.round(iy.detach() + sigma)
    inside = (xn >= 0) & (xn <= W - 1) & (yn >= 0) & (yn <= H - 1)
    if mask is None:
        return inside
    idx = (yn.clamp(0, H - 1) * W + xn.clamp(0, W - 1)).long().reshape(B, H * W)
    return inside & (mask.reshape(B, H * W).gather(1, idx).reshape(B, H, W) == 1)


def ssim_term(x, y):
    xp, yp = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(xp, 3, 1), F.avg_pool2d(yp, 3, 1)
    sg_x = F.avg_pool2d(xp * xp, 3, 1) - mu_x * mu_x
    sg_y = F.avg_pool2d(yp * yp, 3, 1) - mu_y * mu_y
    sg_xy = F.avg_pool2d(xp * yp, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + C1) * (2 * sg_xy + C2)
    d = (mu_x * mu_x + mu_y * mu_y + C1) * (sg_x + sg_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def reproj_term(pred, target):
    """[B,3,H,W] x 2 -> [B,H,W]"""
    return W_SSIM * ssim_term(pred, target).mean(1) + W_L1 * torch.abs(target - pred).mean(1)


def photo_chain(case, sel=None, sigma=0.0, dtype=F64, use_patched_mask=True, overlapped_mask=True,
                use_motion_mask=False, gout=1.0, sampler=None, grads=True):
    """-> dict with, per scale s (lists) and frame f:
    cand [B,4,H,W] (ident0, ident1, reproj0, reproj1 with 100 where the sample missed; +inf for the identity planes
    under a motion mask), argmin [B,H,W] (0..4), pred [2,B,3,H,W], ov [2,B,H,W] bool, ix / iy [2,B,H,W],
    jx / jy [2,B,3,H,W] (cell slopes of pred), loss_sums [S,B] f64, total (the differentiated scalar),
    g_depth[s] [B,1,h,w], g_up[s] [B,H,W], dT[f] [B,4,4].
    sel: list per scale of [B,H,W] integer maps 0..4, or None for the chain's own argmin.
    sampler: None (the sampler of this file) or "grid_sample" (F.grid_sample; sigma must be 0)."""
    B, H, W = case["B"], case["H"], case["W"]
    S = len(case["maps"])
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    img0, srcs = t(case["img0"]), [t(a) for a in case["src"]]
    pm = torch.from_numpy(case["patched_mask"]) if use_patched_mask else None       # f64 also in an fp32 run
    mm = t(case["motion_mask"]) if use_motion_mask else None
    K64 = torch.from_numpy(case["P2"][:, :3, :3]).to(F64)
    K, invK = K64.to(dtype), torch.linalg.inv(K64).to(dtype)
    Ts = [t(a).requires_grad_(grads) for a in case["T"]]
    dmaps = [t(a).requires_grad_(grads) for a in case["depths"]]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=dtype)], 0)
    rays = torch.matmul(invK, pix)                                                    # [B,3,HW]
    if mm is None:
        ident = [reproj_term(srcs[f], img0) for f in range(2)]
    else:
        ident = [torch.full((B, H, W), float("inf"), dtype=dtype)] * 2
    hundred = torch.full((B, H, W), 100.0, dtype=dtype)
    out = dict(cand=[], argmin=[], pred=[], ov=[], ix=[], iy=[], jx=[], jy=[], ups=[])
    loss_sums, total = [], 0.0
    denom = (pm.sum() if pm is not None else float(B * H * W)) + 1e-6
    for s in range(S):
        up = F.interpolate(dmaps[s], [H, W], mode="bilinear", align_corners=True)
        out["ups"].append(up)
        cam = up.reshape(B, 1, H * W) * rays
        rv, ovs, preds, ixs, iys, jxs, jys = [], [], [], [], [], [], []
        for f in range(2):
            Pf = torch.matmul(K, Ts[f][:, :3, :])
            c = torch.matmul(Pf[:, :, :3], cam) + Pf[:, :, 3:]
            u, v = c[:, 0] / (c[:, 2] + 1e-7), c[:, 1] / (c[:, 2] + 1e-7)
            un, vn = (u / (W - 1) - 0.5) * 2, (v / (H - 1) - 0.5) * 2
            if sampler == "grid_sample":
                assert sigma == 0.0
                grid = torch.stack([un, vn], -1).reshape(B, H, W, 2)
                pred = F.grid_sample(srcs[f], grid, padding_mode="border", align_corners=True)
                jx = jy = torch.zeros_like(pred)
            ix, iy = ((un + 1) / 2 * (W - 1)).reshape(B, H, W), ((vn + 1) / 2 * (H - 1)).reshape(B, H, W)
            if sampler != "grid_sample":
                pred, jx, jy = sample_bilinear_border(srcs[f], ix, iy, sigma)
            ov = sample_nearest_zeros(pm, ix, iy, sigma) if overlapped_mask else torch.ones(B, H, W, dtype=torch.bool)
            rv.append(reproj_term(pred, img0)); ovs.append(ov); preds.append(pred.detach())
            ixs.append(ix.detach()); iys.append(iy.detach()); jxs.append(jx); jys.append(jy)
        cand = torch.stack(ident + [torch.where(ovs[f], rv[f], hundred) for f in range(2)], 1)
        am = cand.detach().argmin(1)                                    # (the first of equal candidates, as the kernel)
        am = torch.where(((am == 2) & ~ovs[0]) | ((am == 3) & ~ovs[1]), torch.full_like(am, 4), am)
        if sel is None:
            chosen = cand.min(1)[0]
        else:
            five = torch.stack(ident + rv + [hundred], 1)
            chosen = five.gather(1, torch.as_tensor(sel[s]).long().reshape(B, 1, H, W)).squeeze(1)
        valued = chosen if pm is None else chosen.to(F64) * pm           # float64 promotion under an f64 mask
        loss_sums.append(valued.detach().to(F64).sum((1, 2)))
        if mm is not None:
            chosen = chosen.detach() * mm + chosen * (1 - mm)
            valued = chosen if pm is None else chosen.to(F64) * pm
        total = total + valued.to(F64).sum() / denom
        out["cand"].append(cand.detach()); out["argmin"].append(am)
        out["pred"].append(torch.stack(preds)); out["ov"].append(torch.stack(ovs))
        out["ix"].append(torch.stack(ixs)); out["iy"].append(torch.stack(iys))
        out["jx"].append(torch.stack(jxs)); out["jy"].append(torch.stack(jys))
    total = total * gout / S
    out["loss_sums"] = torch.stack(loss_sums)
    out["total"] = total.detach()
    ups = out.pop("ups")
    if grads:
        if total.requires_grad:
            gr = torch.autograd.grad(total, dmaps + ups + Ts, allow_unused=True)
            gr = [torch.zeros_like(x) if g is None else g for g, x in zip(gr, dmaps + ups + Ts)]
        else:                                                            # (no pixel selected a reprojection term)
            gr = [torch.zeros_like(x) for x in dmaps + ups + Ts]
        out["g_depth"] = [g.to(F64) for g in gr[:S]]
        out["g_up"] = [g.to(F64).reshape(B, H, W) for g in gr[S:2 * S]]
        out["dT"] = [g.to(F64) for g in gr[2 * S:]]
    return out


def upsample_transpose(a, h, w):
    """a [B,H,W] >= 0 pushed through the transpose of the bilinear align_corners=True upsample -> [B,1,h,w]"""
    B, H, W = a.shape
    z = torch.zeros(B, 1, h, w, dtype=F64, requires_grad=True)
    up = F.interpolate(z, [H, W], mode="bilinear", align_corners=True)
    return torch.autograd.grad(up, z, a.reshape(B, 1, H, W).to(F64))[0]


# --------------------------------------------------------------------------------------------- yardsticks
def near_half_integer(c, delta):
    return (c - (torch.floor(c) + 0.5)).abs() < delta


def yardsticks(case, opts, sel=None):
    """Everything a comparison needs for one input: R64 (free selection), R64 / R32 under `sel` (default: R64's own
    argmin) at sigma = 0 and R64 at sigma = +-delta, the reference's own fp32 noise e per quantity, delta, the
    excused cells and the allowance A."""
    H, W, S = case["H"], case["W"], len(case["maps"])
    free64 = photo_chain(case, grads=False, **opts)
    free32 = photo_chain(case, dtype=torch.float32, grads=False, **opts)
    y = dict(free64=free64, free32=free32)
    # coordinate noise of the fp32 reference where a decision can depend on it (samples within a pixel of the frame)
    dc = 0.0
    for s in range(S):
        near = (free64["ix"][s] > -1) & (free64["ix"][s] < W) & (free64["iy"][s] > -1) & (free64["iy"][s] < H)
        for k in ("ix", "iy"):
            d = (free32[k][s].to(F64) - free64[k][s]).abs()[near]
            dc = max(dc, float(d.max()) if d.numel() else 0.0)
    y["e_coord"] = dc
    delta = y["delta"] = max(2e-4, 4 * dc)
    ovm = opts.get("overlapped_mask", True)
    y["ov_excused"], y["sel_excused"], y["e_cand"], y["e_pred"] = [], [], [], []
    for s in range(S):
        ix, iy = free64["ix"][s], free64["iy"][s]
        ex = (near_half_integer(ix, delta) | near_half_integer(iy, delta)) if ovm else torch.zeros_like(ix, dtype=torch.bool)
        y["ov_excused"].append(ex)
        c64, c32 = free64["cand"][s], free32["cand"][s].to(F64)
        same = torch.isfinite(c64) & ((c64 == 100) == (c32 == 100))
        e_c = float((c32 - c64)[same].abs().max())
        y["e_cand"].append(e_c)
        two = torch.topk(c64, 2, dim=1, largest=False)[0]
        # (two samples that both missed the frame tie at the constant 100 in every arithmetic: nothing to excuse)
        y["sel_excused"].append(((two[:, 1] - two[:, 0]) < 4 * e_c) & ~((two[:, 0] == 100) & (two[:, 1] == 100)))
        y["e_pred"].append(float((free32["pred"][s].to(F64) - free64["pred"][s]).abs().max()))
    sel = [a.clone() for a in free64["argmin"]] if sel is None else sel
    y["sel"] = sel
    r0 = y["r0"] = photo_chain(case, sel=sel, **opts)
    r32 = y["r32"] = photo_chain(case, sel=sel, dtype=torch.float32, **opts)
    rp = photo_chain(case, sel=sel, sigma=delta, **opts)
    rm = photo_chain(case, sel=sel, sigma=-delta, **opts)
    y["e_loss"] = float((r32["loss_sums"] - r0["loss_sums"]).abs().max())
    y["e_depth"] = [float((r32["g_depth"][s] - r0["g_depth"][s]).abs().max()) for s in range(S)]
    y["e_dT"] = [float((r32["dT"][f] - r0["dT"][f]).abs().max()) for f in range(2)]
    y["A"] = []
    for s, (h, w) in enumerate(case["maps"]):
        a = (rp["g_up"][s] - r0["g_up"][s]).abs() + (rm["g_up"][s] - r0["g_up"][s]).abs()
        y["A"].append(upsample_transpose(a, h, w))
    y["A_dT"] = [(rp["dT"][f] - r0["dT"][f]).abs() + (rm["dT"][f] - r0["dT"][f]).abs() for f in range(2)]
    return y


def out_of_frame_share(ref, case, s, f):
    """share of the samples of frame f at scale s whose nearest texel lies outside the source image"""
    return 1.0 - float(sample_nearest_zeros(None, ref["ix"][s][f], ref["iy"][s][f]).double().mean())


def check_conditions(case, opts, y):
    """The conditions under which the comparisons of the sweep mean something; -> list of violations (empty = fine)"""
    H, W, S = case["H"], case["W"], len(case["maps"])
    bad = []
    r64, r32 = y["free64"], y["free32"]
    for s in range(S):
        if multi_strip(H, W):
            for f in range(2):
                share = out_of_frame_share(r64, case, s, f)
                if not 0.05 <= share <= 0.25:
                    bad.append("scale %d frame %d: %.3f of the samples leave the frame" % (s, f, share))
        exc = y["ov_excused"][s].any(0) | y["sel_excused"][s]
        if float(exc.double().mean()) > 0.005:
            bad.append("scale %d: %.4f of the cells excused" % (s, float(exc.double().mean())))
        if bool(((r32["ov"][s] != r64["ov"][s]) & ~y["ov_excused"][s]).any()):
            bad.append("scale %d: the fp32 reference's ov differs outside the excused cells" % s)
        if bool(((r32["argmin"][s] != r64["argmin"][s]) & ~exc).any()):
            bad.append("scale %d: the fp32 reference's selection differs outside the excused cells" % s)
        big = float((y["A"][s] > 4 * y["e_depth"][s]).double().mean())
        if big > 0.02:
            bad.append("scale %d: allowance above 4 e on %.4f of the cells" % (s, big))
    return bad
