"""The float64 chain of tests/helpers_photo64.py over N = 1..4 source frames, for the kernels of photo_multi.hip
(tests/test_photo64n_cpu.py pins this file on the CPU, tests/test_photo_multi_gpu.py compares the kernels with it).

Same chain, same samplers (imported), same yardsticks; what changes is the frame count and with it the selection code:
0..N-1 the identity terms, N..2N-1 the reprojection terms, 2N the constant 100 (a selected reprojection term whose
sample missed the source frame).  With N = 2 every function here returns what its two-frame original returns.

Inputs (make_case_n): the frames are cut from one canvas at different offsets as in make_case, and source frame k is
the clean one (little independent noise) in vertical band k of the image and noisy in the others, so that every one of
the 2N candidates wins somewhere and every frame's backward and every identity plane is exercised
(check_conditions_n's extra condition)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import helpers_photo64 as P
from tests.helpers_photo64 import F64, reproj_term, sample_bilinear_border, sample_nearest_zeros, upsample_transpose

OFFSETS = ((1, -3), (-2, 4), (2, 3), (-1, -4))          # canvas offsets of the source frames (the target: (0, 0))
MIN_SHARE = 0.02                                         # every candidate wins at least this share of scale 0

_cases = {}


def big_enough(B, H, W, N):
    """can every one of 2N candidates take 2 % of the pixels at all?  Each frame's band has to exist: at least 8 columns
    wide on at least 8 rows, so that 2 % of the frame is more than a pixel or two of it.  That leaves out the 2- and
    3-pixel sides of the sweep only (2 x 2 x B has fewer pixels than N = 4 has candidates); there the condition is not
    asked."""
    return H >= 8 and W >= 8 * N


BAND_AREA = 0.065      # share of the frame in which one frame's warp competes (its reprojection term wins ~ 45 % of it)


def blob_mask_n(H, W, N):
    """where the reprojection terms compete when the gradient is confined (blobs=True): one patch per band of BAND_AREA
    of the frame, so that every frame's reprojection term can
    win 2 % of the pixels but no more than it must (every selected pixel next to a sampler cell boundary puts up to four
    cells of a coarse depth map under the allowance, and the cap on those is 2 % of a few dozen cells).  The first
    band's patch lies in the top left corner and the last band's in the bottom right one (the virtual rows / columns);
    the others start at their band's first column across the kernels' first row seam (rows 16 or 32), which puts the
    column seams 60 / 62 inside one of them whenever a band starts there."""
    m = np.zeros((H, W), bool)
    # (N = 1: the one band's share as three patches — the two corners and the seams — laid out like three bands)
    L = 3 if N == 1 else N
    area = BAND_AREA * H * W * N / L
    cy = 32 if H > 32 else (16 if H > 16 else H // 2)
    for k in range(L):
        lo, hi = (k * W + L - 1) // L, ((k + 1) * W + L - 1) // L
        bh = int(min(H, max(2, round(np.sqrt(area / 2)))))
        bw = int(min(hi - lo, max(1, np.ceil(area / bh))))
        if k == 0:
            r0, c0 = 0, 0
        elif k == L - 1:
            r0, c0 = H - bh, W - bw
        else:
            r0, c0 = min(max(cy - bh // 2, 0), H - bh), lo
        m[r0:r0 + bh, c0:c0 + bw] = True
    return m


def make_case_n(B, H, W, N, maps=None, seed=0, blobs=False):
    """make_case for N source frames.  Band k of the image (columns [k W / N, (k + 1) W / N)) is where source frame k
    carries little independent noise and the other frames much, so that frame k's two terms win there.  Which of the
    two: where the reprojection terms are to compete (inside the blobs; without blobs: below the top third of the rows)
    a source frame is the canvas shifted against the target by what its warp displaces the image centre at mid depth,
    so that the warped frame lines up with the target to within the parallax and beats the identity term, which meets
    the shift whole.  Elsewhere a source frame is the target + a little noise, and the identity term wins."""
    maps = tuple(maps) if maps is not None else ((H, W),)
    key = (B, H, W, N, maps, seed, blobs)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(7919 * seed + 1000003 * B + 1009 * H + W + 104729 * N)
    Pd = 16
    P2 = np.zeros((B, 3, 4), np.float32)
    P2[:, 0, 0], P2[:, 0, 2] = 0.58 * W, 0.5 * W + 0.37
    P2[:, 1, 1], P2[:, 1, 2] = 1.92 * H, 0.5 * H - 0.21
    P2[:, 2, 2] = 1
    Ts = []
    for f in range(N):
        T = np.zeros((B, 4, 4))
        for b in range(B):
            sg = 1.0 if f % 2 == 0 else -1.0
            up = 1.0 if f < 2 else -1.0                   # frames 2, 3: the vertical components the other way round
            j = 1 + 0.25 * rng.random(6)
            aa = np.array([sg * up * 0.024 * j[0], -sg * 0.10 * j[1], sg * 0.03 * j[2] * (1 if b % 2 else -1)])
            T[b, :3, :3] = P._rot(aa)
            T[b, :3, 3] = [sg * 0.25 * j[3], -up * 0.07 * j[4], -sg * 0.6 * j[5]]
            T[b, 3, 3] = 1
        Ts.append(T.astype(np.float32))
    yy, xx = np.meshgrid(np.arange(H + 2 * Pd) / max(H, 8), np.arange(W + 2 * Pd) / max(W, 8), indexing="ij")
    fr, ph = 2 + 5 * rng.random((B, 3, 1, 1)), 6.28 * rng.random((B, 3, 1, 1))
    smooth = 0.5 + 0.22 * np.sin(fr * 6.28 * xx + ph) * np.cos(fr * 3.1 * yy + 0.5 * ph) + 0.12 * np.sin(23.0 * xx * yy + ph)
    texture = rng.random((B, 3, H + 2 * Pd, W + 2 * Pd)) - 0.5
    band = np.minimum(np.arange(W) * N // max(W, 1), N - 1)                      # [W]: the frame that is clean there
    if blobs:
        compete = blob_mask_n(H, W, N)
    else:
        compete = np.zeros((H, W), bool)
        compete[H // 3:] = True
    canvas = smooth + 0.30 * texture
    img0 = np.clip(canvas[:, :, Pd:Pd + H, Pd:Pd + W] + 0.06 * (rng.random((B, 3, H, W)) - 0.5), 0.0, 1.0)
    srcs = []
    for k in range(N):
        clean = (band == k)[None, None, None, :]
        im = np.empty((B, 3, H, W))
        for b in range(B):
            # where the warp of frame k sends the image centre at depth 10, in pixels
            K = P2[b, :, :3].astype(np.float64)
            c = np.array([0.5 * (W - 1), 0.5 * (H - 1), 1.0])
            q = K @ (Ts[k][b, :3, :3].astype(np.float64) @ (10.0 * (np.linalg.inv(K) @ c)) + Ts[k][b, :3, 3])
            dx, dy = q[0] / q[2] - c[0], q[1] / q[2] - c[1]
            ox, oy = int(np.clip(np.rint(-dx), -Pd + 1, Pd - 1)), int(np.clip(np.rint(-dy), -Pd + 1, Pd - 1))
            im[b] = canvas[b, :, Pd + oy:Pd + oy + H, Pd + ox:Pd + ox + W]
        im = im + np.where(clean, 0.04, 0.35) * (rng.random((B, 3, H, W)) - 0.5)
        near = img0 + np.where(clean, 0.02, 0.12) * (rng.random((B, 3, H, W)) - 0.5)
        srcs.append(np.clip(np.where(compete, im, near), 0.0, 1.0).astype(np.float32))
    depths = [(3 + 20 * rng.random((B, 1, h, w))).astype(np.float32) for h, w in maps]
    mm = rng.random((B, H, W)) < 0.3
    if blobs:
        mm = np.where(compete, mm, True)
    case = dict(B=B, H=H, W=W, N=N, maps=maps, img0=img0.astype(np.float32), src=srcs, depths=depths, P2=P2, T=Ts,
                patched_mask=(rng.random((B, H, W)) < 0.7).astype(np.float64), motion_mask=mm.astype(np.float32))
    _cases[key] = case
    return case


# --------------------------------------------------------------------------------------------- the chain
def photo_chain_n(case, sel=None, sigma=0.0, dtype=F64, use_patched_mask=True, overlapped_mask=True,
                  use_motion_mask=False, gout=1.0, sampler=None, grads=True):
    """photo_chain of helpers_photo64.py with N = len(case["src"]) frames: cand [B,2N,H,W], argmin 0..2N, pred
    [N,B,3,H,W], ov / ix / iy [N,B,H,W], dT[f] for f < N; sel: per scale [B,H,W] maps 0..2N or None."""
    B, H, W = case["B"], case["H"], case["W"]
    S = len(case["maps"])
    N = len(case["src"])
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
        ident = [reproj_term(srcs[f], img0) for f in range(N)]
    else:
        ident = [torch.full((B, H, W), float("inf"), dtype=dtype)] * N
    hundred = torch.full((B, H, W), 100.0, dtype=dtype)
    out = dict(cand=[], argmin=[], pred=[], ov=[], ix=[], iy=[], jx=[], jy=[], ups=[])
    loss_sums, total = [], 0.0
    denom = (pm.sum() if pm is not None else float(B * H * W)) + 1e-6
    for s in range(S):
        up = F.interpolate(dmaps[s], [H, W], mode="bilinear", align_corners=True)
        out["ups"].append(up)
        cam = up.reshape(B, 1, H * W) * rays
        rv, ovs, preds, ixs, iys, jxs, jys = [], [], [], [], [], [], []
        for f in range(N):
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
        cand = torch.stack(ident + [torch.where(ovs[f], rv[f], hundred) for f in range(N)], 1)
        am = cand.detach().argmin(1)                                    # (the first of equal candidates, as the kernel)
        missed = torch.zeros_like(am, dtype=torch.bool)
        for f in range(N):
            missed = missed | ((am == N + f) & ~ovs[f])
        am = torch.where(missed, torch.full_like(am, 2 * N), am)
        if sel is None:
            chosen = cand.min(1)[0]
        else:
            allc = torch.stack(ident + rv + [hundred], 1)
            chosen = allc.gather(1, torch.as_tensor(sel[s]).long().reshape(B, 1, H, W)).squeeze(1)
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


def yardsticks_n(case, opts, sel=None):
    """yardsticks() of helpers_photo64.py for N frames (the same quantities under the same names)"""
    H, W, S = case["H"], case["W"], len(case["maps"])
    N = len(case["src"])
    free64 = photo_chain_n(case, grads=False, **opts)
    free32 = photo_chain_n(case, dtype=torch.float32, grads=False, **opts)
    y = dict(free64=free64, free32=free32)
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
        ex = (P.near_half_integer(ix, delta) | P.near_half_integer(iy, delta)) if ovm else torch.zeros_like(ix, dtype=torch.bool)
        y["ov_excused"].append(ex)
        c64, c32 = free64["cand"][s], free32["cand"][s].to(F64)
        same = torch.isfinite(c64) & ((c64 == 100) == (c32 == 100))
        e_c = float((c32 - c64)[same].abs().max())
        y["e_cand"].append(e_c)
        if c64.shape[1] >= 2:
            two = torch.topk(c64, 2, dim=1, largest=False)[0]
            # (two samples that both missed the frame tie at the constant 100 in every arithmetic: nothing to excuse)
            y["sel_excused"].append(((two[:, 1] - two[:, 0]) < 4 * e_c) & ~((two[:, 0] == 100) & (two[:, 1] == 100)))
        else:
            y["sel_excused"].append(torch.zeros_like(c64[:, 0], dtype=torch.bool))
        y["e_pred"].append(float((free32["pred"][s].to(F64) - free64["pred"][s]).abs().max()))
    sel = [a.clone() for a in free64["argmin"]] if sel is None else sel
    y["sel"] = sel
    r0 = y["r0"] = photo_chain_n(case, sel=sel, **opts)
    r32 = y["r32"] = photo_chain_n(case, sel=sel, dtype=torch.float32, **opts)
    rp = photo_chain_n(case, sel=sel, sigma=delta, **opts)
    rm = photo_chain_n(case, sel=sel, sigma=-delta, **opts)
    y["e_loss"] = float((r32["loss_sums"] - r0["loss_sums"]).abs().max())
    y["e_depth"] = [float((r32["g_depth"][s] - r0["g_depth"][s]).abs().max()) for s in range(S)]
    y["e_dT"] = [float((r32["dT"][f] - r0["dT"][f]).abs().max()) for f in range(N)]
    y["A"] = []
    for s, (h, w) in enumerate(case["maps"]):
        a = (rp["g_up"][s] - r0["g_up"][s]).abs() + (rm["g_up"][s] - r0["g_up"][s]).abs()
        y["A"].append(upsample_transpose(a, h, w))
    y["A_dT"] = [(rp["dT"][f] - r0["dT"][f]).abs() + (rm["dT"][f] - r0["dT"][f]).abs() for f in range(N)]
    return y


def win_shares(ref, N, s=0):
    """share of the pixels of scale s each of the 2N candidates wins (the constant 100 counted for nobody)"""
    am = ref["argmin"][s]
    return [float((am == k).double().mean()) for k in range(2 * N)]


def check_conditions_n(case, opts, y):
    """check_conditions() of helpers_photo64.py for N frames, plus: at scale 0 every one of the 2N candidates (under a
    motion mask: every one of the N reprojection candidates) wins at least 2 % of the pixels, where big_enough()."""
    B, H, W, S = case["B"], case["H"], case["W"], len(case["maps"])
    N = len(case["src"])
    bad = []
    r64, r32 = y["free64"], y["free32"]
    for s in range(S):
        if P.multi_strip(H, W):
            for f in range(N):
                share = P.out_of_frame_share(r64, case, s, f)
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
    # one more decision the yardstick has no allowance for: the sign of the L1 term's gradient, sign(target - warped).
    # Where a selected reprojection term has |target - warped| within 4 e_pred in a channel (what the warped image may
    # differ by, FACTOR["pred"] of the GPU test), that sign is not decided by the input
    img0 = torch.from_numpy(case["img0"]).to(F64)
    for s in range(S):
        for f in range(N):
            picked = r64["argmin"][s] == N + f
            if opts.get("use_patched_mask", True):                 # (only where a gradient flows at all)
                picked = picked & (torch.from_numpy(case["patched_mask"]) == 1)
            if opts.get("use_motion_mask"):
                picked = picked & (torch.from_numpy(case["motion_mask"]) < 1)
            picked = picked.unsqueeze(1)
            close = (img0 - r64["pred"][s][f]).abs() < 4 * y["e_pred"][s]
            if bool((picked & close).any()):
                bad.append("scale %d frame %d: the L1 term's sign lies within the warped image's noise at %d pixels"
                           % (s, f, int((picked & close).any(1).sum())))
    if big_enough(B, H, W, N):
        shares = win_shares(r64, N)
        lo = N if opts.get("use_motion_mask") else 0
        for k in range(lo, 2 * N):
            if shares[k] < MIN_SHARE:
                bad.append("scale 0: candidate %d wins %.4f of the pixels" % (k, shares[k]))
    return bad


# --------------------------------------------------------------------------------------------- shapes and names
def strips():
    """[(columns, rows)] of the identity, forward and backward kernels' strips, from the library"""
    import ctypes as C
    import os
    from fsnet_amd.hip import binding, lib
    if not os.path.exists(os.environ.get("FSNET_HIP_LIB", binding.LIB_PATH)):
        from fsnet_amd.csrc import build as B        # (the shape lists are built when the test files are collected)
        B.build(verbose=False)
    out = []
    for which in range(3):
        c, r = C.c_int32(0), C.c_int32(0)
        assert lib.fs_photo_multi_strip(which, C.byref(c), C.byref(r)) == 0
        out.append((c.value, r.value))
    return out


def shapes_b(st):
    """the rule of helpers_photo64.SHAPES_B on the strips `st`: sides 2 and 3; a last strip of one, two and exactly a full
    strip of columns / rows for every kernel (c - 1, c, c + 1, c + 2 and 2 c - 1, 2 c, 2 c + 1 columns; r - 1, r, r + 1
    rows and two past the tallest strip); every height and width twice, and the two shapes in which the seams of two
    kernels both fall inside"""
    cols, rows = sorted({c for c, _ in st}), sorted({r for _, r in st})
    hs = sorted({2, 3} | {r + d for r in rows for d in (-1, 0, 1)} | {rows[-1] + 2})
    ws = sorted({2, 3} | {c + d for c in cols for d in (-1, 0, 1, 2)} | {2 * c + d for c in cols for d in (-1, 0, 1)})
    n = len(hs)
    out = [(hs[i % n], w) for i, w in enumerate(ws)] + [(hs[(i + 4) % n], w) for i, w in enumerate(ws)]
    both = [(rows[-1] + 1, cols[0] + 1), (rows[-1] + 1, 2 * cols[-1] + 1)]
    return tuple(out + [b for b in both if b not in out])


SHAPES_A = ((24, 64, 2), (40, 72, 2))                    # all four scales through ops.PhotometricLoss, N = 1, 3, 4
CASES_C = {4: (33, 61, ((33, 61), (16, 30), (9, 17), (4, 7))), 3: (20, 70, ((1, 1), (1, 9), (7, 1)))}
SHAPE_D = (40, 72, 2)                                    # the option runs, N = 3
N1_SWEEP = 4                                             # N = 1 runs four shapes of the sweep: the first, middle and last multi-strip one and the last single-strip one

# seeds per input: the smallest one (from 1) at which the input meets check_conditions_n()
SEEDS = {
    "n1-b-24-31x121": 4, "n1-b-29-33x125": 2, "n1-b-6-32x63": 2, "n3-a-24x64-B2": 3, "n3-a-40x72-B2": 21,
    "n3-b-11-15x123": 37, "n3-b-16-32x59": 2, "n3-b-18-34x61": 4, "n3-b-2-15x59": 3, "n3-b-23-17x120": 5,
    "n3-b-26-33x124": 9, "n3-b-27-34x125": 4, "n3-b-28-33x61": 4, "n3-b-29-33x125": 9, "n3-b-4-17x61": 2,
    "n3-b-8-34x119": 4, "n3-c-20x70": 33, "n3-d-40x72-gout": 21, "n3-d-40x72-motion_mask": 23,
    "n3-d-40x72-no_overlap_mask": 23, "n3-d-40x72-no_patched_mask": 23, "n4-a-24x64-B2": 13, "n4-a-40x72-B2": 50,
    "n4-b-11-15x123": 5, "n4-b-13-17x125": 4, "n4-b-14-17x2": 2, "n4-b-18-34x61": 3, "n4-b-20-3x63": 2,
    "n4-b-22-16x119": 2, "n4-b-23-17x120": 2, "n4-b-24-31x121": 3, "n4-b-27-34x125": 7, "n4-b-28-33x61": 5,
    "n4-b-4-17x61": 4, "n4-b-7-33x64": 2, "n4-b-8-34x119": 6, "n4-c-33x61": 33,
}   # (every other input: seed 1)


def names(st=None):
    """every input of tests/test_photo_multi_gpu.py by group"""
    sb = shapes_b(st if st is not None else strips())
    g = dict(a=[], b=[], c=[], d=[])
    for N in (1, 3, 4):
        g["a"] += ["n%d-a-%dx%d-B%d" % ((N,) + s_) for s_ in SHAPES_A]
    for N in (3, 4):
        g["b"] += ["n%d-b-%d-%dx%d" % ((N, i) + sb[i]) for i in range(len(sb))]
    multi = [i for i in range(len(sb)) if P.multi_strip(*sb[i])]
    pick = [multi[0], multi[len(multi) // 2], multi[-1], [i for i in range(len(sb)) if not P.multi_strip(*sb[i])][-1]]
    g["b"] += ["n1-b-%d-%dx%d" % ((i,) + sb[i]) for i in pick[:N1_SWEEP]]
    g["c"] = ["n%d-c-%dx%d" % ((N,) + CASES_C[N][:2]) for N in (4, 3)]
    g["d"] = ["n3-d-%dx%d-%s" % (SHAPE_D[0], SHAPE_D[1], o) for o in P.OPTIONS_D]
    return g


def case_named_n(name, st=None, seed=None):
    """'n<N>-a-HxW-Bn', 'n<N>-b-<index>-HxW', 'n<N>-c-HxW', 'n<N>-d-HxW-<option>' -> (case, options)"""
    nn, kind, rest = name.split("-", 2)
    N = int(nn[1:])
    seed = SEEDS.get(name, 1) if seed is None else seed
    if kind == "a":
        H, W, B = [s_ for s_ in SHAPES_A if "%dx%d-B%d" % s_ == rest][0]
        return make_case_n(B, H, W, N, [(H >> s, W >> s) for s in range(4)], seed, True), {}
    if kind == "b":
        i, hw = rest.split("-")
        H, W = [int(v) for v in hw.split("x")]
        # (blobs as well: the fewer pixels select a reprojection term, the further the kernels' loss sums stay from the
        # bound — their identity terms are ~ 20 x closer to float64 than the fp32 reference's, their warped terms as close
        # as the reference's, and the yardstick e_loss is one draw of the reference's summed noise)
        return make_case_n(1 + int(i) % 2, H, W, N, None, seed, True), {}
    if kind == "c":
        H, W, maps = CASES_C[N]
        return make_case_n(2, H, W, N, maps, seed, True), {}
    hw, opt = rest.split("-", 1)
    H, W, B = SHAPE_D
    return make_case_n(B, H, W, N, [(H >> s, W >> s) for s in range(4)], seed, True), P.options(opt)
