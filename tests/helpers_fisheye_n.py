"""Inputs of the fisheye (Mei) loss chain over N = 1, 3, 4 source frames, and the conditions they meet
(tests/test_fisheye_n_cpu.py asserts the conditions on the oracle alone; tests/test_fisheye_n_gpu.py compares the kernels of
fs_photo_mei_multi_* on these inputs; tools/gen_golden.py::gen_fisheye_nsrc runs the REAL FishEyeDecoder.loss on them).

The recipe of tools/gen_golden.py::gen_fisheye extended to a frame list (synthetic_batch(frame_ids=...), translation
0.6 f) leaves most of the 2N candidates of the per-pixel minimum without a pixel to win, so a wrong frame slot could not
show.  The source frames are built the way tests/helpers_photo64n.make_case_n(blobs=True) builds them for the pinhole
chain instead: the middle of the image (inside the ray-table mask) is cut into 2 x N cells, and in cell (0, k) frame k's
identity term, in cell (1, k) frame k's warped term is the best candidate:
  * the target is an analytic texture c(x, y) (wavelengths of 3 to 6 px) + a little noise;
  * in cell (0, k) frame k is the target itself (its identity term is exactly 0 there, which no warped term and no
    draw of the reference's tie-break noise comes near) and every other frame the target + 30 % noise;
  * in cell (1, k) frame k is the texture displaced by what frame k's warp displaces that pixel at the scale-0 depth,
    c(p - d_k(p)), so that the warped frame lines up with the target and the identity term meets the displacement
    whole; every other frame is the target + 30 % noise;
  * elsewhere frame k is the target + 2.4 k % noise: the first frame is the target itself and its identity term wins.
The translations are scaled so that no valid ray moves a sample by more than 0.42 px along either axis: a nearest-neighbour
sample of the overlap mask then never sits at a half-integer coordinate by the geometry (condition 3; the cells outside
the ray-table mask all project a fixed ray and land where the seed puts them).  A displacement of 0.2 .. 0.4 px changes the
texture by ~ 0.1, ten times the noise of a clean frame, so the cells are decided by a margin.

Conditions (check_conditions), at scale 0:
  1. every one of the 2N candidates is the per-pixel minimum on at least 1 % of the pixels;
  2. at most 0.001 of the pixels have their two smallest candidates within 1e-6 of each other;
  3. at most 0.0005 of the overlap-mask cells have a sample coordinate within 1e-3 px of a half-integer;
  4. (ours) the reference's tie-break noise (randn * 1e-5 on the identity terms, monodepth2_decoder.py:258-259; the
     kernels run without it in these tests) moves the total loss by at most 2.5e-7, half the bound the total is held to;
  5. (ours) and reverses no decision that carries a gradient: at every scale the pixels that select a warped term, and
     the term they select, are the same with and without it (the golden's gradients are the reference's, noise included).
The seed of a case is the first one from the base seed upward that meets them (SEEDS; the CPU test asserts it)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fisheye_oracle as FO
from oracle import fsnet_oracle as O

FRAME_LISTS = {1: (0, -1), 3: (0, -2, -1, 1), 4: (0, -2, -1, 1, 2)}
SHAPES = {"golden": (64, 64), "ragged": (66, 70)}
B = 2
MIN_DEPTH, MAX_DEPTH = 0.5, 150.0
MAX_SHIFT = 0.42            # px: the largest displacement of a valid ray's sample along an axis
BASE_SEED = 1
MIN_WIN, MAX_TIES, MAX_FRAGILE, MAX_NOISE_SHIFT = 0.01, 0.001, 0.0005, 2.5e-7
# what the reference's noise can reverse: two identity terms closer than the difference of two draws of randn * 1e-5
# (|draw| < 5 sigma among the 2 * 64 * 64 * 4 of a case)
NOISE_GAP = 1e-4

# first seed from BASE_SEED upward that meets check_conditions(), per case (filled by find_seed; asserted on the CPU)
SEEDS = {"golden-n1": 22, "golden-n3": 1, "golden-n4": 1, "ragged-n1": 21, "ragged-n3": 4, "ragged-n4": 2}
# (N = 1 goes furthest: its one warped cell is the widest, and condition 5 asks that none of its pixels at any of the four
# scales has the identity and the warped term within a draw of the noise)

_cases = {}


def case_names():
    return ["%s-n%d" % (k, N) for k in SHAPES for N in (1, 3, 4)]


def calibrations(H, W):
    Ps, calibs = zip(*[FO.synthetic_calib(H, W, b % 2) for b in range(B)])
    return torch.stack(Ps, 0), list(calibs)


def sample_coords(norm, T, P, calib):
    """un-normalised sample coordinates (ix, iy) [B,H,W] of FishEyeDecoder._generate_images_pred for the full-resolution
    ray norm [B,1,H,W] and the transform T, in the oracle's arithmetic; and the ray-table mask [B,H,W]"""
    Bn, _, H, W = norm.shape
    points, lmask = FO.image2cam(norm, P, calib)
    homo = torch.cat([points, torch.ones_like(points[..., :1])], -1).squeeze(1)[..., None]
    tp = torch.matmul(T[:, None, None], homo)[..., 0]
    uv = [FO.cam2image(tp[b, ..., 0:3], P[b], calib[b]) for b in range(Bn)]
    u, v = torch.stack([a for a, _ in uv], 0), torch.stack([a for _, a in uv], 0)
    un, vn = u / max(W - 1, 1) * 2 - 1, v / max(H - 1, 1) * 2 - 1
    return (un + 1) * 0.5 * (W - 1), (vn + 1) * 0.5 * (H - 1), lmask[:, 0]


def cells(H, W, N):
    """[(row, k, y0, y1, x0, x1)]: the 2 x N cells of the middle 56 % of the image (inside the ray-table mask at both shapes)"""
    ya, yb, xa, xb = int(round(0.22 * H)), int(round(0.78 * H)), int(round(0.22 * W)), int(round(0.78 * W))
    ym = (ya + yb) // 2
    out = []
    for k in range(N):
        x0, x1 = xa + (xb - xa) * k // N, xa + (xb - xa) * (k + 1) // N
        out += [(0, k, ya, ym, x0, x1), (1, k, ym, yb, x0, x1)]
    return out


def _texture(rng, H, W):
    """c(b, channel, x, y) for float coordinate arrays [H,W] -> [B,3,H,W]"""
    lam = 3.0 + 3.0 * rng.random((5, B, 3, 1, 1))
    ph = 6.28 * rng.random((5, B, 3, 1, 1))
    k = 2 * np.pi / lam

    def c(x, y):
        x, y = x[:, None], y[:, None]                  # [B,1,H,W]
        return (0.5 + 0.14 * np.sin(k[0] * x + ph[0]) * np.cos(k[1] * y + ph[1]) + 0.10 * np.sin(k[2] * (x + y) + ph[2])
                + 0.08 * np.sin(k[3] * x - k[4] * y + ph[3]))
    return c


def image_from_u8(a):
    return torch.from_numpy(a).float() / 255


def make_case(name, seed=None):
    """-> dict(name, N, fids, H, W, data (the input dict of the loss), depths [4 x [B,1,h,w]], aa / tr {f: [B,1,3]})"""
    shape, nn = name.split("-")
    N = int(nn[1:])
    seed = SEEDS[name] if seed is None else seed
    key = (name, seed)
    if key in _cases:
        return _cases[key]
    H, W = SHAPES[shape]
    fids = FRAME_LISTS[N]
    rng = np.random.default_rng(7919 * seed + 1009 * H + W + 104729 * N)
    g = torch.Generator().manual_seed(1000 * seed + N)
    P, calib = calibrations(H, W)
    depths = []
    for s in range(4):
        h, w = H >> s, W >> s
        ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
        depths.append(8 + 6 * (1 - ys) + 2 * torch.rand(B, 1, h, w, generator=g))
    norm0 = F.interpolate(depths[0], [H, W], mode="bilinear", align_corners=True)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    aa, tr, shift = {}, {}, {}
    for f in fids[1:]:
        a = 0.001 * torch.randn(B, 1, 3, generator=g)
        # |f| = 1: along x, |f| = 2: along the diagonal, towards the side of the frame's sign
        d = torch.tensor([[[1.0, -0.02, 0.05]]]) if abs(f) == 1 else torch.tensor([[[0.75, 0.6, -0.04]]])
        t = (d * (1.0 if f > 0 else -1.0)).repeat(B, 1, 1) * (1 + 0.1 * torch.rand(B, 1, 3, generator=g))
        for b in range(B):                              # scale the translation to MAX_SHIFT on the valid rays
            for _ in range(3):
                T = O.transformation_from_parameters(a, t, invert=(f < 0))
                ix, iy, lm = sample_coords(norm0, T, P, calib)
                big = max(float(((ix - xx).abs() * lm)[b].max()), float(((iy - yy).abs() * lm)[b].max()))
                t[b] *= MAX_SHIFT / big
        aa[f], tr[f] = a, t
        T = O.transformation_from_parameters(a, t, invert=(f < 0))
        ix, iy, lm = sample_coords(norm0, T, P, calib)
        shift[f] = ((ix - xx).numpy().astype(np.float64), (iy - yy).numpy().astype(np.float64))
    c = _texture(rng, H, W)
    X, Y = np.broadcast_to(xx.numpy().astype(np.float64), (B, H, W)), np.broadcast_to(yy.numpy().astype(np.float64), (B, H, W))
    img0 = c(X, Y) + 0.02 * (rng.random((B, 3, H, W)) - 0.5)
    img0 = np.rint(np.clip(img0, 0, 1) * 255) / 255       # (the frames are built around the target as it will be stored)
    srcs = {}
    for k, f in enumerate(fids[1:]):
        im = img0 + 0.024 * k * (rng.random((B, 3, H, W)) - 0.5)
        lined = c(X - shift[f][0], Y - shift[f][1]) + 0.004 * (rng.random((B, 3, H, W)) - 0.5)
        clean = img0
        noisy = img0 + 0.30 * (rng.random((B, 3, H, W)) - 0.5)
        for row, kk, y0, y1, x0, x1 in cells(H, W, N):
            part = noisy if kk != k else (clean if row == 0 else lined)
            im[:, :, y0:y1, x0:x1] = part[:, :, y0:y1, x0:x1]
        srcs[f] = im
    # 8-bit images, as a camera delivers them (and a golden file holds them in a quarter of the bytes)
    srcs[0] = img0
    u8 = {f: np.rint(np.clip(srcs[f], 0, 1) * 255).astype(np.uint8) for f in fids}
    data = {("original_image", f): image_from_u8(u8[f]) for f in fids}
    pm = torch.ones(B, H, W, dtype=torch.float64)
    pm[:, :5, :] = 0
    data["patched_mask"], data["P2"], data["calib_meta"] = pm, P, calib
    case = dict(name=name, N=N, fids=fids, H=H, W=W, data=data, depths=depths, aa=aa, tr=tr, seed=seed, u8=u8)
    _cases[key] = case
    return case


def transforms(case, leaves=False):
    """[T_f] of the case's frames (leaves=True: from aa / tr that require a gradient, returned as well)"""
    Ts, lv = [], []
    for f in case["fids"][1:]:
        a, t = case["aa"][f].clone().requires_grad_(leaves), case["tr"][f].clone().requires_grad_(leaves)
        lv.append((a, t))
        Ts.append(O.transformation_from_parameters(a, t, invert=(f < 0)))
    return (Ts, lv) if leaves else Ts


def oracle_chain(case, noise=None, grads=False, detach_disp=False):
    """FO.photometric_loss on the case -> dict(total, ld, outputs, depths (leaves), pose leaves); detach_disp: the
    smoothness term sends no gradient to the depth (the photometric chain's gradient alone)"""
    outputs = {}
    dl = [d.clone().requires_grad_(grads) for d in case["depths"]]
    for s in range(4):
        outputs[("depth", s, s)] = dl[s]
        disp = O.depth_to_disp(dl[s], MIN_DEPTH, MAX_DEPTH)
        outputs[("disp", s)] = disp.detach() if detach_disp else disp
    Ts, lv = transforms(case, leaves=True) if grads else (transforms(case), None)
    for f, T in zip(case["fids"][1:], Ts):
        outputs[("cam_T_cam", f)] = T
    total, ld = FO.photometric_loss(outputs, case["data"], frame_ids=tuple(case["fids"]), noise=noise)
    if grads:
        total.backward()
    return dict(total=total.detach(), ld=ld, outputs=outputs, depths=dl, poses=lv)


def reference_noise(case):
    """the reference's tie-break noise (:258-259): the first draw after torch.manual_seed(0), one per scale"""
    torch.manual_seed(0)
    return {s: torch.randn(B, case["N"], case["H"], case["W"]) * 0.00001 for s in range(4)}


def candidates(case, res, scale=0):
    """[B,2N,H,W] candidates of the per-pixel minimum at `scale` from an oracle_chain() result (no noise)"""
    data, out = case["data"], res["outputs"]
    tgt = data[("original_image", 0)]
    ident = [O.reprojection_loss(data[("original_image", f)], tgt) for f in case["fids"][1:]]
    rp = []
    for f in case["fids"][1:]:
        pl = O.reprojection_loss(out[("original_image", f, scale)].detach(), tgt)
        rp.append(torch.where(out[("overlapped_mask", f, scale)].unsqueeze(1), pl, torch.full_like(pl, 100.0)))
    return torch.cat(ident + rp, 1)


def gap(cand):
    """difference of the two smallest candidates per pixel [B,H,W]"""
    two = torch.topk(cand, 2, dim=1, largest=False)[0]
    return two[:, 1] - two[:, 0]


def fragile(case, scale=0):
    """[N,B,H,W] bool: overlap-mask cells whose sample coordinate lies within 1e-3 px of a half-integer"""
    H, W = case["H"], case["W"]
    norm = F.interpolate(case["depths"][scale], [H, W], mode="bilinear", align_corners=True)
    out = []
    for T in transforms(case):
        ix, iy, _ = sample_coords(norm, T, case["data"]["P2"], case["data"]["calib_meta"])
        near = lambda v: ((v - torch.floor(v)) - 0.5).abs() < 1e-3
        out.append(near(ix.double()) | near(iy.double()))
    return torch.stack(out)


def measure(case):
    """the measured quantities of check_conditions()"""
    N = case["N"]
    res = oracle_chain(case)
    cand = candidates(case, res)
    am = cand.argmin(1)
    wins = [float((am == k).double().mean()) for k in range(2 * N)]
    ties = float((gap(cand) < 1e-6).double().mean())
    frag = float(fragile(case).double().mean())
    noisy = oracle_chain(case, noise=reference_noise(case))
    flips = 0
    for s in range(4):
        a, b = res["outputs"][("min_idx", s)], noisy["outputs"][("min_idx", s)]
        flips += int((((a >= N) | (b >= N)) & (a != b)).sum())
    return dict(wins=wins, ties=ties, fragile=frag, noise_shift=abs(float(noisy["total"]) - float(res["total"])),
                flips=flips)


def check_conditions(case, m=None):
    m = measure(case) if m is None else m
    bad = []
    for k, w in enumerate(m["wins"]):
        if w < MIN_WIN:
            bad.append("candidate %d wins %.4f of the pixels" % (k, w))
    if m["ties"] > MAX_TIES:
        bad.append("%.5f of the pixels are near-ties" % m["ties"])
    if m["fragile"] > MAX_FRAGILE:
        bad.append("%.5f of the overlap samples are fragile" % m["fragile"])
    if m["noise_shift"] > MAX_NOISE_SHIFT:
        bad.append("the reference's noise moves the total by %.2e" % m["noise_shift"])
    if m["flips"]:
        bad.append("the reference's noise reverses %d selections of a warped term" % m["flips"])
    return bad


def find_seed(name, limit=40):
    for seed in range(BASE_SEED, BASE_SEED + limit):
        if not check_conditions(make_case(name, seed)):
            return seed
    return None
