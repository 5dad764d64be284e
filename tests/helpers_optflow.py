"""CPU restatement of the motion-mask precompute (fsnet_amd/csrc/optflow.hip) — TEST INFRASTRUCTURE ONLY.

* Dense Farneback flow, OpenCV 4.x optflowgf.cpp (calcOpticalFlowFarneback, FarnebackPolyExp,
  FarnebackUpdateMatrices, FarnebackUpdateFlow_Blur / _GaussianBlur) as read from its published source, in numpy fp32
  (f64 where OpenCV accumulates in double).  OpenCV is not installed here, so parity with cv2 itself is UNPINNED; the
  kernel is pinned to this restatement.  Choices where the restatement fixes what OpenCV leaves to its SIMD paths:
  the separable blurs are k0 * c + sum_i k_i * (lo_i + hi_i) in fp32 (horizontal, then vertical); the box window is
  a direct f64 sum (rows -m..m, then columns -m..m) instead of OpenCV's running sum; the 6x6 moment matrix is inverted
  in closed form; the flow of the coarser level is scaled by (float)(1 / pyr_scale).
* The epipolar block of the reference's hooks (base_precompute_hooks.py:58-89, :109-148), in torch as written there.
* A corridor scene (tests/helpers_scene.corridor_batch) with one independently moving box, the exact rigid flow of
  the corridor and the box's pixels.
"""
import numpy as np
import torch

F32 = np.float32
MIN_SIZE = 32
GAUSSIAN = 256
BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], F32)
# the parameters of tools/bench_motion_mask.py (a typical flow_estimator_cfg of the reference's hook)
FLOW_CFG = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)


def gray(img):
    """uint8 [H,W,3] -> fp32 [H,W]: cv2.cvtColor(COLOR_BGR2GRAY) with channel 0 as blue"""
    c = img.astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(F32)


def pyramid_plan(H, W, pyr_scale, levels):
    """[(k, h, w, ksize, sigma)] from the coarsest level down to 0 (k stops at the first level whose size would fall
    under 32 px)"""
    scale = 1.0
    k = 0
    while k < levels:
        scale *= pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    out = []
    for lv in range(k, -1, -1):
        s = 1.0
        for _ in range(lv):
            s *= pyr_scale
        sigma = (1.0 / s - 1.0) * 0.5
        ksize = max(int(np.rint(sigma * 5)) | 1, 3)
        out.append((lv, int(np.rint(H * s)), int(np.rint(W * s)), ksize, sigma))
    return out


def blur_weights(ksize, sigma):
    """cv::getGaussianKernel(ksize, sigma, CV_32F): centre and one half [k0 .. kr]"""
    sx = sigma if sigma > 0 else ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8
    s2 = -0.5 / (sx * sx)
    cf = []
    for i in range(ksize):
        x = i - (ksize - 1) * 0.5
        t = (0.5 if i == 1 else 0.25) if (sigma <= 0 and ksize == 3) else np.exp(s2 * x * x)
        cf.append(F32(t))
    total = 0.0
    for c in cf:
        total += float(c)
    total = 1.0 / total
    r = ksize // 2
    return [F32(float(cf[r + i]) * total) for i in range(r + 1)]


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    while np.any((i < 0) | (i >= n)):
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return i


def blur_h(img, k):
    H, W = img.shape
    x = np.arange(W)
    s = img * k[0]
    for t in range(1, len(k)):
        s = s + k[t] * (img[:, reflect101(x - t, W)] + img[:, reflect101(x + t, W)])
    return s.astype(F32)


def blur_v(img, k):
    H, W = img.shape
    y = np.arange(H)
    s = img * k[0]
    for t in range(1, len(k)):
        s = s + k[t] * (img[reflect101(y - t, H)] + img[reflect101(y + t, H)])
    return s.astype(F32)


def _lin_coords(n_dst, n_src):
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    lo, hi = s < 0, s >= n_src - 1
    f = np.where(lo | hi, F32(0), f).astype(F32)
    s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    return s, f


def resize_linear(src, w, h):
    """cv2.resize INTER_LINEAR of fp32 [H,W] or [H,W,C] (horizontal weights, then vertical)"""
    H, W = src.shape[:2]
    x0, fx = _lin_coords(w, W)
    y0, fy = _lin_coords(h, H)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    one = F32(1)
    fxe, fye = (fx[None, :, None], fy[:, None, None]) if src.ndim > 2 else (fx[None, :], fy[:, None])
    top = src[y0][:, x0] * (one - fxe) + src[y0][:, x1] * fxe
    bot = src[y1][:, x0] * (one - fxe) + src[y1][:, x1] * fxe
    return (top * (one - fye) + bot * fye).astype(F32)


def level_image(g, h, w, ksize, sigma):
    """the level's image: Gaussian blur of the full-resolution gray (REFLECT_101), INTER_LINEAR resize"""
    k = blur_weights(ksize, sigma)
    return resize_linear(blur_v(blur_h(g, k), k), w, h)


def poly_weights(n, sigma):
    if sigma < 1.1920928955078125e-07:
        sigma = n * 0.3
    g = np.array([F32(np.exp(-x * x / (2 * sigma * sigma))) for x in range(-n, n + 1)], F32)
    s = 0.0
    for v in g:
        s += float(v)
    s = 1.0 / s
    g = np.array([F32(float(v) * s) for v in g], F32)
    G00 = G11 = G33 = G55 = 0.0
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            gg = float(g[y + n]) * float(g[x + n])
            G00 += gg
            G11 += gg * x * x
            G33 += gg * x * x * x * x
            G55 += gg * x * x * y * y
    a, b, c, d = G00, G11, G33, G55
    D = a * (c + d) - 2 * b * b
    xs = np.arange(0, n + 1)
    gh = g[n:]
    return dict(g=gh, xg=(xs.astype(F32) * gh).astype(F32), xxg=((xs * xs).astype(F32) * gh).astype(F32),
                ig11=1.0 / b, ig03=-b / D, ig33=(a * c - b * b) / ((c - d) * D), ig55=1.0 / d, n=n)


def poly_exp(img, n, sigma):
    """FarnebackPolyExp: fp32 [h,w] -> R [5,h,w] (r_y, r_x, r_yy, r_xx, r_xy)"""
    p = poly_weights(n, sigma)
    g, xg, xxg = p["g"], p["xg"], p["xxg"]
    h, w = img.shape
    y = np.arange(h)
    r0 = img * g[0]
    r1 = np.zeros_like(img)
    r2 = np.zeros_like(img)
    for k in range(1, n + 1):
        s0, s1 = img[np.maximum(y - k, 0)], img[np.minimum(y + k, h - 1)]
        q = s0 + s1
        r0 = r0 + g[k] * q
        r1 = r1 + xg[k] * (s1 - s0)
        r2 = r2 + xxg[k] * q
    x = np.arange(w)
    b1 = (r0 * g[0]).astype(np.float64)
    b3 = (r1 * g[0]).astype(np.float64)
    b5 = (r2 * g[0]).astype(np.float64)
    b2 = np.zeros(img.shape)
    b4 = np.zeros(img.shape)
    b6 = np.zeros(img.shape)
    for k in range(1, n + 1):
        lo, hi = np.maximum(x - k, 0), np.minimum(x + k, w - 1)
        tg = (r0[:, hi] + r0[:, lo]).astype(np.float64)
        b1 = b1 + tg * float(g[k])
        b4 = b4 + tg * float(xxg[k])
        b2 = b2 + (r0[:, hi] - r0[:, lo]).astype(np.float64) * float(xg[k])
        b3 = b3 + (r1[:, hi] + r1[:, lo]).astype(np.float64) * float(g[k])
        b6 = b6 + (r1[:, hi] - r1[:, lo]).astype(np.float64) * float(xg[k])
        b5 = b5 + (r2[:, hi] + r2[:, lo]).astype(np.float64) * float(g[k])
    return np.stack([b3 * p["ig11"], b2 * p["ig11"], b1 * p["ig03"] + b5 * p["ig33"], b1 * p["ig03"] + b4 * p["ig33"],
                     b6 * p["ig55"]]).astype(F32)


def update_matrices(R0, R1, flow):
    """FarnebackUpdateMatrices: -> M [5,h,w]"""
    _, h, w = R0.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy = x.astype(F32) + dx, y.astype(F32) + dy
    x1, y1 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    fx, fy = (fx - x1.astype(F32)).astype(F32), (fy - y1.astype(F32)).astype(F32)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xc, yc = np.clip(x1, 0, w - 2), np.clip(y1, 0, h - 2)
    one = F32(1)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    r = [a00 * R1[c][yc, xc] + a01 * R1[c][yc, xc + 1] + a10 * R1[c][yc + 1, xc] + a11 * R1[c][yc + 1, xc + 1]
         for c in range(5)]
    half, quarter = F32(0.5), F32(0.25)
    r2 = np.where(inside, r[0], F32(0))
    r3 = np.where(inside, r[1], F32(0))
    r4 = np.where(inside, (R0[2] + r[2]) * half, R0[2])
    r5 = np.where(inside, (R0[3] + r[3]) * half, R0[3])
    r6 = np.where(inside, (R0[4] + r[4]) * quarter, R0[4] * half)
    r2 = (R0[0] - r2) * half
    r3 = (R0[1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    edge = (x < 5) | (x >= w - 5) | (y < 5) | (y >= h - 5)
    # the kernel's product order: bx_lo * bx_hi * by_lo * by_hi
    blo_x = np.where(x < 5, BORDER[np.clip(x, 0, 4)], F32(1)).astype(F32)
    bhi_x = np.where(x >= w - 5, BORDER[np.clip(w - x - 1, 0, 4)], F32(1)).astype(F32)
    blo_y = np.where(y < 5, BORDER[np.clip(y, 0, 4)], F32(1)).astype(F32)
    bhi_y = np.where(y >= h - 5, BORDER[np.clip(h - y - 1, 0, 4)], F32(1)).astype(F32)
    s = np.where(edge, blo_x * bhi_x * blo_y * bhi_y, F32(1)).astype(F32)
    r2, r3, r4, r5, r6 = (np.where(edge, v * s, v) for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3,
                     r6 * r2 + r5 * r3]).astype(F32)


def window_weights(winsize):
    m = winsize // 2
    sigma = m * 0.3
    s = 1.0
    k = [F32(1.0)]
    for i in range(1, m + 1):
        t = F32(np.exp(-i * i / (2 * sigma * sigma)))
        k.append(t)
        s += float(t * F32(2))
    s = 1.0 / s
    return [F32(float(v) * s) for v in k]


def window_solve(M, winsize, flags):
    """FarnebackUpdateFlow_Blur / _GaussianBlur (window sum + 2x2 solve) -> flow [h,w,2]"""
    _, h, w = M.shape
    m = winsize // 2
    y, x = np.arange(h), np.arange(w)
    if flags == GAUSSIAN:
        k = window_weights(winsize)
        v = M * k[0]
        for j in range(1, m + 1):
            v = v + (M[:, np.minimum(y + j, h - 1)] + M[:, np.maximum(y - j, 0)]) * k[j]
        g = v * k[0]
        for j in range(1, m + 1):
            g = g + k[j] * (v[:, :, np.maximum(x - j, 0)] + v[:, :, np.minimum(x + j, w - 1)])
        g = g.astype(np.float64)
    else:
        v = np.zeros(M.shape)
        for j in range(-m, m + 1):
            v = v + M[:, np.clip(y + j, 0, h - 1)].astype(np.float64)
        g = np.zeros(M.shape)
        for j in range(-m, m + 1):
            g = g + v[:, :, np.clip(x + j, 0, w - 1)]
        g = g * (1.0 / (float(winsize) * winsize))
    idet = 1.0 / (g[0] * g[2] - g[1] * g[1] + 1e-3)
    return np.stack([(g[0] * g[4] - g[1] * g[3]) * idet, (g[2] * g[3] - g[1] * g[4]) * idet], -1).astype(F32)


def upsample_flow(flow, w, h, pyr_scale):
    return (resize_linear(flow, w, h) * F32(1.0 / pyr_scale)).astype(F32)


def farneback(img0, img1, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0,
              trace=None):
    """img0 / img1: uint8 [H,W,3] (or fp32/uint8 gray [H,W]) -> flow [H,W,2] fp32.  trace: optional list that receives
    one dict per level (image pair, R pair, the flow entering each iteration and the flow after it)."""
    g0 = gray(img0) if img0.ndim == 3 else img0.astype(F32)
    g1 = gray(img1) if img1.ndim == 3 else img1.astype(F32)
    H, W = g0.shape
    flow = None
    for lv, h, w, ksize, sigma in pyramid_plan(H, W, pyr_scale, levels):
        sg = 0.0 if lv == 0 else sigma
        I0, I1 = level_image(g0, h, w, ksize, sg), level_image(g1, h, w, ksize, sg)
        R0, R1 = poly_exp(I0, poly_n, poly_sigma), poly_exp(I1, poly_n, poly_sigma)
        flow = np.zeros((h, w, 2), F32) if flow is None else upsample_flow(flow, w, h, pyr_scale)
        rec = dict(level=lv, I=(I0, I1), R=(R0, R1), flows=[flow])
        for _ in range(iterations):
            flow = window_solve(update_matrices(R0, R1, flow), winsize, flags)
            rec["flows"].append(flow)
        if trace is not None:
            trace.append(rec)
    return flow


# ------------------------------------------------------------------------------------------------
# the reference's epipolar block (base_precompute_hooks.py:58-89 / :109-148), torch on the CPU
# ------------------------------------------------------------------------------------------------
def skew(T):
    return np.array([[0, -T[2], T[1]], [T[2], 0, -T[0]], [-T[1], T[0], 0]])


def epipolar_distance(flow, P2, relative_pose):
    """flow [H,W,2] -> signed distance d [H,W] fp32, exactly the reference's torch code"""
    H, W, _ = flow.shape
    flow = torch.from_numpy(np.asarray(flow)).float()
    grid_y, grid_x = torch.meshgrid(torch.arange(0, H), torch.arange(0, W), indexing="ij")
    grid = torch.stack([grid_x, grid_y], dim=-1)
    flowed_grid = grid + flow
    R, T = relative_pose[0:3, 0:3], relative_pose[0:3, 3]
    K_1 = np.linalg.inv(P2[0:3, 0:3])
    Fm = torch.from_numpy(np.transpose(K_1) @ skew(T) @ R @ K_1).float()
    homo_grid = torch.cat([grid, torch.ones([H, W, 1])], dim=-1)
    homo_flowed_grid = torch.cat([flowed_grid, torch.ones([H, W, 1])], dim=-1)
    corr = (Fm @ homo_grid.reshape(-1, 3).transpose(1, 0)).transpose(1, 0).reshape(H, W, -1)
    den = torch.norm(corr[..., 0:2], dim=-1)
    return torch.sum(homo_flowed_grid * (corr / den[..., None]), dim=-1)


def motion_mask(flow, P2, relative_pose, threshold=5.0, mode=0):
    d = epipolar_distance(flow, P2, relative_pose)
    if mode == 0:
        return (torch.abs(d) > threshold).numpy().astype(np.uint8)
    norm = torch.norm(torch.from_numpy(np.asarray(flow)).float(), dim=-1)
    return ((torch.abs(d) / norm) > threshold).numpy().astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def to_u8(img):
    """[3,H,W] in 0..1 -> uint8 [H,W,3]"""
    return (img.permute(1, 2, 0).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).numpy()


def rigid_flow(depth, P2, T):
    """exact flow of frame 0 -> frame 1 for depth [H,W] (camera z), intrinsics P2 [3,4], pose T [4,4] (cam 0 -> 1)"""
    H, W = depth.shape
    K = np.asarray(P2, np.float64)[:, :3]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.linalg.inv(K) @ np.stack([x.ravel(), y.ravel(), np.ones(H * W)])
    X = ray * np.asarray(depth, np.float64).ravel()[None]
    T = np.asarray(T, np.float64)
    X1 = T[:3, :3] @ X + T[:3, 3:4]
    p = K @ X1
    u, v = p[0] / p[2], p[1] / p[2]
    return np.stack([u.reshape(H, W) - x, v.reshape(H, W) - y], -1).astype(F32)


def corridor_pair(H, W, seed=0, step=0.25):
    """(img0 u8, img1 u8, P2 [3,4] f64, T [4,4] f64, rigid flow [H,W,2]) of helpers_scene's corridor, the second
    camera `step` of the way to the corridor's next frame (a whole frame moves the side walls by up to W / 6 px)"""
    from tests import helpers_scene as HS
    batch, truth = HS.corridor_batch(1, H, W, seed=seed, frame_ids=(0, step))
    P2 = batch["P2"][0].double().numpy()
    T = truth[("T", step)][0].double().numpy()
    img0, img1 = to_u8(batch[("original_image", 0)][0]), to_u8(batch[("original_image", step)][0])
    return img0, img1, P2, T, rigid_flow(truth["depth"][0, 0].numpy(), P2, T)


def moving_box_pair(H, W, seed=0, box=(0.35, 0.08, 0.3, 0.18), shift=8):
    """corridor_pair with one textured box that moves `shift` px down between the frames (off the epipolar
    direction, which is near-horizontal at the box's place left of the image centre).  box = (top, left, height,
    width) as fractions.  -> (img0, img1, P2, T, rigid flow, box mask of frame 0 (bool), region near the box (bool):
    both box positions dilated by 6 px, which occlusion makes neither box nor rigid background)"""
    img0, img1, P2, T, flow = corridor_pair(H, W, seed)
    rng = np.random.RandomState(seed + 101)
    by, bx, bh, bw = int(box[0] * H), int(box[1] * W), int(box[2] * H), int(box[3] * W)
    coarse = rng.randint(0, 256, size=(bh // 4 + 1, bw // 4 + 1, 3)).astype(np.float64)
    tex = np.kron(coarse, np.ones((4, 4, 1)))[:bh, :bw]
    fine = rng.randint(-30, 31, size=(bh, bw, 3))
    patch = np.clip(tex + fine, 0, 255).astype(np.uint8)
    img0 = img0.copy()
    img1 = img1.copy()
    img0[by:by + bh, bx:bx + bw] = patch
    img1[by + shift:by + shift + bh, bx:bx + bw] = patch
    inbox = np.zeros((H, W), bool)
    inbox[by:by + bh, bx:bx + bw] = True
    near = np.zeros((H, W), bool)
    near[max(by - 6, 0):by + shift + bh + 6, max(bx - 6, 0):bx + bw + 6] = True
    flow = flow.copy()
    flow[inbox] = (0.0, float(shift))
    return img0, img1, P2, T, flow, inbox, near


def workspace_views(ws, B, H, W):
    """the planes fs_optflow_farneback leaves in its workspace (the layout of optflow.hip make_plan), all of the
    finest level after a call: gray [B,2,H,W], tmp (horizontal blur) [B,2,H,W], img [B,2,H,W], R [B,2,5,H,W],
    M [B,5,H,W], flow buffers f0 / f1 [B,H,W,2]"""
    HW = H * W
    out, o = {}, 0
    for name, n, shape in (("gray", 2 * B * HW, (B, 2, H, W)), ("tmp", 2 * B * HW, (B, 2, H, W)),
                           ("img", 2 * B * HW, (B, 2, H, W)), ("R", 10 * B * HW, (B, 2, 5, H, W)),
                           ("M", 5 * B * HW, (B, 5, H, W)), ("f0", 2 * B * HW, (B, H, W, 2)),
                           ("f1", 2 * B * HW, (B, H, W, 2))):
        out[name] = ws[o:o + 4 * n].view(torch.float32).view(shape)
        o = (o + 4 * n + 255) & ~255
    return out


def write_flow_pngs(root, n, H, W, seed=4, spread=300):
    """n seeded 16-bit flow PNGs `{i:08d}.png` (values 2^15 +- spread, i.e. +-spread/64 px) for the ARFlow hook"""
    import os
    from fsnet_amd.monodepth.data.datasets.utils import write_png16
    os.makedirs(root, exist_ok=True)
    rng = np.random.RandomState(seed)
    for i in range(n):
        write_png16(os.path.join(root, "%08d.png" % i), rng.randint(2 ** 15 - spread, 2 ** 15 + spread, size=(H, W, 3)))


def raw_dataset_cfg(raw, split, prefix, **kw):
    """KittiDepthMonoDataset config whose samples keep the frames as the raw uint8 arrays the hooks read (EmptyAug)"""
    return dict(name=prefix + 'monodepth.data.datasets.mono_dataset.KittiDepthMonoDataset', raw_path=raw,
                split_file=split, frame_idxs=[0, 1, -1], is_filter_static=True,
                augmentation=dict(name=prefix + 'vision_base.data.augmentations.augmentations.EmptyAug'), **kw)


# the golden case of tools/gen_golden.py::gen_motion_mask (tests/golden/motion_mask.npz)
GOLDEN_HW = (96, 320)
GOLDEN_TREE_SEED = 11
GOLDEN_FLOW_CFG = dict(pyr_scale=0.5, levels=3, winsize=9, iterations=3, poly_n=5, poly_sigma=1.1, flags=0)
GOLDEN_FLOW_CFG_G = dict(GOLDEN_FLOW_CFG, poly_n=7, poly_sigma=1.5, flags=GAUSSIAN)
GOLDEN_THR = (5.0, 0.9)
