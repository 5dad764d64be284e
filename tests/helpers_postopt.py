"""CPU restatement of the sparse-VO depth post-optimisation (monodepth/networks/utils/postopt_utils.py:104-226) in
torch, written from the reference's semantics: denorm -> Lab -> SLIC over (Lab, x, y, depth) -> VO point selection ->
per-segment log-scale targets -> the smoothness-coupled linear system -> per-segment log shift.  Vectorised (no
per-segment Python loop) and chunked over centres, so 320x1024 runs in seconds.

Pins the reference's choices where it has them (fp32 distances summed Lab + depth + image, first index on ties,
divisor count + 1e-4 in fp32, empty centres moving to 0, the early stop on equal P-means) and the project's where it
has none (top-k ties: lowest pixel index first).  Sums are formed in float64 and rounded once (the reference sums in
fp32, the device exactly in fixed point); the system is solved in float64."""
import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
HOOK_DEFAULTS = dict(lab_dist_weight=1, depth_dist_weight=1, image_dist_weight=1, h_seg=10, w_seg=18, iter_num=3,
                     lambda0=0.54 / (10 * 18), lambda1=1.0, lambda2=0.4)
FUNCTION_DEFAULTS = dict(lab_dist_weight=1, depth_dist_weight=1, image_dist_weight=1, iter_num=5, lambda0=0.0,
                         lambda1=1.0, lambda2=0.001)

_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
_WHITE = (0.95047, 1.0, 1.08883)


def denorm(image_chw, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[3,H,W] float32 normalised -> [H,W,3] uint8 (float64 arithmetic, truncating cast; postopt_utils.py:8-11)"""
    img = np.asarray(image_chw, np.float32).transpose(1, 2, 0)
    v = np.clip((img * np.asarray(std, np.float64) + np.asarray(mean, np.float64)) * 255, 0, 255)
    return np.array(v, dtype=np.uint8)


def rgb2lab(u8):
    """skimage.color.rgb2lab restated from its published constants (sRGB, D65 / 2 degrees), float64"""
    c = np.asarray(u8).astype(np.float64) / 255.0
    c = np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    xyz = [(r * _M[i, 0] + g * _M[i, 1] + b * _M[i, 2]) / _WHITE[i] for i in range(3)]
    fx, fy, fz = [np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0) for t in xyz]
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=-1)


def centre_table(h_seg, w_seg):
    """[K,2] float32 grid_sample coordinates; K from numpy's arange (component 0 = the h-range, read as x)"""
    c = np.stack(np.meshgrid(np.arange(-1, 1.0, 2.0 / h_seg), np.arange(-1, 1.0, 2.0 / w_seg), indexing='ij'),
                 axis=-1).reshape(-1, 2)
    return c.astype(np.float32)


def _round_means(sums64, count):
    return sums64.float() / (count.float() + 1e-4)


def slic(lab, depth, h_seg, w_seg, lab_dist_weight=1, iter_num=5, depth_dist_weight=1, image_dist_weight=1,
         chunk=32):
    """lab [H,W,3] float32, depth [H,W] float32.  Returns (labels [H,W] int64 centre index, P-means [K,3],
    counts [K], iterations run)"""
    H, W = depth.shape
    lab_t = torch.as_tensor(lab, dtype=torch.float32).permute(2, 0, 1).contiguous()          # [3,H,W]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    P = torch.stack([xs, ys, torch.as_tensor(depth, dtype=torch.float32)])                   # [3,H,W]
    grid = torch.from_numpy(centre_table(h_seg, w_seg)).reshape(1, -1, 1, 2)
    K = grid.shape[1]
    c_lab = torch.nn.functional.grid_sample(lab_t[None], grid, align_corners=True)[0, :, :, 0].t().contiguous()
    c_p = torch.nn.functional.grid_sample(P[None], grid, align_corners=True)[0, :, :, 0].t().contiguous()  # [K,3]
    labf = lab_t.reshape(3, -1).t()        # [N,3]
    Pf = P.reshape(3, -1).t()
    lw, dw, iw = float(lab_dist_weight), float(depth_dist_weight), float(image_dist_weight)
    labels = None
    its = 0
    for _ in range(iter_num):
        best = torch.full((H * W,), float('inf'))
        arg = torch.zeros(H * W, dtype=torch.int64)
        for k0 in range(0, K, chunk):
            cl, cp = c_lab[k0:k0 + chunk], c_p[k0:k0 + chunk]
            d = labf[None] - cl[:, None]                                          # [k,N,3]
            rgb = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
            dp = Pf[None] - cp[:, None]
            img = torch.sqrt(dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1])
            tot = rgb * lw + torch.abs(dp[..., 2]) * dw + img * iw                 # [k,N]
            v, i = torch.min(tot, dim=0)                                          # first index on ties
            better = v < best
            best = torch.where(better, v, best)
            arg = torch.where(better, i + k0, arg)
        labels = arg
        its += 1
        cnt = torch.bincount(labels, minlength=K)
        s_lab = torch.zeros(K, 3, dtype=torch.float64).index_add_(0, labels, labf.double())
        s_p = torch.zeros(K, 3, dtype=torch.float64).index_add_(0, labels, Pf.double())
        c_lab = _round_means(s_lab, cnt[:, None])
        new_p = _round_means(s_p, cnt[:, None])
        if torch.equal(new_p, c_p):
            break
        c_p = new_p
    return labels.reshape(H, W), c_p, cnt, its


def select_vo(lp, lv, max_points):
    """VO mask (postopt_utils.py:156-168); top-k over all pixels, ties at the threshold: lowest pixel index first"""
    lpf, lvf = lp.reshape(-1), lv.reshape(-1)
    valid = (lvf < np.float32(np.log(80))) & (lvf > np.float32(np.log(3)))
    if int(valid.sum()) < max_points:
        return valid.reshape(lp.shape)
    diff = (lpf - lvf).abs()
    order = np.argsort(diff.numpy(), kind='stable')[:max_points]
    top = torch.zeros_like(valid)
    top[torch.from_numpy(order)] = True
    return (valid & top).reshape(lp.shape)


def post_optimize(image, depth, vo, h_seg, w_seg, lab_dist_weight=1, iter_num=5, depth_dist_weight=1,
                  image_dist_weight=1, lambda0=0.0, lambda1=1.0, lambda2=0.001, max_points=800,
                  rgb_mean=IMAGENET_MEAN, rgb_std=IMAGENET_STD, details=False):
    """one image: image [3,H,W] normalised, depth [H,W] > 0, vo [H,W] (numpy or CPU tensors) -> refined [H,W]
    float32 (and, with details, labels compacted to the non-empty segments, centres [n,2], the empty-slot count)"""
    image = np.asarray(image, np.float32)
    depth = torch.as_tensor(np.asarray(depth, np.float32))
    vo = torch.as_tensor(np.asarray(vo, np.float32))
    lab = rgb2lab(denorm(image, rgb_mean, rgb_std)).astype(np.float32)
    labels, c_p, cnt, its = slic(lab, depth, h_seg, w_seg, lab_dist_weight, iter_num, depth_dist_weight,
                                 image_dist_weight)
    K = cnt.shape[0]
    lp, lv = torch.log(depth), torch.log(vo)
    sel = select_vo(lp, lv, max_points).reshape(-1)
    nonempty = cnt > 0
    ids = torch.nonzero(nonempty)[:, 0]
    remap = torch.full((K,), -1, dtype=torch.int64)
    remap[ids] = torch.arange(ids.numel())
    seg = remap[labels.reshape(-1)]
    n = ids.numel()
    lpf, lvf = lp.reshape(-1), lv.reshape(-1)
    cnt_s = torch.bincount(seg, minlength=n)
    base = (torch.zeros(n, dtype=torch.float64).index_add_(0, seg, lpf.double()).float() / cnt_s.float())
    mcnt = torch.bincount(seg[sel], minlength=n)
    dsum = torch.zeros(n, dtype=torch.float64).index_add_(0, seg[sel], (lvf - lpf)[sel].double()).float()
    m = mcnt > 0
    target = torch.where(m, dsum / mcnt.clamp(min=1).float() + base, torch.ones(n))
    centres = c_p[ids, 0:2]                                                     # [n,2] (cx, cy)
    cd = torch.sqrt(((centres[None, :, :] - centres[:, None, :]) ** 2).sum(-1))
    w = torch.exp(-cd / 20)                                                     # fp32 like the reference
    wd = w.double()
    s = wd.sum(-1)
    l0, l1, l2 = float(lambda0), float(lambda1), float(lambda2)
    mf = m.double()
    A = torch.diag(l0 * s + l1 * mf + l2) - l0 * wd
    bd = base.double()
    rhs = l2 * bd + l1 * mf * target.double() + l0 * ((bd[:, None] - bd[None, :]) * wd).sum(-1)
    x = torch.linalg.solve(A, rhs)
    shift = x.float() - base
    out = torch.exp(lpf + shift[seg]).reshape(depth.shape)
    if not details:
        return out
    return out, seg.reshape(depth.shape).to(torch.int32), centres, int(K - n), its


def synthetic_scene(H, W, seed, n_regions=24, vo_frac=0.02, noise=6.0, vo_noise=0.0):
    """piecewise-planar scene: Voronoi regions, each with its own colour and depth plane (3..60 m).  Returns
    (image [3,H,W] normalised float32, true depth, prediction = true depth x a per-region scale error of +-20..40 %,
    vo = true depth (x (1 + vo_noise * N(0,1))) at ~vo_frac of the pixels and 120 elsewhere — read_sparse_vo's marker
    for no point).  Without VO noise |log pred - log vo| is constant per region: top-k ties everywhere."""
    rng = np.random.RandomState(seed)
    sy, sx = rng.rand(n_regions) * H, rng.rand(n_regions) * W
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    reg = np.argmin((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2, axis=-1)
    colour = rng.randint(20, 236, size=(n_regions, 3)).astype(np.float64)
    u8 = np.clip(colour[reg] + rng.randn(H, W, 3) * noise, 0, 255).astype(np.uint8)
    mean, std = np.array(IMAGENET_MEAN, np.float32), np.array(IMAGENET_STD, np.float32)
    image = ((u8.astype(np.float32) / 255.0 - mean) / std).transpose(2, 0, 1).astype(np.float32)
    d0 = rng.uniform(5, 40, n_regions)
    gx, gy = rng.uniform(-0.02, 0.02, n_regions), rng.uniform(-0.05, 0.05, n_regions)
    true = np.clip(d0[reg] + gx[reg] * (xx - sx[reg]) + gy[reg] * (yy - sy[reg]), 3.5, 60.0).astype(np.float32)
    scale = 1 + rng.uniform(0.2, 0.4, n_regions) * rng.choice([-1.0, 1.0], n_regions)
    pred = (true * scale[reg]).astype(np.float32)
    vo = np.full((H, W), 120.0, np.float32)
    pick = rng.rand(H, W) < vo_frac
    vo[pick] = (true * (1 + vo_noise * rng.randn(H, W)))[pick]
    return np.ascontiguousarray(image), true, pred, vo
