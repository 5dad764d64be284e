"""The loss prologue's two one-read kernels against what they replace.

fs_photo_identity_rows (row-walking strips of 62 columns x RS rows) is compared with an f64 numpy restatement of
reproj_at() and with fs_photo_identity (the tile kernel, which adds the nine window taps in the reference's order) on
the same inputs: strip seams in x (W around 62 and 124) and in y (H around RS and 2 RS), the degenerate 2- and 3-pixel
sides, B = 1 and 3, with and without a patched mask.  fs_color_pyramid_multi is compared bit for bit with one
fs_color_pyramid launch per level, on the one-launch path and on the per-level fallback.

Accuracy bound: both kernels sum nine fp32 terms per window and run the same unfused arithmetic on the sums (the new
one's quotient and channel means are within 1 ulp of the divisions), so what differs is the order of the nine
additions: on every shape the new kernel's largest absolute error against f64 may be at most twice the tile kernel's
on the same inputs.  Measured (RS = 16), rows / tile on one shape each: the largest rows error 1.934e-6 / 1.577e-6
(B 3, 16 x 63); at B = 1 1.288e-6 / 1.181e-6 (3 x 124); the largest ratio 1.111e-6 / 5.992e-7 = 1.85 (B 1, 2 x 63)."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WS = (2, 3, 61, 62, 63, 124, 125)


def _rs():
    from fsnet_amd.hip import lib
    return int(lib.fs_photo_identity_strip_rows())


def _hs():
    rs = _rs()
    return (2, 3, rs - 1, rs, rs + 1, 2 * rs + 1)


def _f32(v):
    return float(np.float32(v))


def ident_ref(t, x):
    """reproj_at() of photometric.hip in f64: t, x [B,3,H,W] -> [B,H,W]"""
    H, W = t.shape[2:]
    c1, c2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))

    def box(a):
        p = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
        return sum(p[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0

    mux, muy = box(x), box(t)
    sgx, sgy, sgxy = box(x * x) - mux * mux, box(t * t) - muy * muy, box(x * t) - mux * muy
    n = (2.0 * mux * muy + c1) * (2.0 * sgxy + c2)
    d = (mux * mux + muy * muy + c1) * (sgx + sgy + c2)
    ssim = np.clip((1.0 - n / d) * 0.5, 0.0, 1.0).sum(1) / 3.0
    l1 = np.abs(t - x).sum(1) / 3.0
    return _f32(0.85) * ssim + _f32(0.15) * l1


_inputs = {}


def frames(B, H, W):
    """seeded frames in [0, 1] (host f32) + an f64 0/1 mask, made once per shape"""
    key = (B, H, W)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * B + 17 * H + W)
        img = rng.random((3, B, 3, H, W), dtype=np.float32)
        mask = (rng.random((B, H, W)) < 0.7).astype(np.float64)
        ref = np.stack([ident_ref(img[0].astype(np.float64), img[1 + f].astype(np.float64)) for f in range(2)], 1)
        _inputs[key] = (img, mask, ref)
    return _inputs[key]


def run_ident(dev, fn, t, s0, s1, mask):
    """-> (ident [B,2,H,W] f32 numpy, mask_sum [B] f64 numpy)"""
    import torch
    from fsnet_amd.hip.binding import FsPhotoArgs, check, stream_ptr
    B, _, H, W = t.shape
    ident = torch.full((B, 2, H, W), float("nan"), dtype=torch.float32, device=dev)
    msum = torch.zeros(B, dtype=torch.float64, device=dev)
    geo = torch.zeros(B, 48, dtype=torch.float32, device=dev)
    pa = FsPhotoArgs()
    pa.img0, pa.img_src[0], pa.img_src[1] = t.data_ptr(), s0.data_ptr(), s1.data_ptr()
    pa.patched_mask = None if mask is None else mask.data_ptr()
    pa.ident, pa.mask_sum, pa.geo = ident.data_ptr(), msum.data_ptr(), geo.data_ptr()
    pa.B, pa.H, pa.W, pa.S = B, H, W, 1
    check(fn(C.byref(pa), stream_ptr()), "identity")
    torch.cuda.synchronize()
    return ident.cpu().numpy(), msum.cpu().numpy()


def on_dev(dev, img, mask, with_mask):
    import torch
    t, s0, s1 = (torch.from_numpy(img[i]).to(dev).contiguous() for i in range(3))
    m = torch.from_numpy(mask).to(dev).contiguous() if with_mask else None
    return t, s0, s1, m


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B", [1, 3])
def test_identity_rows_vs_f64_and_tile_kernel(dev, B, with_mask):
    from fsnet_amd.hip import lib
    worst_new = worst_old = 0.0
    worst = None
    for H, W in itertools.product(_hs(), WS):
        img, mask, ref = frames(B, H, W)
        t, s0, s1, m = on_dev(dev, img, mask, with_mask)
        new, msum_new = run_ident(dev, lib.fs_photo_identity_rows, t, s0, s1, m)
        old, msum_old = run_ident(dev, lib.fs_photo_identity, t, s0, s1, m)
        assert np.isfinite(new).all(), (H, W)              # every pixel of both planes was written
        e_new, e_old = float(np.abs(new - ref).max()), float(np.abs(old - ref).max())
        print("B %d H %3d W %3d  max |err| vs f64: rows %.3e  tile %.3e" % (B, H, W, e_new, e_old))
        assert e_new <= 2.0 * e_old, (B, H, W, e_new, e_old)
        if e_new > worst_new:
            worst = (H, W, e_new, e_old)
        worst_new, worst_old = max(worst_new, e_new), max(worst_old, e_old)
        want = mask.sum((1, 2)) if with_mask else np.full(B, float(H * W))
        assert np.array_equal(msum_new, want), (H, W, msum_new, want)
        assert np.array_equal(msum_old, want)
    print("largest: rows %.3e at H %d W %d (tile there %.3e); tile kernel's largest %.3e" % (
        worst[2], worst[0], worst[1], worst[3], worst_old))


@pytest.mark.parametrize("B", [1, 3])
def test_identity_rows_identical_frames_give_exact_zero(dev, B):
    from fsnet_amd.hip import lib
    for H, W in itertools.product(_hs(), WS):
        img, mask, _ = frames(B, H, W)
        t, _, s1, _ = on_dev(dev, img, mask, False)
        out, _ = run_ident(dev, lib.fs_photo_identity_rows, t, t.clone(), s1, None)
        assert (out[:, 0] == 0.0).all(), (H, W, float(np.abs(out[:, 0]).max()))
        out, _ = run_ident(dev, lib.fs_photo_identity_rows, t, s1, t, None)
        assert (out[:, 1] == 0.0).all(), (H, W)


def test_identity_rows_is_deterministic(dev):
    from fsnet_amd.hip import lib
    rs = _rs()
    for B, H, W in ((3, 2 * rs + 1, 125), (1, rs, 62), (3, 3, 2)):
        img, mask, _ = frames(B, H, W)
        t, s0, s1, m = on_dev(dev, img, mask, True)
        a, ma = run_ident(dev, lib.fs_photo_identity_rows, t, s0, s1, m)
        b, mb = run_ident(dev, lib.fs_photo_identity_rows, t, s0, s1, m)
        assert np.array_equal(a, b) and np.array_equal(ma, mb)


def test_identity_rows_rejects_bad_arguments(dev):
    import torch
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsPhotoArgs
    assert lib.fs_photo_identity_rows(None, None) == 1
    pa = FsPhotoArgs()
    x = torch.zeros(64, dtype=torch.float64, device=dev)
    pa.img0 = pa.img_src[0] = pa.img_src[1] = pa.geo = pa.ident = pa.mask_sum = x.data_ptr()
    pa.B, pa.H, pa.W, pa.S = 1, 1, 4, 1
    assert lib.fs_photo_identity_rows(C.byref(pa), None) == 1          # H < 2


def pyramid_levels(dev, img, hw, multi):
    import torch
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import check, stream_ptr
    B, _, H, W = img.shape
    outs = [torch.full((B, 3, h, w), float("nan"), dtype=torch.float32, device=dev) for h, w in hw]
    if multi:
        n = len(hw)
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        hs, ws = (C.c_int32 * n)(*[h for h, _ in hw]), (C.c_int32 * n)(*[w for _, w in hw])
        check(lib.fs_color_pyramid_multi(img.data_ptr(), ptrs, hs, ws, n, B, H, W, stream_ptr()), "pyramid_multi")
    else:
        for o, (h, w) in zip(outs, hw):
            check(lib.fs_color_pyramid(img.data_ptr(), o.data_ptr(), B, H, W, h, w, stream_ptr()), "pyramid")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("H,W,hw", [
    (64, 128, None), (8, 8, None),                       # scales {0, 1, 2, 3}: the one-launch kernel
    (64, 128, [(8, 16), (32, 64), (16, 32)]),            # the same levels in another order
    (36, 60, [(18, 30), (9, 15), (12, 20)]),             # sides not divisible by 8, a ratio of 3: per-level kernel
    (64, 128, [(32, 64), (16, 32)]),                     # two levels: per-level kernel
], ids=["64x128", "8x8", "64x128-reordered", "36x60-fallback", "two-level-fallback"])
def test_color_pyramid_multi_matches_per_level_kernel(dev, H, W, hw):
    import torch
    B = 2
    hw = hw or [(H >> s, W >> s) for s in (1, 2, 3)]
    rng = np.random.default_rng(H * 1000 + W)
    img = torch.from_numpy(rng.random((B, 3, H, W), dtype=np.float32)).to(dev)
    got = pyramid_levels(dev, img, hw, True)
    want = pyramid_levels(dev, img, hw, False)
    ref = img.cpu().numpy().astype(np.float64)
    for g, w_, (h, w) in zip(got, want, hw):
        assert np.array_equal(g, w_), (h, w)
        mean = ref.reshape(B, 3, h, H // h, w, W // w).mean((3, 5))
        n = (H // h) * (W // w)                  # n - 1 fp32 additions of partial sums <= n, one division: in units of the mean
        assert np.abs(g - mean).max() <= n * 2.0 ** -24


def test_color_pyramid_multi_rejects_bad_arguments(dev):
    import torch
    from fsnet_amd.hip import lib
    x = torch.zeros(3 * 8 * 8, dtype=torch.float32, device=dev)
    ptrs, hs, ws = (C.c_void_p * 1)(x.data_ptr()), (C.c_int32 * 1)(3), (C.c_int32 * 1)(4)
    assert lib.fs_color_pyramid_multi(None, ptrs, hs, ws, 1, 1, 8, 8, None) == 1
    assert lib.fs_color_pyramid_multi(x.data_ptr(), ptrs, hs, ws, 1, 1, 8, 8, None) == 1      # 8 % 3 != 0
    assert lib.fs_color_pyramid_multi(x.data_ptr(), ptrs, hs, ws, 5, 1, 8, 8, None) == 1
