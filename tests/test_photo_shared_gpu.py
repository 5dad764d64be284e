"""One kernel text under two frame-count policies gives equal bits: the identity rows, the setup and the pose gradient
of photometric.hip serve fs_photo_* (two sources) and fs_photo_multi_* (one to four), and the file compiles with
contraction off, so the results are compared with torch.equal — no tolerance.  (The fused forward and backward are not
asked to agree bit for bit across their instantiations: they allow FMAs, which the compiler may place differently; their
yardstick stays the float64 chains of test_photo_fused_seams_gpu.py and test_photo_multi_gpu.py.)

The two image sizes cross one and two strip seams in both directions (strips of 62 columns x 16 rows)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, dtype=torch.float32)


def _ident_two(dev, t, s0, s1, mask):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsPhotoArgs, check, stream_ptr
    B, _, H, W = t.shape
    ident = torch.full((B, 2, H, W), NAN, dtype=torch.float32, device=dev)
    msum = torch.zeros(B, dtype=torch.float64, device=dev)
    geo = torch.zeros(B, 48, dtype=torch.float32, device=dev)
    pa = FsPhotoArgs()
    pa.img0, pa.img_src[0], pa.img_src[1] = t.data_ptr(), s0.data_ptr(), s1.data_ptr()
    pa.patched_mask = mask.data_ptr()
    pa.ident, pa.mask_sum, pa.geo = ident.data_ptr(), msum.data_ptr(), geo.data_ptr()
    pa.B, pa.H, pa.W, pa.S = B, H, W, 1
    check(lib.fs_photo_identity_rows(C.byref(pa), stream_ptr()), "identity_rows")
    torch.cuda.synchronize()
    return ident.cpu(), msum.cpu()


def _ident_n(dev, t, srcs, mask):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsPhotoMultiArgs, check, stream_ptr
    B, _, H, W = t.shape
    N = len(srcs)
    ident = torch.full((B, N, H, W), NAN, dtype=torch.float32, device=dev)
    msum = torch.zeros(B, dtype=torch.float64, device=dev)
    geo = torch.zeros(B, 18 + 12 * N, dtype=torch.float32, device=dev)
    pa = FsPhotoMultiArgs()
    pa.img0 = t.data_ptr()
    for f in range(N):
        pa.img_src[f] = srcs[f].data_ptr()
    pa.patched_mask = mask.data_ptr()
    pa.ident, pa.mask_sum, pa.geo = ident.data_ptr(), msum.data_ptr(), geo.data_ptr()
    pa.B, pa.H, pa.W, pa.S, pa.nsrc = B, H, W, 1, N
    check(lib.fs_photo_multi_identity(C.byref(pa), stream_ptr()), "multi_identity")
    torch.cuda.synchronize()
    return ident.cpu(), msum.cpu()


@pytest.mark.parametrize("H,W", [(17, 63), (33, 125)])
def test_identity_planes_equal_under_both_policies(dev, H, W):
    B = 2
    gen = torch.Generator().manual_seed(100 * H + W)
    t, s0, s1, s2 = (_rand(gen, B, 3, H, W).to(dev).contiguous() for _ in range(4))
    mask = (_rand(gen, B, H, W) < 0.7).double().to(dev).contiguous()
    assert bool((mask == 0).any()) and bool((mask == 1).any())
    two, msum_two = _ident_two(dev, t, s0, s1, mask)
    assert bool(torch.isfinite(two).all())
    assert torch.equal(msum_two, mask.sum((1, 2)).cpu())
    n2, msum_n2 = _ident_n(dev, t, [s0, s1], mask)
    assert torch.equal(n2, two) and torch.equal(msum_n2, msum_two)
    # N = 3: a full pair and a half-filled one; the mask sum is added once, by the first pair's waves
    n3, msum_n3 = _ident_n(dev, t, [s0, s1, s2], mask)
    third, _ = _ident_two(dev, t, s2, s0, mask)
    assert torch.equal(n3[:, :2], two)
    assert torch.equal(n3[:, 2], third[:, 0])
    assert torch.equal(msum_n3, msum_two)


def _poses(gen, B, n):
    Ts = []
    for _ in range(n):
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, :3, :] += 0.2 * (_rand(gen, B, 3, 4) - 0.5)
        Ts.append(T.contiguous())
    return Ts


def _intrinsics(gen, B, H=192, W=640):
    P2 = torch.zeros(B, 3, 4)
    P2[:, 0, 0] = 0.58 * W * (1 + 0.1 * _rand(gen, B))
    P2[:, 1, 1] = 1.92 * H * (1 + 0.1 * _rand(gen, B))
    P2[:, 0, 2], P2[:, 1, 2], P2[:, 2, 2] = 0.5 * W + _rand(gen, B), 0.5 * H + _rand(gen, B), 1.0
    P2[:, 0, 1] = 0.01 * _rand(gen, B)
    P2[:, :, 3] = _rand(gen, B, 3)          # the fourth column is not read
    return P2.contiguous()


def _setup_two(dev, P2, T0, T1, fisheye=0):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import check, stream_ptr
    B = P2.shape[0]
    geo = torch.full((B, 48), NAN, dtype=torch.float32, device=dev)
    check(lib.fs_photo_setup(P2.data_ptr(), T0.data_ptr(), T1.data_ptr(), geo.data_ptr(), B, None, fisheye, stream_ptr()),
          "setup")
    torch.cuda.synchronize()
    return geo


def _setup_n(dev, P2, Ts):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import check, stream_ptr
    B, N = P2.shape[0], len(Ts)
    geo = torch.full((B, 18 + 12 * N), NAN, dtype=torch.float32, device=dev)
    Tp = (C.c_void_p * 4)(*[T.data_ptr() for T in Ts])
    check(lib.fs_photo_multi_setup(P2.data_ptr(), Tp, N, geo.data_ptr(), B, None, stream_ptr()), "multi_setup")
    torch.cuda.synchronize()
    return geo


def test_setup_equal_under_both_entry_points(dev):
    B = 3
    gen = torch.Generator().manual_seed(7)
    P2 = _intrinsics(gen, B).to(dev)
    Ts = [T.to(dev) for T in _poses(gen, B, 4)]
    two = _setup_two(dev, P2, Ts[0], Ts[1])
    assert bool(torch.isfinite(two[:, :42]).all())
    assert torch.equal(two[:, :42], _setup_n(dev, P2, Ts[:2]))
    four = _setup_n(dev, P2, Ts)
    assert bool(torch.isfinite(four).all())
    assert torch.equal(four[:, :42], two[:, :42])                                   # invK, K, P of (T0, T1)
    assert torch.equal(four[:, 42:66], _setup_two(dev, P2, Ts[2], Ts[3])[:, 18:42])     # P of (T2, T3)
    # the seed counter is bumped once per launch by either entry point
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import check, stream_ptr
    seed = torch.zeros(1, dtype=torch.int32, device=dev)
    geo = torch.zeros(B, 66, dtype=torch.float32, device=dev)
    Tp = (C.c_void_p * 4)(*[T.data_ptr() for T in Ts])
    check(lib.fs_photo_setup(P2.data_ptr(), Ts[0].data_ptr(), Ts[1].data_ptr(), geo.data_ptr(), B, seed.data_ptr(), 0,
                             stream_ptr()), "setup")
    check(lib.fs_photo_multi_setup(P2.data_ptr(), Tp, 4, geo.data_ptr(), B, seed.data_ptr(), stream_ptr()), "multi_setup")
    torch.cuda.synchronize()
    assert int(seed.item()) == 2


def test_setup_fisheye_stores_identity_and_the_transforms(dev):
    B = 3
    gen = torch.Generator().manual_seed(8)
    P2 = _intrinsics(gen, B).to(dev)
    T0, T1 = (T.to(dev) for T in _poses(gen, B, 2))
    geo = _setup_two(dev, P2, T0, T1, fisheye=1)
    eye = torch.eye(3, device=dev).reshape(1, 9).expand(B, 9)
    assert torch.equal(geo[:, 0:9], eye) and torch.equal(geo[:, 9:18], eye)
    assert torch.equal(geo[:, 18:30], T0[:, :3, :].reshape(B, 12))
    assert torch.equal(geo[:, 30:42], T1[:, :3, :].reshape(B, 12))


@pytest.mark.parametrize("S,tiles", [(2, 7), (4, 66)], ids=["rows14", "rows264"])
def test_pose_gradient_equal_under_both_entry_points(dev, S, tiles):
    """S * tiles = 14: fewer rows than the 85 reduction lanes; 264: the benchmark's (192 x 640, four scales)"""
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import check, stream_ptr
    B, N = 3, 4
    gen = torch.Generator().manual_seed(9 + S)
    P2 = _intrinsics(gen, B).to(dev)
    Ts = [T.to(dev) for T in _poses(gen, B, N)]
    geo4 = _setup_n(dev, P2, Ts)
    geo2 = _setup_two(dev, P2, Ts[0], Ts[1])
    dP = (_rand(gen, S, B, tiles, N, 12) - 0.5).to(dev).contiguous()
    dT4 = torch.full((N, B, 4, 4), NAN, dtype=torch.float32, device=dev)
    check(lib.fs_photo_multi_pose_grad(geo4.data_ptr(), dP.data_ptr(), dT4.data_ptr(), N, B, S, tiles, stream_ptr()),
          "multi_pose_grad")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dT4).all())
    assert bool((dT4[:, :, 3, :] == 0).all())
    assert bool((dT4[:, :, :3, :] != 0).any())
    for fa in (0, 2):
        part = dP[:, :, :, fa:fa + 2, :].contiguous()
        d0, d1 = (torch.full((B, 4, 4), NAN, dtype=torch.float32, device=dev) for _ in range(2))
        check(lib.fs_photo_pose_grad(geo2.data_ptr(), part.data_ptr(), d0.data_ptr(), d1.data_ptr(), B, S, tiles,
                                     stream_ptr()), "pose_grad")
        torch.cuda.synchronize()
        assert torch.equal(dT4[fa], d0) and torch.equal(dT4[fa + 1], d1), fa
        assert bool((d0[:, 3, :] == 0).all()) and bool((d1[:, 3, :] == 0).all())
