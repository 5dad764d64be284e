"""The loss tail of the step held against float64 alone: the edge-aware smoothness loss and its gradient (fs_smooth_mean
/ fwd / bwd, directly and through ops.PhotometricLoss), fs_loss_finalize, fs_sumsq, the depth-bin head and the pose tail
— each against the restatement of tests/helpers_loss_tail.py, which test_loss_tail_restatement_cpu.py holds against the
oracle and which also shows the branch every case below takes.

Every element of every output is compared, and every output buffer has a NaN region behind it that must stay NaN.
Two kinds of bound.  Derived ones (sums, finalize, sumsq) are stated at their assert.  Measured ones (d_disp, the head's
depth / disp / dlogits, the pose tail's outputs) are T.bound: 8 x the deviation of the same restatement in torch.float32
on the CPU from float64, + 4 float32 ulps of the largest reference magnitude; bf16 outputs add 2^-8 of the reference
element (one round-to-nearest).  Each such comparison prints its yardstick and the measured deviation (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_loss_tail as T

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FS_EINVAL = 1
PAD = 64


def guarded(n, dtype, dev, fill=None):
    """(the n elements the kernel may write, the whole buffer: PAD NaNs follow them)"""
    full = torch.full((n + PAD,), float("nan"), dtype=dtype, device=dev)
    if fill is not None:
        full[:n] = fill
    return full[:n], full


def intact(*fulls):
    return all(bool(torch.isnan(f[-PAD:]).all()) for f in fulls)


def held(tag, got, ref64, ref32):
    """every element of got within T.bound of the float64 reference (bf16: + 2^-8 of the element)"""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    dev_ = (got.double() - ref64).abs()
    lim = T.bound(ref64, ref32)
    top = float(ref64.abs().max())
    print("%-44s max|ref| %.3e  yardstick %.3e  bound %.3e  measured %.3e%s" % (
        tag, top, T.yardstick(ref64, ref32), lim, float(dev_.max()), "  (+2^-8 |ref|)" if got.dtype == BF16 else ""))
    if got.dtype == BF16:
        lim = lim + 2.0 ** -8 * ref64.abs()
    assert bool((dev_ <= lim).all()), (tag, float(dev_.max()), float(lim if isinstance(lim, float) else lim.max()))


def lib_():
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import stream_ptr
    return lib, stream_ptr


# ---------------------------------------------------------------------------------------------- smoothness, direct
class SmoothRun:
    """FsSmoothArgs over guarded buffers; the accumulators (disp_sum[S*B], sm_sums[2*S*B], dot[S*B]) zeroed here"""

    def __init__(self, dev, B, hw, sids, disps, colors, gout):
        from fsnet_amd.hip.binding import FsSmoothArgs
        S = self.S = len(hw)
        self.B, self.hw = B, hw
        self.sa = sa = FsSmoothArgs()
        self.acc, self.acc_full = guarded(4 * S * B, F64, dev, 0.0)
        self.disp = [d.to(dev).contiguous() for d in disps]
        self.color = [c.float().to(dev).contiguous() for c in colors]
        self.dd = [guarded(B * h * w, F32, dev) for h, w in hw]
        self.gout = None if gout is None else torch.tensor(gout, dtype=F64, device=dev)
        sa.disp_sum = self.acc.data_ptr()
        sa.sm_sums = self.acc[S * B:].data_ptr()
        sa.dot = self.acc[3 * S * B:].data_ptr()
        sa.gout = None if gout is None else self.gout.data_ptr()
        sa.B, sa.S = B, S
        for s, (h, w) in enumerate(hw):
            assert self.disp[s].shape == (B, 1, h, w) and self.color[s].shape == (B, 3, h, w)
            sa.disp[s], sa.color[s], sa.d_disp[s] = self.disp[s].data_ptr(), self.color[s].data_ptr(), self.dd[s][0].data_ptr()
            sa.h[s], sa.w[s], sa.scale_id[s] = h, w, sids[s]

    def call(self, name):
        lib, stream_ptr = lib_()
        return int(getattr(lib, name)(C.byref(self.sa), stream_ptr()))


@pytest.mark.parametrize("gout", [None, 0.37], ids=["gout-none", "gout-0.37"])
@pytest.mark.parametrize("name", [c[0] for c in T.SMOOTH_CASES])
def test_smoothness_direct(dev, name, gout):
    B, hw, sids, disps, colors, const_b = T.smooth_case(name)
    S = len(hw)
    ref = T.smooth_terms(disps, colors, sids, gout, F64)
    ref32 = T.smooth_terms(disps, colors, sids, gout, F32)
    run = SmoothRun(dev, B, hw, sids, disps, colors, gout)
    for entry in ("fs_smooth_mean", "fs_smooth_fwd", "fs_smooth_bwd"):
        assert run.call(entry) == 0, entry
    torch.cuda.synchronize()
    acc = run.acc.cpu()
    disp_sum, sm_sums = acc[:S * B].view(S, B), acc[S * B:3 * S * B].view(S, B, 2)
    for s in range(S):
        # 2^-20 relative: a thread adds at most two float terms before the f64 block sum (h*w <= 2 * 32 * 256), the
        # normalised difference and the product are a few float roundings, expf is within a few ulp
        want = ref[s]["disp_sum"]
        assert bool(((disp_sum[s] - want).abs() <= 2.0 ** -20 * want.abs()).all()), (name, s, "disp_sum")
        for k, key in enumerate(("sx_sum", "sy_sum")):
            want = ref[s][key]
            err = (sm_sums[s, :, k] - want).abs()
            print("smooth %s s%d %s: rel err %.3e (bound %.3e)" % (name, s, key, float((err / want.clamp_min(1e-300)).max()),
                                                                    2.0 ** -20))
            assert bool((err <= 2.0 ** -20 * want.abs()).all()), (name, s, key)
        h, w = hw[s]
        got = run.dd[s][0].view(B, 1, h, w)
        held("d_disp %s s%d %s" % (name, s, "gout" if gout else "none"), got, ref[s]["d_disp"], ref32[s]["d_disp"])
        if const_b is not None:           # pins the (s * B + b) indexing of disp_sum and dot
            assert bool((got[const_b] == 0.0).all())
            assert all(bool((got[b] != 0.0).any()) for b in range(B) if b != const_b)
    assert intact(run.acc_full, *[f for _, f in run.dd])


def test_smoothness_rejects(dev):
    """h = 1, S = 5, a null d_disp[s], a null dot: FS_EINVAL, and nothing is launched (the buffers stay as they were)"""
    B, hw, sids, disps, colors, _ = T.smooth_case("b")

    def fresh():
        return SmoothRun(dev, B, hw, sids, disps, colors, None)
    runs = []
    r = fresh(); r.sa.h[0] = 1; runs.append(r)
    assert [r.call(e) for e in ("fs_smooth_mean", "fs_smooth_fwd", "fs_smooth_bwd")] == [FS_EINVAL] * 3
    r = fresh(); r.sa.S = 5; runs.append(r)
    assert [r.call(e) for e in ("fs_smooth_mean", "fs_smooth_fwd", "fs_smooth_bwd")] == [FS_EINVAL] * 3
    r = fresh(); r.sa.d_disp[0] = None; runs.append(r)
    assert r.call("fs_smooth_bwd") == FS_EINVAL
    r = fresh(); r.sa.dot = None; runs.append(r)
    assert r.call("fs_smooth_bwd") == FS_EINVAL
    torch.cuda.synchronize()
    for r in runs:
        assert bool((r.acc == 0).all()) and bool(torch.isnan(r.dd[0][1]).all())


# ---------------------------------------------------------------------------------------------- smoothness, plumbing
@pytest.mark.parametrize("gout", [None, 0.37], ids=["gout-none", "gout-0.37"])
@pytest.mark.parametrize("overlap", [True, False], ids=["side-stream", "one-stream"])
def test_smoothness_through_photometric_loss(dev, overlap, gout):
    """each d_disp[s] of ops.PhotometricLoss ALONE against the restatement (the chain tests only see it added to the
    photometric depth gradient, where it is 1e-4 of the norm), with the smoothness kernels on the side stream
    (RT.overlap) and on the caller's.  The two settings are not required to be bit-equal: the f64 atomics arrive in any
    order."""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip import ops
    B, H, W, S = 2, 32, 64, 4
    data, depths, disps = T.chain_batch()
    hw = [(H >> s, W >> s) for s in range(S)]
    img0 = data[("original_image", 0)]
    ref = T.smooth_terms(disps, T.color_pyramid(img0, hw, F64), [0, 1, 2, 3], gout, F64)
    ref32 = T.smooth_terms(disps, T.color_pyramid(img0, hw, F32), [0, 1, 2, 3], gout, F32)
    was = RT.overlap
    RT.overlap = overlap
    try:
        pl = ops.PhotometricLoss(B, H, W, [0, 1, 2, 3], dev, 0.5, 100.0)
        fulls = [guarded(B * h * w, F32, dev) for h, w in hw]
        pl.d_disp = [v.view(B, 1, h, w) for (v, _), (h, w) in zip(fulls, hw)]
        assert (pl._fork(dev) is not None) == overlap
        out = pl.forward(img0.to(dev), [data[("original_image", 1)].to(dev), data[("original_image", -1)].to(dev)],
                         data["P2"].to(dev), [data[("relative_pose", 1)].to(dev), data[("relative_pose", -1)].to(dev)],
                         None, [d.to(dev) for d in depths], [d.to(dev) for d in disps])
        g = None if gout is None else torch.tensor(gout, dtype=F64, device=dev)
        _, d_disp, _ = pl.backward(g)
        torch.cuda.synchronize()
    finally:
        RT.overlap = was
    out = out.cpu()
    for s in range(S):
        # smooth_loss/s: 2^-20 for the float sums (as in the direct test) + 2^-22 for the three float operations of
        # loss_finalize + 2^-22 for the colour pyramid, whose float32 block means (up to 64 terms) move an edge weight
        # by a few 1e-7 with either sign
        want = float(ref[s]["loss"])
        assert abs(float(out[S + s]) - want) <= (2.0 ** -20 + 2.0 ** -21) * want, (s, float(out[S + s]), want)
        assert d_disp[s].data_ptr() == fulls[s][0].data_ptr()
        held("d_disp chain s%d %s %s" % (s, "side" if overlap else "one", "gout" if gout else "none"), d_disp[s],
             ref[s]["d_disp"], ref32[s]["d_disp"])
        assert bool((d_disp[s][1] == 0.0).all()) and bool((d_disp[s][0] != 0.0).any())
    assert intact(*[f for _, f in fulls])


# ---------------------------------------------------------------------------------------------- fs_loss_finalize
@pytest.mark.parametrize("with_total", [True, False], ids=["total_out", "total_null"])
@pytest.mark.parametrize("case", range(len(T.FINALIZE_CASES)), ids=["B%d-S%d" % (B, len(hw)) for B, hw, _ in T.FINALIZE_CASES])
def test_loss_finalize(dev, case, with_total):
    from fsnet_amd.hip.binding import FsSmoothArgs
    lib, stream_ptr = lib_()
    B, hw, sids = T.FINALIZE_CASES[case]
    S = len(hw)
    ls, ms, sm = T.finalize_sums(B, hw, case)
    want = T.finalize(ls, ms, sm, B, [h for h, _ in hw], [w for _, w in hw], sids)
    sa = FsSmoothArgs()
    sa.B, sa.S = B, S
    for s, (h, w) in enumerate(hw):
        sa.h[s], sa.w[s], sa.scale_id[s] = h, w, sids[s]
    d_ls, d_ms, d_sm = (torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev) for a in (ls, ms, sm))
    out, out_full = guarded(2 * S + 1, F64, dev)
    tot, tot_full = guarded(1, F64, dev)
    st = lib.fs_loss_finalize(d_ls.data_ptr(), d_ms.data_ptr(), d_sm.data_ptr(), C.byref(sa), out.data_ptr(),
                              tot.data_ptr() if with_total else None, stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s in range(S):
        # smooth_loss/s: three float operations (the cast of the f64 mean, the sum, the product; the division by 2^k is
        # exact) -> 2^-22 relative.  loss/s: the f64 part to 1e-12 relative, plus that float error of its smoothness term
        assert abs(got[S + s] - want[S + s]) <= 2.0 ** -22 * want[S + s], (s, got[S + s], want[S + s])
        assert abs(got[s] - want[s]) <= 1e-12 * want[s] + 2.0 ** -22 * want[S + s], (s, got[s], want[s])
    assert abs(got[2 * S] - want[2 * S]) <= 1e-12 * want[2 * S] + 2.0 ** -22 * want[S:2 * S].mean()
    if with_total:
        assert torch.equal(out[2 * S:], tot)                      # bit for bit
    else:
        assert bool(torch.isnan(tot_full).all())
    assert intact(out_full, tot_full)


# ---------------------------------------------------------------------------------------------- fs_sumsq
@pytest.mark.parametrize("n", T.SUMSQ_NS)
def test_sumsq(dev, n):
    lib, stream_ptr = lib_()
    g = (3 * torch.randn(n, generator=torch.Generator().manual_seed(n))).float()
    want = float((g.double() ** 2).sum())
    gd = g.to(dev)
    assert gd.data_ptr() % 16 == 0
    out, out_full = guarded(1, F64, dev, 1.5)
    ctr = torch.tensor([41, 77, 77, 77], dtype=torch.int32, device=dev)
    assert lib.fs_sumsq(gd.data_ptr(), n, out.data_ptr(), ctr.data_ptr(), stream_ptr()) == 0
    out2, out2_full = guarded(1, F64, dev, 1.5)
    assert lib.fs_sumsq(gd.data_ptr(), n, out2.data_ptr(), None, stream_ptr()) == 0         # step_counter = NULL
    torch.cuda.synchronize()
    # the kernel ADDS to out.  2^-21 relative: two float pair-sums (four roundings of products, two of sums) per
    # 16-byte unit, everything after that is f64
    for o in (out, out2):
        got = float(o.cpu()[0]) - 1.5
        print("sumsq n=%d: rel err %.3e (bound %.3e)" % (n, abs(got - want) / want, 2.0 ** -21))
        assert abs(got - want) <= 2.0 ** -21 * want, (n, got, want)
    assert ctr.cpu().tolist() == [42, 77, 77, 77]
    assert intact(out_full, out2_full)


# ---------------------------------------------------------------------------------------------- depth-bin head
def _bins(K, dev):
    from oracle import fsnet_oracle as O
    b = O.depth_bins(T.MIN_D, T.MAX_D, K).float()
    assert b.shape == (K,)
    return b, b.to(dev)


GRADS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("pad", [0, 4], ids=["Cl=K", "Cl=K+4"])
@pytest.mark.parametrize("K", T.HEAD_KS)
def test_depth_head_single(dev, K, pad):
    lib, stream_ptr = lib_()
    Cl = K + pad
    n, h, w = T.HEAD_SINGLE
    M = n * h * w
    g = torch.Generator().manual_seed(10 * K + pad)
    logits = T.head_logits(g, M, K, Cl)
    bins, bins_d = _bins(K, dev)
    gd, gp = torch.randn(M, generator=g), torch.randn(M, generator=g)
    ld, gd_d, gp_d = logits.to(dev), gd.to(dev), gp.to(dev)
    assert ld.data_ptr() % 16 == 0
    depth, depth_full = guarded(M, F32, dev)
    disp, disp_full = guarded(M, F32, dev)
    assert lib.fs_depth_head_fwd(ld.data_ptr(), bins_d.data_ptr(), depth.data_ptr(), disp.data_ptr(), M, K, Cl,
                                 T.MIN_D, T.MAX_D, stream_ptr()) == 0
    torch.cuda.synchronize()
    r64 = T.head(logits[:, :K], bins, None, T.MIN_D, T.MAX_D, gd, gp, F64)
    r32 = T.head(logits[:, :K], bins, None, T.MIN_D, T.MAX_D, gd, gp, F32)
    held("head K%d Cl%d depth" % (K, Cl), depth, r64[0], r32[0])
    held("head K%d Cl%d disp" % (K, Cl), disp, r64[1], r32[1])
    assert intact(depth_full, disp_full)
    for use_d, use_p in GRADS:
        a, b = (gd if use_d else None), (gp if use_p else None)
        r64 = T.head(logits[:, :K], bins, None, T.MIN_D, T.MAX_D, a, b, F64)
        r32 = T.head(logits[:, :K], bins, None, T.MIN_D, T.MAX_D, a, b, F32)
        for dt, code in ((F32, 0), (BF16, 1)):
            dl, dl_full = guarded(M * Cl, dt, dev)
            assert lib.fs_depth_head_bwd(ld.data_ptr(), bins_d.data_ptr(), gd_d.data_ptr() if use_d else None,
                                         gp_d.data_ptr() if use_p else None, dl.data_ptr(), M, K, Cl, T.MIN_D, T.MAX_D,
                                         code, stream_ptr()) == 0
            torch.cuda.synchronize()
            got = dl.view(M, Cl)[:, :K]
            held("head K%d Cl%d dlogits %s d%d p%d" % (K, Cl, "bf16" if code else "f32", use_d, use_p), got, r64[2], r32[2])
            if not (use_d or use_p):
                assert bool((got == 0).all())
            assert intact(dl_full)


def _head_batch(dev, logits, P2_d, bwd, dt, gds, gps):
    """FsHeadBatch over guarded outputs -> (hb, outputs per scale, the tensors to keep alive)"""
    from fsnet_amd.hip.binding import FsHeadBatch
    hb = FsHeadBatch()
    hb.n = len(logits)
    if P2_d is not None:
        hb.P2, hb.base_fx, hb.nimg = P2_d.data_ptr(), T.HEAD_BASE_FX, P2_d.shape[0]
    outs, keep = [], []
    for s, lg in enumerate(logits):
        M = lg.shape[0]
        hb.logits[s], hb.M[s] = lg.data_ptr(), M
        if bwd:
            o = guarded(M * lg.shape[1], dt, dev)
            hb.dlogits[s] = o[0].data_ptr()
            for arr, src in ((hb.d_depth, gds[s]), (hb.d_disp, gps[s])):
                if src is not None:
                    keep.append(src.to(dev))
                    arr[s] = keep[-1].data_ptr()
            outs.append(o)
        else:
            a, b = guarded(M, F32, dev), guarded(M, F32, dev)
            hb.depth[s], hb.disp[s] = a[0].data_ptr(), b[0].data_ptr()
            outs.append((a, b))
    return hb, outs, keep


@pytest.mark.parametrize("scaled", [True, False], ids=["focal-scale", "no-scale"])
@pytest.mark.parametrize("pad", [0, 4], ids=["Cl=K", "Cl=K+4"])
@pytest.mark.parametrize("K", T.HEAD_KS)
def test_depth_head_multi(dev, K, pad, scaled):
    """all scales in one launch; with the per-image focal scale, three images at fx = (0.7, 1.0, 1.9) x base_fx: a wrong
    image index or a missing `g *= sc` shows"""
    lib, stream_ptr = lib_()
    Cl = K + pad
    g = torch.Generator().manual_seed(1000 + 10 * K + pad)
    Ms = [n * h * w for n, h, w in T.HEAD_MULTI]
    nimg = T.HEAD_MULTI[0][0]
    logits = [T.head_logits(g, M, K, Cl) for M in Ms]
    bins, bins_d = _bins(K, dev)
    P2 = T.head_P2(nimg)
    P2_d = P2.to(dev) if scaled else None
    gds = [torch.randn(M, generator=g) for M in Ms]
    gps = [torch.randn(M, generator=g) for M in Ms]
    gds[1], gps[2] = None, None
    ld = [x.to(dev) for x in logits]

    def sc(s, dtype):
        return T.head_scale(P2, T.HEAD_BASE_FX, Ms[s] // nimg, dtype) if scaled else None
    hb, outs, _ = _head_batch(dev, ld, P2_d, False, F32, None, None)
    assert lib.fs_depth_head_fwd_multi(C.byref(hb), bins_d.data_ptr(), K, Cl, T.MIN_D, T.MAX_D, stream_ptr()) == 0
    torch.cuda.synchronize()
    tag = "head multi%s K%d Cl%d" % ("+fx" if scaled else "", K, Cl)
    for s in range(3):
        r64 = T.head(logits[s][:, :K], bins, sc(s, F64), T.MIN_D, T.MAX_D, gds[s], gps[s], F64)
        r32 = T.head(logits[s][:, :K], bins, sc(s, F32), T.MIN_D, T.MAX_D, gds[s], gps[s], F32)
        (depth, depth_full), (disp, disp_full) = outs[s]
        held("%s s%d depth" % (tag, s), depth, r64[0], r32[0])
        held("%s s%d disp" % (tag, s), disp, r64[1], r32[1])
        assert intact(depth_full, disp_full)
    for dt, code in ((F32, 0), (BF16, 1)):
        hb, outs, keep = _head_batch(dev, ld, P2_d, True, dt, gds, gps)
        assert lib.fs_depth_head_bwd_multi(C.byref(hb), bins_d.data_ptr(), K, Cl, T.MIN_D, T.MAX_D, code, stream_ptr()) == 0
        torch.cuda.synchronize()
        for s in range(3):
            r64 = T.head(logits[s][:, :K], bins, sc(s, F64), T.MIN_D, T.MAX_D, gds[s], gps[s], F64)
            r32 = T.head(logits[s][:, :K], bins, sc(s, F32), T.MIN_D, T.MAX_D, gds[s], gps[s], F32)
            dl, dl_full = outs[s]
            held("%s s%d dlogits %s" % (tag, s, "bf16" if code else "f32"), dl.view(Ms[s], Cl)[:, :K], r64[2], r32[2])
            assert intact(dl_full)


def test_depth_head_rejects(dev):
    """K = 24, Cl < K, P2 with M % nimg != 0: FS_EINVAL and no launch"""
    lib, stream_ptr = lib_()
    Ms = [n * h * w for n, h, w in T.HEAD_MULTI]
    g = torch.Generator().manual_seed(3)
    ld = [T.head_logits(g, M, 16, 24).to(dev) for M in Ms]
    bins_d = torch.ones(64, device=dev)
    P2_two = T.head_P2(2).to(dev)
    outs_all = []
    for K, Cl, P2_d in ((24, 24, None), (16, 12, None), (16, 24, P2_two)):
        if P2_d is None:
            depth, disp, dl = guarded(Ms[0], F32, dev), guarded(Ms[0], F32, dev), guarded(Ms[0] * 24, F32, dev)
            outs_all += [depth, disp, dl]
            assert lib.fs_depth_head_fwd(ld[0].data_ptr(), bins_d.data_ptr(), depth[0].data_ptr(), disp[0].data_ptr(), Ms[0], K,
                                         Cl, T.MIN_D, T.MAX_D, stream_ptr()) == FS_EINVAL
            for code in (0, 1):
                assert lib.fs_depth_head_bwd(ld[0].data_ptr(), bins_d.data_ptr(), None, None, dl[0].data_ptr(), Ms[0], K, Cl,
                                             T.MIN_D, T.MAX_D, code, stream_ptr()) == FS_EINVAL
        hb, outs, _ = _head_batch(dev, ld, P2_d, False, F32, None, None)
        outs_all += [o for pair in outs for o in pair]
        assert lib.fs_depth_head_fwd_multi(C.byref(hb), bins_d.data_ptr(), K, Cl, T.MIN_D, T.MAX_D, stream_ptr()) == FS_EINVAL
        for code in (0, 1):
            hb, outs, _ = _head_batch(dev, ld, P2_d, True, F32, [None] * 3, [None] * 3)
            outs_all += outs
            assert lib.fs_depth_head_bwd_multi(C.byref(hb), bins_d.data_ptr(), K, Cl, T.MIN_D, T.MAX_D, code,
                                               stream_ptr()) == FS_EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(full).all()) for _, full in outs_all)


# ---------------------------------------------------------------------------------------------- pose tail
@pytest.mark.parametrize("hw", T.POSE_HW)
@pytest.mark.parametrize("nframes,Cx", [(1, 8), (2, 16)], ids=["1frame-C8", "2frames-C16"])
def test_pose_tail(dev, nframes, Cx, hw):
    lib, stream_ptr = lib_()
    for B in (1, 3):
        for invert in (False, True):
            g = torch.Generator().manual_seed(hw * 100 + B * 10 + nframes * 2 + int(invert))
            x = T.pose_features(g, B, hw, Cx)
            dT = torch.randn(B, 4, 4, generator=g)
            r64 = T.pose_tail(x, nframes, invert, 0.01, dT, F64)
            r32 = T.pose_tail(x, nframes, invert, 0.01, dT, F32)
            assert float(r64[0][:, 0].norm(dim=-1).min()) > 1e-3          # never a zero rotation
            xd, dT_d = x.to(dev), dT.to(dev)
            aa, aa_full = guarded(B * nframes * 3, F32, dev)
            tr, tr_full = guarded(B * nframes * 3, F32, dev)
            Tm, Tm_full = guarded(B * 16, F32, dev)
            assert lib.fs_pose_tail_fwd(xd.data_ptr(), aa.data_ptr(), tr.data_ptr(), Tm.data_ptr(), B, hw, Cx, nframes,
                                        int(invert), 0.01, stream_ptr()) == 0
            torch.cuda.synchronize()
            tag = "pose f%d hw%d B%d %s" % (nframes, hw, B, "inv" if invert else "fwd")
            held(tag + " axisangle", aa.view(B, nframes, 1, 3), r64[0], r32[0])
            held(tag + " translation", tr.view(B, nframes, 1, 3), r64[1], r32[1])
            held(tag + " T", Tm.view(B, 4, 4), r64[2], r32[2])
            assert intact(aa_full, tr_full, Tm_full)
            for dt, code in ((F32, 0), (BF16, 1)):
                dx, dx_full = guarded(B * hw * Cx, dt, dev)
                assert lib.fs_pose_tail_bwd(xd.data_ptr(), dT_d.data_ptr(), dx.data_ptr(), B, hw, Cx, nframes, int(invert),
                                            0.01, code, stream_ptr()) == 0
                torch.cuda.synchronize()
                got = dx.view(B, hw, Cx)
                held(tag + " dx " + ("bf16" if code else "f32"), got, r64[3], r32[3])
                assert bool((got[:, :, 6:] == 0).all())           # frame 1's channels included
                assert bool((got[:, :, :6] != 0).all())
                assert intact(dx_full)
