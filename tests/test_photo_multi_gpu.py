"""The kernels of photo_multi.hip (photometric loss over N = 1..4 source frames) against the float64 chain of
tests/helpers_photo64n.py, compared as tests/test_photo_fused_seams_gpu.py compares the two-frame kernels: the same
yardstick (e = the reference's own fp32 noise per quantity and shape, the allowance A for the sampler's cell decisions,
1e-4 px of coordinate approximation on the warped image) and the same FACTORs, imported from that file — per frame the
arithmetic is the two-frame kernels', so their measured margins carry over.

Shapes come from fs_photo_multi_strip() by the rule of helpers_photo64.SHAPES_B (helpers_photo64n.shapes_b); the inputs
and the conditions they meet are those of helpers_photo64n (tests/test_photo64n_cpu.py asserts the conditions for every
input used here)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_photo64 as P
from tests import helpers_photo64n as Q
from tests.test_photo_fused_seams_gpu import FACTOR, _ratio, _where, run_ops as run_ops_two

pytestmark = pytest.mark.gpu

NAMES = Q.names()


def _on_dev(case, opts, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(img0=t(case["img0"]), src=[t(a) for a in case["src"]], P2=t(case["P2"]), T=[t(a) for a in case["T"]],
                depths=[t(a) for a in case["depths"]],
                pm=t(case["patched_mask"]) if opts.get("use_patched_mask", True) else None,
                mm=t(case["motion_mask"]) if opts.get("use_motion_mask") else None)


def run_ops(dev, case, opts, want_pred=True, noise_seed=-1):
    """forward + backward through ops.PhotometricLoss on the N-frame kernels, N = 2 included (maps = (H >> s, W >> s));
    pred / ov / sel pre-filled with NaN / 255 / 255 so that an unwritten cell shows"""
    from fsnet_amd.hip import ops
    B, H, W, S, N = case["B"], case["H"], case["W"], len(case["maps"]), len(case["src"])
    assert list(case["maps"]) == [(H >> s, W >> s) for s in range(S)]
    d = _on_dev(case, opts, dev)
    pl = ops.PhotometricLoss(B, H, W, list(range(S)), dev, 0.5, 100.0, nsrc=N, force_multi=True, want_pred=want_pred,
                             overlapped_mask=opts.get("overlapped_mask", True))
    assert pl.multi
    if want_pred:
        pl.pred.fill_(float("nan"))
        pl.ov.fill_(255)
    pl.sel.fill_(255)
    disps = [1.0 / x for x in d["depths"]]
    pl.forward(d["img0"], d["src"], d["P2"], d["T"], d["pm"], d["depths"], disps, noise_seed=noise_seed,
               motion_mask=d["mm"])
    loss_sums = pl.loss_sums.clone()
    gout = torch.tensor(opts["gout"], dtype=torch.float64, device=dev) if "gout" in opts else None
    d_depth, _, dT = pl.backward(gout)
    torch.cuda.synchronize()
    return dict(sel=pl.sel.cpu(), pred=pl.pred.cpu() if want_pred else None, ov=pl.ov.cpu() if want_pred else None,
                loss_sums=loss_sums.cpu().view(S, B), d_depth=[x.cpu().double() for x in d_depth],
                dT=[x.cpu().double() for x in dT], ident=pl.ident.cpu())


def run_direct(dev, case, opts):
    """the same through the C ABI with a hand-filled FsPhotoMultiArgs: depth maps of any size"""
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsPhotoMultiArgs, check, stream_ptr
    B, H, W, S, N = case["B"], case["H"], case["W"], len(case["maps"]), len(case["src"])
    d = _on_dev(case, opts, dev)
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=dev)
    geo, msum, loss_sums = z(B, 18 + 12 * N), z(B, dtype=f64), z(S * B, dtype=f64)
    ident = torch.full((B, N, H, W), float("nan"), dtype=f32, device=dev)
    pred = torch.full((S, N, B, 3, H, W), float("nan"), dtype=f32, device=dev)
    ov = torch.full((S, N, B, H, W), 255, dtype=u8, device=dev)
    sel = torch.full((S, B, H, W), 255, dtype=u8, device=dev)
    tiles = int(lib.fs_photo_multi_bwd_tiles(H, W))
    dP = z(S * B * tiles, N, 12)
    dd = [z(B, 1, h, w) for h, w in case["maps"]]
    dT = z(N, B, 4, 4)
    pa = FsPhotoMultiArgs()
    pa.img0 = d["img0"].data_ptr()
    for f in range(N):
        pa.img_src[f] = d["src"][f].data_ptr()
    pa.patched_mask = None if d["pm"] is None else d["pm"].data_ptr()
    pa.motion_mask = None if d["mm"] is None else d["mm"].data_ptr()
    for i, (h, w) in enumerate(case["maps"]):
        pa.depth[i], pa.d_depth[i], pa.dh[i], pa.dw[i] = d["depths"][i].data_ptr(), dd[i].data_ptr(), h, w
    pa.geo, pa.pred, pa.ov, pa.ident, pa.sel = geo.data_ptr(), pred.data_ptr(), ov.data_ptr(), ident.data_ptr(), sel.data_ptr()
    pa.loss_sums, pa.mask_sum, pa.dP = loss_sums.data_ptr(), msum.data_ptr(), dP.data_ptr()
    pa.B, pa.H, pa.W, pa.S, pa.nsrc = B, H, W, S, N
    pa.noise_seed = -1
    pa.no_overlap_mask = 0 if opts.get("overlapped_mask", True) else 1
    st = stream_ptr()
    Tp = (C.c_void_p * 4)(*[t.data_ptr() for t in d["T"]])
    check(lib.fs_photo_multi_setup(d["P2"].data_ptr(), Tp, N, geo.data_ptr(), B, None, st), "setup")
    check(lib.fs_photo_multi_identity(C.byref(pa), st), "identity")
    check(lib.fs_photo_multi_fwd(C.byref(pa), st), "fwd")
    check(lib.fs_photo_multi_bwd(C.byref(pa), st), "bwd")
    check(lib.fs_photo_multi_pose_grad(geo.data_ptr(), dP.data_ptr(), dT.data_ptr(), N, B, S, tiles, st), "pose_grad")
    torch.cuda.synchronize()
    return dict(sel=sel.cpu(), pred=pred.cpu(), ov=ov.cpu(), loss_sums=loss_sums.cpu().view(S, B),
                d_depth=[x.cpu().double() for x in dd], dT=[dT[f].cpu().double() for f in range(N)], ident=ident.cpu())


def compare(name, case, opts, got):
    """all assertions of test_photo_fused_seams_gpu.compare for N frames; prints the ratio of every quantity first"""
    B, H, W, S, N = case["B"], case["H"], case["W"], len(case["maps"]), len(case["src"])
    sel = got["sel"].long()
    assert int(sel.max()) <= 2 * N, "%s: unwritten sel cells at %s" % (name, _where(sel > 2 * N))
    assert bool(torch.isfinite(got["pred"]).all()), "%s: unwritten pred cells at %s" % (name, _where(~torch.isfinite(got["pred"])))
    assert int(got["ov"].max()) <= 1, "%s: unwritten ov cells at %s" % (name, _where(got["ov"] > 1))
    assert bool(torch.isfinite(got["ident"]).all()), "%s: unwritten identity cells at %s" % (name, _where(~torch.isfinite(got["ident"])))
    y = Q.yardsticks_n(case, opts, sel=[sel[s] for s in range(S)])
    r64, r0 = y["free64"], y["r0"]
    fails, line = [], []
    for s in range(S):
        ov_exc = y["ov_excused"][s]
        exc = ov_exc.any(0) | y["sel_excused"][s]
        assert float(exc.double().mean()) <= 0.005, (name, s)
        bad = (got["ov"][s].bool() != r64["ov"][s]) & ~ov_exc
        if bool(bad.any()):
            fails.append("scale %d: ov differs at (f, b, y, x) %s" % (s, _where(bad)))
        bad = (sel[s] != r64["argmin"][s]) & ~exc
        if bool(bad.any()):
            fails.append("scale %d: sel differs at (b, y, x) %s" % (s, _where(bad)))
        err = (got["pred"][s].double() - r64["pred"][s]).abs() - 1e-4 * (r64["jx"][s].abs() + r64["jy"][s].abs())
        rp = _ratio(err.clamp(min=0).max(), y["e_pred"][s])
        if rp > FACTOR["pred"]:
            fails.append("scale %d: pred %.2f e at (f, b, c, y, x) %s" % (s, rp, _where(err > FACTOR["pred"] * y["e_pred"][s])))
        A, e = y["A"][s], y["e_depth"][s]
        assert float((A > 4 * e).double().mean()) <= 0.02, (name, s)
        err = (got["d_depth"][s] - r0["g_depth"][s]).abs() - A
        rd = _ratio(err.clamp(min=0).max(), e)
        if rd > FACTOR["d_depth"]:
            at = err > FACTOR["d_depth"] * e
            fails.append("scale %d: d_depth %.2f e (e %.2e) at (b, 0, y, x) %s: excess / reference / allowance %s" % (
                s, rd, e, _where(at), [("%.2e" % a, "%.2e" % b, "%.2e" % c) for a, b, c in
                                       zip(err[at][:6].tolist(), r0["g_depth"][s][at][:6].tolist(), A[at][:6].tolist())]))
        stay = (r0["g_depth"][s] == 0) & (A == 0)
        if bool((got["d_depth"][s][stay] != 0).any()):
            fails.append("scale %d: d_depth written where no gradient arrives: %s" % (s, _where(stay & (got["d_depth"][s] != 0))))
        raw = _ratio((got["pred"][s].double() - r64["pred"][s]).abs().max(), y["e_pred"][s])
        line.append("s%d pred %.2f (without the coordinate term %.1f) d_depth %.2f" % (s, rp, raw, rd))
    rl = _ratio((got["loss_sums"] - r0["loss_sums"]).abs().max(), y["e_loss"])
    if rl > FACTOR["loss"]:
        fails.append("loss_sums %.2f e: %s vs %s" % (rl, got["loss_sums"].tolist(), r0["loss_sums"].tolist()))
    rt = []
    for f in range(N):
        err = (got["dT"][f] - r0["dT"][f]).abs() - y["A_dT"][f]
        rt.append(_ratio(err.clamp(min=0).max(), y["e_dT"][f]))
        if rt[-1] > FACTOR["dT"]:
            fails.append("dT[%d] %.2f e (e %.2e): got %s reference %s" % (f, rt[-1], y["e_dT"][f], got["dT"][f].tolist(), r0["dT"][f].tolist()))
    print("RATIO %-30s loss %.2f dT %s | %s" % (name, rl, " ".join("%.2f" % v for v in rt), " | ".join(line)))
    assert not fails, "%s: %s" % (name, "; ".join(fails))
    return y


@pytest.mark.parametrize("name", NAMES["a"])
def test_production_plumbing_all_scales(dev, name):
    case, opts = Q.case_named_n(name)
    got = run_ops(dev, case, opts)
    compare(name, case, opts, got)
    if name.endswith("B2") and "24x64" in name:          # the same once without pred / ov, per N
        lean = run_ops(dev, case, opts, want_pred=False)
        assert torch.equal(lean["sel"], got["sel"])


@pytest.mark.parametrize("name", NAMES["b"])
def test_scale0_sweep_over_strip_seams(dev, name):
    case, opts = Q.case_named_n(name)
    compare(name, case, opts, run_ops(dev, case, opts))


@pytest.mark.parametrize("name", NAMES["c"])
def test_free_depth_map_sizes(dev, name):
    case, opts = Q.case_named_n(name)
    compare(name, case, opts, run_direct(dev, case, opts))


@pytest.mark.parametrize("name", NAMES["d"])
def test_loss_options(dev, name):
    case, opts = Q.case_named_n(name)
    compare(name, case, opts, run_ops(dev, case, opts))


def _as_n(case):
    c = dict(case)
    c["N"] = len(case["src"])
    return c


def test_two_frames_through_the_new_path_match_the_two_source_kernels(dev):
    """N = 2 on a-40x128-B2 of the two-frame sweep: the same yardstick, and sel / ov equal to the two-source path's
    outside the excused cells"""
    case, opts = P.case_named("a-40x128-B2")
    got = run_ops(dev, _as_n(case), opts)
    y = compare("n2-a-40x128-B2", _as_n(case), opts, got)
    old = run_ops_two(dev, case, opts)
    for s in range(len(case["maps"])):
        ov_exc = y["ov_excused"][s]
        exc = ov_exc.any(0) | y["sel_excused"][s]
        assert not bool(((got["sel"][s] != old["sel"][s]) & ~exc).any()), s
        assert not bool(((got["ov"][s] != old["ov"][s]) & ~ov_exc).any()), s


@pytest.mark.parametrize("N", [1, 3, 4])
def test_sources_equal_to_the_target(dev, N):
    """identical frames: the identity terms are exactly zero, the first one wins everywhere (strict <), and nothing may
    reach d_depth or dT"""
    case = dict(Q.make_case_n(2, 17, 63, N, ((17, 63), (5, 9)), seed=5))
    case["src"] = [case["img0"].copy() for _ in range(N)]
    got = run_direct(dev, case, {})
    assert bool((got["ident"] == 0).all())
    assert int(got["sel"].max()) < N and int(got["sel"].max()) == 0
    assert all(bool((x == 0).all()) for x in got["d_depth"]) and all(bool((x == 0).all()) for x in got["dT"])


@pytest.mark.parametrize("N", [1, 3, 4])
def test_tie_noise_spreads_equal_identity_terms(dev, N):
    """the same with the tie-break noise on (seed 3): every identity index wins between 1 / (2 N) and 2 / N of the
    pixels, no reprojection term wins, and the same seed gives the same selection twice"""
    H, W = 32, 120
    case = dict(Q.make_case_n(2, H, W, N, [(H >> s, W >> s) for s in range(4)], seed=1))
    case["src"] = [case["img0"].copy() for _ in range(N)]
    a = run_ops(dev, case, {}, noise_seed=3)
    b = run_ops(dev, case, {}, noise_seed=3)
    assert torch.equal(a["sel"], b["sel"])
    assert int(a["sel"].max()) < N
    for s in range(4):
        for k in range(N):
            share = float((a["sel"][s] == k).double().mean())
            assert 1.0 / (2 * N) <= share <= 2.0 / N, (s, k, share)
    assert all(bool((x == 0).all()) for x in a["d_depth"]) and all(bool((x == 0).all()) for x in a["dT"])


def test_two_runs_are_bit_identical(dev):
    case, opts = Q.case_named_n("n4-a-40x72-B2")
    a, b = run_ops(dev, case, opts), run_ops(dev, case, opts)
    assert torch.equal(a["sel"], b["sel"]) and torch.equal(a["ov"], b["ov"]) and torch.equal(a["pred"], b["pred"])
