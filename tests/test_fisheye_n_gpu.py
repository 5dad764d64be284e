"""The fisheye (Mei) loss chain over N = 1, 3, 4 source frames on the GPU (fs_photo_mei_multi_*, FishEyeDecoder with
frame_ids of any admitted length): against the REAL FishEyeDecoder.loss (tests/golden/fisheye_nsrc.npz), against the CPU
oracle at a shape with ragged last strips, N = 2 through the new kernels against the two-source fisheye kernels, the
degenerate cases, and the model.  The bounds are those of tests/test_fisheye_gpu.py: the per-frame arithmetic is the
same text.  Inputs and the conditions they meet: tests/helpers_fisheye_n.py (asserted in tests/test_fisheye_n_cpu.py).

The 66 x 70 runs go through the C ABI with a hand-filled FsPhotoMeiMultiArgs (run_direct): ops.PhotometricLoss also
launches the smoothness term, whose colour pyramid (fs_color_pyramid_multi) takes integer ratios only and refuses a
66 x 70 image with 8 x 8 maps.  Those runs therefore hold every quantity the photometric chain produces (per-scale loss
and total without the smoothness term, warp, overlap masks, selection, d_depth, pose gradients) to the same bounds; the
smoothness bound has nothing to be applied to there.  The figures every test prints are in docs/LAB_r07.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import fisheye_oracle as FO
from oracle import fsnet_oracle as O
from tests import helpers_fisheye_n as Q
from tests.test_fisheye_n_cpu import case_from_fisheye_golden
from tests.test_oracle_golden import fisheye_chain_inputs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_ref = {}


def to_dev(data, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in data.items()}


def run_chain(dev, case, want_pred=True, force_multi=False, srcs=None):
    """forward + backward through ops.PhotometricLoss with the ray tables staged; pred / ov / sel pre-filled with
    NaN / 255 / 255 so that an unwritten cell shows"""
    from fsnet_amd.hip import ops
    from fsnet_amd.monodepth.networks.utils.mei_fisheye_utils import MeiCameraProjection
    data, fids, H, W, N = case["data"], case["fids"], case["H"], case["W"], case["N"]
    B = data["P2"].shape[0]
    pl = ops.PhotometricLoss(B, H, W, [0, 1, 2, 3], dev, Q.MIN_DEPTH, Q.MAX_DEPTH, nsrc=N, force_multi=force_multi,
                             want_pred=want_pred)
    assert pl.multi == (force_multi or N != 2)
    tabs, rows = MeiCameraProjection().tables(H, W, data["P2"], data["calib_meta"], dev)
    pl.stage_fisheye(tabs, rows)
    assert pl._be.name == ("photo_mei_multi" if pl.multi else "photo_fused")
    if want_pred:
        pl.pred.fill_(float("nan"))
        pl.ov.fill_(255)
    pl.sel.fill_(255)
    pl.ident.fill_(float("nan"))
    depths = case["depths"]
    disps = [O.depth_to_disp(d, Q.MIN_DEPTH, Q.MAX_DEPTH) for d in depths]
    Ts = Q.transforms(case)
    if srcs is None:
        srcs = [data[("original_image", f)] for f in fids[1:]]
    out = pl.forward(data[("original_image", 0)].to(dev), [s.to(dev) for s in srcs], data["P2"].to(dev),
                     [t.to(dev).contiguous() for t in Ts], data["patched_mask"].to(dev), [d.to(dev) for d in depths],
                     [d.to(dev) for d in disps], noise_seed=-1)
    loss_sums = pl.loss_sums.clone()
    d_depth, d_disp, dT = pl.backward()
    torch.cuda.synchronize()
    out = out.cpu()
    gdepth = []
    for s in range(4):                      # d loss / d depth_s: the chain's own part + the smoothness term's through disp
        d = depths[s].clone().requires_grad_(True)
        O.depth_to_disp(d, Q.MIN_DEPTH, Q.MAX_DEPTH).backward(d_disp[s].cpu())
        gdepth.append(d_depth[s].cpu() + d.grad)
    return dict(total=float(out[8]), loss=[float(out[s]) for s in range(4)], smooth=[float(out[4 + s]) for s in range(4)],
                out=out, sel=pl.sel.cpu(), pred=pl.pred.cpu() if want_pred else None,
                ov=pl.ov.cpu() if want_pred else None, ident=pl.ident.cpu(), loss_sums=loss_sums.cpu(),
                gdepth=gdepth, d_depth=[x.cpu() for x in d_depth], dT=[x.cpu() for x in dT])


def run_direct(dev, case, want_pred=True, srcs=None):
    """the photometric chain alone through the C ABI with a hand-filled FsPhotoMeiMultiArgs (any image size): setup,
    mask staging, identity planes, forward, backward, pose gradient; outputs pre-filled as in run_chain"""
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsPhotoMeiMultiArgs, check, stream_ptr
    from fsnet_amd.monodepth.networks.utils.mei_fisheye_utils import MeiCameraProjection
    data, fids, H, W, N = case["data"], case["fids"], case["H"], case["W"], case["N"]
    B, S = data["P2"].shape[0], 4
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=dev)
    tabs, rows = MeiCameraProjection().tables(H, W, data["P2"], data["calib_meta"], dev)
    lut = torch.tensor([t.data_ptr() for t in tabs], dtype=torch.int64).to(dev)
    mei = torch.from_numpy(rows.copy()).to(dev)
    img0 = data[("original_image", 0)].to(dev)
    srcs = [(data[("original_image", f)] if srcs is None else srcs[j]).to(dev).contiguous() for j, f in enumerate(fids[1:])]
    pm = data["patched_mask"].to(dev)
    depths = [d.to(dev).contiguous() for d in case["depths"]]
    Ts = [t.to(dev).contiguous() for t in Q.transforms(case)]
    geo, msum, loss_sums = z(B, 18 + 12 * N), z(B, dtype=f64), z(S * B, dtype=f64)
    warp_mask = torch.full((B, H, W), float("nan"), dtype=f32, device=dev)
    ident = torch.full((B, N, H, W), float("nan"), dtype=f32, device=dev)
    pred = torch.full((S, N, B, 3, H, W), float("nan"), dtype=f32, device=dev) if want_pred else None
    ov = torch.full((S, N, B, H, W), 255, dtype=u8, device=dev) if want_pred else None
    sel = torch.full((S, B, H, W), 255, dtype=u8, device=dev)
    tiles = int(lib.fs_photo_multi_bwd_tiles(H, W))
    dP = z(S * B * tiles, N, 12)
    dd = [z(*d.shape) for d in depths]
    dT = z(N, B, 4, 4)
    pa = FsPhotoMeiMultiArgs()
    pa.img0 = img0.data_ptr()
    for j in range(N):
        pa.img_src[j] = srcs[j].data_ptr()
    pa.patched_mask = pm.data_ptr()
    for i, d in enumerate(depths):
        pa.depth[i], pa.d_depth[i], pa.dh[i], pa.dw[i] = d.data_ptr(), dd[i].data_ptr(), d.shape[2], d.shape[3]
    pa.geo, pa.ident, pa.sel = geo.data_ptr(), ident.data_ptr(), sel.data_ptr()
    pa.pred, pa.ov = (pred.data_ptr(), ov.data_ptr()) if want_pred else (None, None)
    pa.loss_sums, pa.mask_sum, pa.dP = loss_sums.data_ptr(), msum.data_ptr(), dP.data_ptr()
    pa.B, pa.H, pa.W, pa.S, pa.nsrc = B, H, W, S, N
    pa.noise_seed = -1
    pa.lut_ptrs, pa.mei, pa.warp_mask = lut.data_ptr(), mei.data_ptr(), warp_mask.data_ptr()
    st = stream_ptr()
    Tp = (C.c_void_p * 4)(*[t.data_ptr() for t in Ts])
    check(lib.fs_photo_mei_multi_setup(Tp, N, geo.data_ptr(), B, None, st), "setup")
    check(lib.fs_mei_stage_mask(lut.data_ptr(), pm.data_ptr(), warp_mask.data_ptr(), B, H, W, st), "stage_mask")
    check(lib.fs_photo_multi_identity(C.byref(pa), st), "identity")
    check(lib.fs_photo_mei_multi_fwd(C.byref(pa), st), "fwd")
    check(lib.fs_photo_mei_multi_bwd(C.byref(pa), st), "bwd")
    check(lib.fs_photo_multi_pose_grad(geo.data_ptr(), dP.data_ptr(), dT.data_ptr(), N, B, S, tiles, st), "pose_grad")
    torch.cuda.synchronize()
    ls = loss_sums.cpu().view(S, B)
    loss = [float(ls[s].sum() / (msum.cpu().sum() + 1e-6)) for s in range(S)]
    geo_h = geo.cpu()
    assert bool((geo_h[:, :9] == torch.eye(3).reshape(9)).all()) and bool((geo_h[:, 9:18] == torch.eye(3).reshape(9)).all())
    return dict(total=sum(loss) / S, loss=loss, smooth=None, sel=sel.cpu(), pred=pred.cpu() if want_pred else None,
                ov=ov.cpu() if want_pred else None, ident=ident.cpu(), loss_sums=loss_sums.cpu(),
                gdepth=[x.cpu() for x in dd], d_depth=[x.cpu() for x in dd], dT=[dT[j].cpu() for j in range(N)])


def golden_reference(g, tag, fids):
    """the quantities compare() reads, from a golden file's entries"""
    return dict(total=float(g[tag + "total_loss"]), loss=[float(g[tag + "ld_loss_%d" % s]) for s in range(4)],
                smooth=[float(g[tag + "ld_smooth_loss_%d" % s]) for s in range(4)],
                warp={f: torch.from_numpy(g[tag + "warp0_%d" % f]) for f in fids[1:]},
                ov={f: g[tag + "ovmask0_%d" % f] for f in fids[1:]},
                gdepth=[torch.from_numpy(g[tag + "gdepth_%d" % s]) for s in range(4)],
                gaa={f: torch.from_numpy(g[tag + "gaa_%d" % f]) for f in fids[1:]},
                gtr={f: torch.from_numpy(g[tag + "gtr_%d" % f]) for f in fids[1:]})


def oracle_reference(case):
    """the same from FO.photometric_loss run here (no tie-break noise, as the kernels), for run_direct: the photometric
    chain alone — per-scale loss and total without the smoothness term, which sends no gradient either"""
    if case["name"] not in _ref:
        o = Q.oracle_chain(case, grads=True, detach_disp=True)
        fids = case["fids"]
        photo = [float(o["ld"]["loss/%d" % s]) - float(o["ld"]["smooth_loss/%d" % s]) for s in range(4)]
        _ref[case["name"]] = dict(
            total=sum(photo) / 4, loss=photo, smooth=None,
            warp={f: o["outputs"][("original_image", f, 0)].detach()[:, :, ::2, ::2] for f in fids[1:]},
            ov={f: o["outputs"][("overlapped_mask", f, 0)].numpy() for f in fids[1:]},
            gdepth=[d.grad for d in o["depths"]],
            gaa={f: a.grad for f, (a, t) in zip(fids[1:], o["poses"])},
            gtr={f: t.grad for f, (a, t) in zip(fids[1:], o["poses"])},
            min_idx=[o["outputs"][("min_idx", s)] for s in range(4)])
    return _ref[case["name"]]


def compare(name, case, got, ref):
    """the assertions of tests/test_fisheye_gpu.py::test_fisheye_chain_vs_reference_golden, with its bounds, for the
    case's frame list; prints every figure first"""
    fids, N = case["fids"], case["N"]
    sel = got["sel"].long()
    assert int(sel.max()) <= 2 * N, "%s: unwritten sel cells" % name
    assert bool(torch.isfinite(got["pred"]).all()), "%s: unwritten pred cells" % name
    assert int(got["ov"].max()) <= 1, "%s: unwritten ov cells" % name
    assert bool(torch.isfinite(got["ident"]).all()), "%s: unwritten identity cells" % name
    d_tot = abs(got["total"] - ref["total"])
    d_loss = [abs(got["loss"][s] - ref["loss"][s]) for s in range(4)]
    # (run_direct launches the photometric chain alone: no smoothness term on either side)
    d_sm = [abs(got["smooth"][s] - ref["smooth"][s]) for s in range(4)] if ref["smooth"] is not None else [0.0]
    assert (got["smooth"] is None) == (ref["smooth"] is None)
    d_warp = [float((got["pred"][0, j][:, :, ::2, ::2] - ref["warp"][f]).abs().max()) for j, f in enumerate(fids[1:])]
    ov = [float((got["ov"][0, j].bool().numpy() == ref["ov"][f]).mean()) for j, f in enumerate(fids[1:])]
    d_g = [float((got["gdepth"][s] - ref["gdepth"][s]).norm() / ref["gdepth"][s].norm()) for s in range(4)]
    Ts, leaves = Q.transforms(case, leaves=True)
    d_pose = []
    for j, f in enumerate(fids[1:]):
        (Ts[j] * got["dT"][j]).sum().backward()
        for g_, r in ((leaves[j][0].grad, ref["gaa"][f]), (leaves[j][1].grad, ref["gtr"][f])):
            d_pose.append(float((g_ - r).abs().max()) / (float(r.abs().max()) + 1e-9))
    print("FIGURES %-10s total %.2e loss/s %s smooth %.1e warp %s ov %s d_depth rel %s pose (of the largest) %s" % (
        name, d_tot, " ".join("%.1e" % v for v in d_loss), max(d_sm), " ".join("%.1e" % v for v in d_warp),
        " ".join("%.5f" % v for v in ov), " ".join("%.1e" % v for v in d_g), " ".join("%.1e" % v for v in d_pose)))
    assert d_tot < 5e-7
    assert max(d_loss) < 1e-6 and max(d_sm) < 1e-9
    assert max(d_warp) < 3e-5
    assert min(ov) > 0.9995
    assert max(d_g) < 3e-3, d_g
    for j, f in enumerate(fids[1:]):
        for g_, r, key in ((leaves[j][0].grad, ref["gaa"][f], "gaa"), (leaves[j][1].grad, ref["gtr"][f], "gtr")):
            assert float((g_ - r).abs().max()) < 1e-2 * float(r.abs().max()) + 1e-9, (key, f)


def check_sel(name, case, got, min_idx, gap_limit):
    """sel against the oracle's min_idx outside the pixels whose two smallest candidates lie within gap_limit (index
    convention of fs_photo_multi_*: 0..N-1 identity, N..2N-1 warped, 2N = a selected warped term whose sample missed,
    which the oracle's index does not have: it never wins next to an identity term)"""
    res = Q.oracle_chain(case)
    for s in range(4):
        close = Q.gap(Q.candidates(case, res, s)) < gap_limit
        bad = (got["sel"][s].long() != torch.as_tensor(min_idx[s]).long()) & ~close
        print("SEL %-10s scale %d: %d cells differ, %d excused of %d" % (name, s, int(bad.sum()), int(close.sum()), close.numel()))
        assert float(close.double().mean()) < 0.02
        assert not bool(bad.any()), (name, s, bad.nonzero()[:6].tolist())


@pytest.mark.parametrize("N", [1, 3, 4])
def test_chain_vs_reference_golden(dev, N):
    g = np.load(os.path.join(GOLD, "fisheye_nsrc.npz"))
    case = Q.make_case("golden-n%d" % N)
    tag = "n%d_" % N
    got = run_chain(dev, case)
    compare(case["name"], case, got, golden_reference(g, tag, case["fids"]))
    # the golden's min_idx carries the reference's tie-break noise: what a draw can reverse is excused
    check_sel(case["name"], case, got, [g[tag + "minidx_%d" % s] for s in range(4)], Q.NOISE_GAP)


@pytest.mark.parametrize("N", [1, 3, 4])
def test_ragged_shape_vs_oracle(dev, N):
    """66 x 70: ragged last strips in both directions, odd coarse maps; and the same run without pred / ov"""
    case = Q.make_case("ragged-n%d" % N)
    ref = oracle_reference(case)
    got = run_direct(dev, case)
    compare(case["name"], case, got, ref)
    check_sel(case["name"], case, got, ref["min_idx"], 1e-6)
    lean = run_direct(dev, case, want_pred=False)
    assert torch.equal(lean["sel"], got["sel"])


def test_two_frames_through_the_new_path_match_the_two_source_kernels(dev):
    """N = 2 on the inputs of tests/golden/fisheye.npz: force_multi=True (fs_photo_mei_multi_*) and the two-source
    kernels (fs_photo_fused_*) both meet the golden's bounds, and sel / ov agree outside the near-tie and fragile cells.
    Whether losses and pred are bit-equal is printed, not asserted: the two instantiations may contract differently."""
    g = np.load(os.path.join(GOLD, "fisheye.npz"))
    case = case_from_fisheye_golden(g, fisheye_chain_inputs(g))
    ref = dict(total=float(g["total_loss"]), loss=[float(g["ld_loss_%d" % s]) for s in range(4)],
               smooth=[float(g["ld_smooth_loss_%d" % s]) for s in range(4)],
               warp={1: torch.from_numpy(g["warp0_p"]), -1: torch.from_numpy(g["warp0_m"])},
               ov={1: g["ovmask0_p"], -1: g["ovmask0_m"]}, gdepth=[torch.from_numpy(g["gdepth_%d" % s]) for s in range(4)],
               gaa={1: torch.from_numpy(g["gaa_p"]), -1: torch.from_numpy(g["gaa_m"])},
               gtr={1: torch.from_numpy(g["gtr_p"]), -1: torch.from_numpy(g["gtr_m"])})
    new = run_chain(dev, case, force_multi=True)
    old = run_chain(dev, case)
    compare("n2-multi", case, new, ref)
    compare("n2-fused", case, old, ref)
    res = Q.oracle_chain(case)
    for s in range(4):
        close = Q.gap(Q.candidates(case, res, s)) < 1e-6
        frag = Q.fragile(case, s)
        assert not bool(((new["sel"][s] != old["sel"][s]) & ~close).any()), s
        assert not bool(((new["ov"][s] != old["ov"][s]) & ~frag).any()), s
    print("BITS n2: loss sums equal %s, loss vector equal %s, pred equal %s (largest difference %.2e), sel equal %s, ov equal %s" % (
        torch.equal(new["loss_sums"], old["loss_sums"]), torch.equal(new["out"], old["out"]),
        torch.equal(new["pred"], old["pred"]), float((new["pred"] - old["pred"]).abs().max()),
        torch.equal(new["sel"], old["sel"]), torch.equal(new["ov"], old["ov"])))


@pytest.mark.parametrize("N", [1, 3, 4])
def test_sources_equal_to_the_target(dev, N):
    """identical frames: every identity plane is exactly zero, index 0 wins everywhere (strict <), and nothing reaches
    d_depth or dT"""
    case = Q.make_case("ragged-n%d" % N)
    img0 = case["data"][("original_image", 0)]
    got = run_direct(dev, case, srcs=[img0.clone() for _ in range(N)])
    assert bool((got["ident"] == 0).all())
    assert int(got["sel"].max()) == 0
    assert all(bool((x == 0).all()) for x in got["d_depth"]) and all(bool((x == 0).all()) for x in got["dT"])


def test_two_runs_are_bit_identical(dev):
    case = Q.make_case("ragged-n4")
    a, b = run_direct(dev, case), run_direct(dev, case)
    assert torch.equal(a["sel"], b["sel"]) and torch.equal(a["ov"], b["ov"]) and torch.equal(a["pred"], b["pred"])
    assert torch.equal(a["loss_sums"], b["loss_sums"])


# ------------------------------------------------------------------------------------------------------- the model
def _model(H, W, dev, sd0, fids):
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.utils.builder import build
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    m = build(**meta_arch_cfg(H, W, with_pose=False, num_output_channels=64, max_depth=150.0, fisheye=True,
                              frame_ids=list(fids)))
    m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    return m.to(dev).train()


def _batch(B, H, W, seed, fids):
    """test_fisheye_gpu._fisheye_batch for a frame list"""
    data = O.synthetic_batch(B, H, W, seed=seed, frame_ids=tuple(fids))
    Ps, calibs = zip(*[FO.synthetic_calib(H, W, b % 2) for b in range(B)])
    data["P2"] = torch.stack(Ps, 0)
    data["calib_meta"] = list(calibs)
    for f in fids[1:]:
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, 0, 3] = 0.6 * f
        T[:, 2, 3] = 0.03
        data[("relative_pose", f)] = T
    return data


def _oracle_step(sd0, data, fids):
    """test_fisheye_gpu._oracle_step for a frame list"""
    sd = {k: v.clone().requires_grad_(O.is_param(k) and v.dtype.is_floating_point) for k, v in sd0.items()}
    feats = O.resnet_forward(sd, "depth_backbone.", data[("image", 0)])
    outputs = O.depth_decoder_forward(sd, "head.depth_decoder.", feats, 0.5, 150.0)
    for f in fids[1:]:
        outputs[("cam_T_cam", f)] = data[("relative_pose", f)]
    total, ld = FO.photometric_loss(outputs, data, frame_ids=tuple(fids))
    names = [k for k in sd if O.is_param(k)]
    grads = torch.autograd.grad(total, [sd[k] for k in names], allow_unused=True)
    return total.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("N", [1, 3])
def test_training_step_matches_oracle(dev, N):
    """MonoDepthWPose + FishEyeDecoder with frame_ids of length N + 1: loss and parameter gradients of a step against the
    oracle; N = 3: four hook steps, calibrations swapped between them, replayed from a hipGraph after two, against the
    same steps run eagerly"""
    from fsnet_amd.configs import training_cfg
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    fids = Q.FRAME_LISTS[N]
    B, H, W = 2, 64, 64
    sd0 = O.init_state(seed=5, with_pose=False, num_out=64, max_depth=150.0)
    m = _model(H, W, dev, sd0, fids)
    data = _batch(B, H, W, 61, fids)
    out = m(to_dev(data, dev), dict(is_training=True))
    out["loss"].backward()
    torch.cuda.synchronize()
    assert m.head._pl.multi and m.head._pl._be.name == "photo_mei_multi"
    total, raw = _oracle_step(sd0, data, fids)
    rel_loss = abs(float(out["loss"].detach()) - float(total)) / abs(float(total))
    gmax = max(float(r.norm()) for r in raw.values() if r is not None)
    worst = 0.0
    for k, p in m.named_parameters():
        ref = raw[k]
        if ref is None or float(ref.norm()) < 1e-3 * gmax:
            continue
        worst = max(worst, float((p.grad.cpu() - ref).norm() / ref.norm()))
    print("MODEL n%d loss rel %.2e worst parameter gradient rel %.2e" % (N, rel_loss, worst))
    assert rel_loss < 2e-5
    assert worst < 3e-2
    if N != 3:
        return
    losses = {}
    for graph_warmup in (99, 2):
        m2 = _model(H, W, dev, sd0, fids)
        tc = training_cfg()
        opt = build_optimizer(m2, name="adam", lr=1e-4, weight_decay=1e-5)
        hook = build(**dict(tc.training_hook, graph_warmup=graph_warmup))
        losses[graph_warmup] = []
        for it in range(4):
            d = _batch(B, H, W, 70 + it, fids)
            if it % 2:
                d["calib_meta"] = d["calib_meta"][::-1]
                d["P2"] = d["P2"].flip(0)
            o = hook(to_dev(d, dev), m2, opt)
            torch.cuda.synchronize()
            losses[graph_warmup].append(float(o["loss"].detach()))
        if graph_warmup == 2:
            assert hook.graph_replays >= 1
        t0, _ = _oracle_step(sd0, _batch(B, H, W, 70, fids), fids)
        assert abs(losses[graph_warmup][0] - float(t0)) < 2e-5 * abs(float(t0))
        assert all(np.isfinite(losses[graph_warmup]))
    print("MODEL n3 hook losses eager %s replayed %s" % (losses[99], losses[2]))
    for a, b in zip(losses[99], losses[2]):
        assert abs(a - b) < 1e-4 * abs(a)
