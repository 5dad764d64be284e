"""Pins tests/helpers_photo64n.py (the float64 photometric chain over N source frames) and the host side of the
N-frame loss path before a GPU test relies on them: against the two-frame helper at N = 2, against the fp32 oracle
for N = 1, 3, 4, the oracle against the real reference's recorded losses and gradients, the conditions of the sweep
for every input of tests/test_photo_multi_gpu.py, the argument checks of the new entry points, the register budget
of photo_multi.hip and MonoDepth2Decoder._check_options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import fsnet_oracle as O
from tests import helpers_photo64 as P
from tests import helpers_photo64n as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = Q.names()
ALL_NAMES = [n for k in "abcd" for n in NAMES[k]]


# --------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("name", ["a-32x120-B3", "d-32x120-motion_mask"])
def test_two_frames_give_the_two_frame_chain(name):
    case, opts = P.case_named(name)
    a, b = P.photo_chain(case, **opts), Q.photo_chain_n(case, **opts)
    for k in ("cand", "argmin", "pred", "ov", "ix", "iy", "jx", "jy", "g_depth", "g_up", "dT"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    assert torch.equal(a["loss_sums"], b["loss_sums"]) and torch.equal(a["total"], b["total"])
    ya, yb = P.yardsticks(case, opts), Q.yardsticks_n(case, opts)
    assert ya["delta"] == yb["delta"] and ya["e_depth"] == yb["e_depth"] and ya["e_dT"] == yb["e_dT"]
    assert all(torch.equal(x, y) for x, y in zip(ya["A"], yb["A"]))
    # (the inputs of the two-frame sweep were not made for the win-share condition: the shared ones only)
    assert [b for b in Q.check_conditions_n(case, opts, yb) if "candidate" not in b] == P.check_conditions(case, opts, ya) == []


def _oracle_case(data, depths, Ts, fids):
    return dict(B=data["P2"].shape[0], H=depths[0].shape[2], W=depths[0].shape[3],
                maps=tuple(tuple(d.shape[2:]) for d in depths), img0=data[("original_image", 0)].numpy(),
                src=[data[("original_image", f)].numpy() for f in fids[1:]],
                depths=[d.detach().numpy() for d in depths], P2=data["P2"].numpy(), T=[t.detach().numpy() for t in Ts],
                patched_mask=data["patched_mask"].numpy(), motion_mask=None)


@pytest.mark.parametrize("fids", [(0, -1), (0, -2, -1, 1), (0, -2, -1, 1, 2)])
def test_fp32_helper_vs_oracle(fids):
    """as tests/test_photo64_cpu.py holds the two-frame chain to the oracle: per-scale loss within 1e-6, warped images
    2e-5, the selection equal where the two best candidates are 1e-5 apart, depth gradient 2e-3 relative L2 — and the
    transform gradients, 2e-3 relative L2 as well"""
    B, H, W = 2, 32, 64
    N = len(fids) - 1
    data = O.synthetic_batch(B, H, W, seed=8, frame_ids=fids)
    g = torch.Generator().manual_seed(4)
    outputs, leaves = {}, []
    for s in range(4):
        d = (3 + 20 * torch.rand(B, 1, H >> s, W >> s, generator=g)).requires_grad_(True)
        leaves.append(d)
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = O.depth_to_disp(d.detach(), 0.5, 100.0)       # (detached: no smoothness gradient)
    Ts = [data[("relative_pose", f)].clone().requires_grad_(True) for f in fids[1:]]
    for f, T in zip(fids[1:], Ts):
        outputs[("cam_T_cam", f)] = T
    total, ld = O.photometric_loss(outputs, data, frame_ids=fids)
    total.backward()
    case = _oracle_case(data, leaves, Ts, fids)
    r = Q.photo_chain_n(case, dtype=torch.float32, sampler="grid_sample")
    denom = float(data["patched_mask"].sum()) + 1e-6
    got_total = 0.0
    for s in range(4):
        want = float(ld["loss/%d" % s]) - float(ld["smooth_loss/%d" % s])
        got = float(r["loss_sums"][s].sum()) / denom
        got_total += (got + float(ld["smooth_loss/%d" % s])) / 4
        print("N %d scale %d: loss %.8f oracle %.8f" % (N, s, got, want))
        assert abs(got - want) < 1e-6
        for k, fid in enumerate(fids[1:]):
            d = (r["pred"][s][k] - outputs[("original_image", fid, s)].detach()).abs().max()
            assert float(d) < 2e-5, (s, k, float(d))
        two = torch.topk(r["cand"][s], 2, dim=1, largest=False)[0]
        # the oracle's index has no code for "constant 100": there the term's own slot stands
        am = r["argmin"][s].clone()
        if bool((am == 2 * N).any()):
            am = torch.where(am == 2 * N, r["cand"][s].argmin(1), am)
        differ = (am != outputs[("min_idx", s)]) & ((two[:, 1] - two[:, 0]) >= 1e-5)
        assert not bool(differ.any()), s
        rel = float((r["g_depth"][s].float() - leaves[s].grad).norm() / leaves[s].grad.norm())
        print("N %d scale %d: depth gradient rel-L2 %.2e" % (N, s, rel))
        assert rel < 2e-3, (s, rel)
    assert abs(got_total - float(total.detach())) < 1e-6
    for k in range(N):
        rel = float((r["dT"][k].float() - Ts[k].grad).norm() / Ts[k].grad.norm())
        print("N %d frame %d: dT rel-L2 %.2e" % (N, k, rel))
        assert rel < 2e-3, (k, rel)


@pytest.mark.parametrize("N", [1, 3, 4])
def test_oracle_vs_reference_golden(N):
    """tests/golden/loss_chain_nsrc.npz (tools/gen_golden.py gen_loss_chain_nsrc): the real reference with 1, 3 and 4
    source frames, the oracle under the same tie-break noise.  Losses within 1e-6; gradients within 3e-3 relative L2, the
    bound tests/test_photo64_cpu.py holds the two-frame fixture to"""
    g = np.load(os.path.join(GOLD, "loss_chain_nsrc.npz"))
    tag = "n%d_" % N
    fids = tuple(int(f) for f in g[tag + "frame_ids"])
    assert len(fids) == N + 1
    T_ = lambda a: torch.from_numpy(np.asarray(a))
    data = {("original_image", f): T_(g[tag + "img_%d" % f]) for f in fids}
    data["P2"], data["patched_mask"] = T_(g[tag + "P2"]), T_(g[tag + "patched_mask"])
    outputs, dl, aas, trs = {}, [], {}, {}
    for s in range(4):
        d = T_(g[tag + "depth_%d" % s]).clone().requires_grad_(True)
        dl.append(d)
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
    for f in fids[1:]:
        aas[f] = T_(g[tag + "aa_%d" % f]).clone().requires_grad_(True)
        trs[f] = T_(g[tag + "tr_%d" % f]).clone().requires_grad_(True)
        outputs[("cam_T_cam", f)] = O.transformation_from_parameters(aas[f], trs[f], invert=(f < 0))
    # the reference's tie-break noise: the first draws after torch.manual_seed(0), one [B,N,H,W] per scale (:258-259)
    torch.manual_seed(0)
    noise = {s: torch.randn(2, N, int(g["H"]), int(g["W"])) * 0.00001 for s in range(4)}
    total, ld = O.photometric_loss(outputs, data, frame_ids=fids, noise=noise)
    total.backward()
    assert abs(float(total.detach()) - float(g[tag + "total_loss"])) < 1e-6
    for s in range(4):
        assert abs(float(ld["loss/%d" % s]) - float(g[tag + "ld_loss_%d" % s])) < 1e-6, s
        assert np.array_equal(outputs[("min_idx", s)].numpy().astype(np.uint8), g[tag + "minidx_%d" % s])
        assert int(g[tag + "minidx_%d" % s].max()) <= 2 * N - 1
        ref = T_(g[tag + "gdepth_%d" % s])
        rel = float((dl[s].grad - ref).norm() / ref.norm())
        print("N %d scale %d: gdepth rel-L2 %.2e" % (N, s, rel))
        assert rel < 3e-3, (s, rel)
    for f in fids[1:]:
        for got, key in ((aas[f].grad, "gaa_%d" % f), (trs[f].grad, "gtr_%d" % f)):
            ref = T_(g[tag + key])
            rel = float((got - ref).norm() / ref.norm())
            print("N %d %s rel-L2 %.2e" % (N, key, rel))
            assert rel < 3e-3, (key, rel)


# --------------------------------------------------------------------------------------------- the inputs
def test_shape_list_follows_the_strips():
    st = Q.strips()
    assert len(st) == 3 and all(c >= 2 and r >= 2 for c, r in st)
    sb = Q.shapes_b(st)
    hs, ws = [h for h, _ in sb], [w for _, w in sb]
    assert {2, 3} <= set(hs) and {2, 3} <= set(ws)
    for c, r in st:
        assert {c + 1, c + 2, c, 2 * c} <= set(ws), c          # one, two, exactly a full strip of columns in the last strip
        assert {r + 1, r} <= set(hs) and (r + 2 in hs or 2 * r + 2 in hs or any(h % r == 2 for h in hs)), r
    cols, rows = sorted({c for c, _ in st}), sorted({r for _, r in st})
    if len(cols) > 1 or len(rows) > 1:
        assert any(h > rows[-1] and w > cols[-1] for h, w in sb)      # the seams of two kernels both inside
    assert len(set(sb)) == len(sb)
    assert len(set(ALL_NAMES)) == len(ALL_NAMES)
    n1 = [n for n in NAMES["b"] if n.startswith("n1-")]
    assert len(n1) == 4 and sum(n.startswith("n3-") for n in NAMES["b"]) == len(sb) == sum(n.startswith("n4-") for n in NAMES["b"])


@pytest.mark.parametrize("name", ALL_NAMES)
def test_inputs_meet_the_conditions(name):
    case, opts = Q.case_named_n(name)
    y = Q.yardsticks_n(case, opts)
    assert Q.check_conditions_n(case, opts, y) == []
    for a in [case["img0"]] + case["src"]:
        assert a.min() >= 0.0 and a.max() <= 1.0
    assert all(d.min() >= 3.0 and d.max() <= 23.0 for d in case["depths"])
    assert 0.6 < case["patched_mask"].mean() < 0.8 or case["patched_mask"].size < 200


# --------------------------------------------------------------------------------------------- the C ABI
def _args(**kw):
    from fsnet_amd.hip.binding import FsPhotoMultiArgs
    a = FsPhotoMultiArgs()
    one = 0x1000                     # a non-NULL address that is never dereferenced: every call below must refuse first
    a.img0 = a.geo = a.ident = a.sel = a.loss_sums = a.mask_sum = a.dP = one
    for i in range(4):
        a.img_src[i] = a.depth[i] = a.d_depth[i] = one
        a.dh[i], a.dw[i] = 4, 4
    a.B, a.H, a.W, a.S, a.nsrc, a.noise_seed = 1, 8, 8, 1, 2, -1
    for k, v in kw.items():
        if k.startswith("img_src"):
            a.img_src[int(k[-1])] = v
        else:
            setattr(a, k, v)
    return a


def test_invalid_arguments_are_rejected_without_a_gpu():
    from fsnet_amd.hip import lib
    calls = (lib.fs_photo_multi_identity, lib.fs_photo_multi_fwd, lib.fs_photo_multi_bwd)
    bad = [dict(nsrc=0), dict(nsrc=5), dict(S=0), dict(S=5), dict(H=1), dict(W=1), dict(H=1 << 15, W=1 << 14),
           dict(img0=None), dict(geo=None), dict(img_src1=None), dict(B=0)]
    for fn in calls:
        assert fn(None, None) == 1
        for kw in bad:
            assert fn(C.byref(_args(**kw)), None) == 1, (fn.__name__, kw)
    assert lib.fs_photo_multi_identity(C.byref(_args(ident=None)), None) == 1
    assert lib.fs_photo_multi_identity(C.byref(_args(mask_sum=None)), None) == 1
    for kw in (dict(sel=None), dict(loss_sums=None), dict(ident=None), dict(pred=0x1000)):
        assert lib.fs_photo_multi_fwd(C.byref(_args(**kw)), None) == 1, kw
    for kw in (dict(sel=None), dict(dP=None), dict(mask_sum=None)):
        assert lib.fs_photo_multi_bwd(C.byref(_args(**kw)), None) == 1, kw
    a = _args()
    a.depth[0] = None
    assert lib.fs_photo_multi_fwd(C.byref(a), None) == 1 and lib.fs_photo_multi_bwd(C.byref(a), None) == 1
    a = _args()
    a.d_depth[0] = None
    assert lib.fs_photo_multi_bwd(C.byref(a), None) == 1
    one = 0x1000
    T = (C.c_void_p * 4)(one, one, one, one)
    assert lib.fs_photo_multi_setup(None, T, 2, one, 1, None, None) == 1
    assert lib.fs_photo_multi_setup(one, None, 2, one, 1, None, None) == 1
    assert lib.fs_photo_multi_setup(one, T, 2, None, 1, None, None) == 1
    assert lib.fs_photo_multi_setup(one, T, 0, one, 1, None, None) == 1
    assert lib.fs_photo_multi_setup(one, T, 5, one, 1, None, None) == 1
    assert lib.fs_photo_multi_setup(one, (C.c_void_p * 4)(one, None, None, None), 2, one, 1, None, None) == 1
    for args in ((None, one, one, 2, 1, 1, 1), (one, None, one, 2, 1, 1, 1), (one, one, None, 2, 1, 1, 1),
                 (one, one, one, 0, 1, 1, 1), (one, one, one, 5, 1, 1, 1), (one, one, one, 2, 1, 0, 1),
                 (one, one, one, 2, 1, 5, 1)):
        assert lib.fs_photo_multi_pose_grad(*args, None) == 1, args
    assert lib.fs_photo_multi_bwd_tiles(192, 640) == lib.fs_photo_fused_bwd_tiles(192, 640)
    assert lib.fs_photo_multi_bwd_tiles(1, 8) == -1 and lib.fs_photo_multi_bwd_tiles(8, 1) == -1
    c, r = C.c_int32(0), C.c_int32(0)
    assert lib.fs_photo_multi_strip(3, C.byref(c), C.byref(r)) == 1 and lib.fs_photo_multi_strip(-1, C.byref(c), C.byref(r)) == 1
    assert lib.fs_photo_multi_strip(0, None, C.byref(r)) == 1 and lib.fs_photo_multi_strip(0, C.byref(c), None) == 1


def test_photo_multi_kernels_do_not_spill(tmp_path):
    """photo_multi.hip compiled to assembly with the library's flags, as tests/test_no_spills_cpu.py compiles its kernels:
    the two resource-summary numbers of every kernel.  Setup, identity planes and pose gradient of the N-frame entry points
    are kernels of photometric.hip: the same two numbers over that file."""
    from fsnet_amd.csrc import build as Bd
    # photo_multi.hip: backward, 2 x forward; photometric.hip: setup, tile identity, pose-grad, identity rows x 2 policies
    for name, count in (("photo_multi", 3), ("photometric", 5)):
        src = os.path.join(Bd.HERE, name + ".hip")
        out = str(tmp_path / (name + ".s"))
        cmd = [Bd.HIPCC] + Bd.FLAGS + Bd.extra_flags(src) + ["--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        asm = open(out).read()
        spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)]
        scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", asm)]
        assert len(spills) == count and len(scratch) == count, (name, spills, scratch)
        assert all(v == 0 for v in spills), (name, spills)
        assert all(v <= 128 for v in scratch), (name, scratch)
        for k in (("photo_multi_bwd_kernel", "photo_multi_fwd_kernel") if name == "photo_multi" else
                  ("photo_setup_kernel", "photo_pose_grad_kernel", "photo_ident_rows_kernelINS_7NFrames")):
            assert k in asm, (name, k)


# --------------------------------------------------------------------------------------------- the decoder's options
def _decoder(cls, fids):
    from fsnet_amd.monodepth.networks.models.heads import monodepth2_decoder as M
    dec = getattr(M, cls).__new__(getattr(M, cls))
    torch.nn.Module.__init__(dec)
    dec.frame_ids = list(fids)
    return dec


@pytest.mark.parametrize("fids", [[0, -1], [0, 1, -1], [0, -2, -1, 1], [0, -2, -1, 1, 2]])
def test_check_options_accepts(fids):
    _decoder("MonoDepth2Decoder", fids)._check_options({})


@pytest.mark.parametrize("cls,fids,word", [("MonoDepth2Decoder", [0, "s"], "stereo"),
                                           ("MonoDepth2Decoder", [0, 1, 1], "once"),
                                           ("MonoDepth2Decoder", [0, 1, 0], "differ"),
                                           ("MonoDepth2Decoder", [0, -3, -2, -1, 1, 2], "at most"),
                                           ("FishEyeDecoder", [0, -1], "two")])
def test_check_options_refuses(cls, fids, word):
    with pytest.raises(NotImplementedError) as e:
        _decoder(cls, fids)._check_options({})
    assert word in str(e.value) and repr(fids) in str(e.value)
    if cls == "FishEyeDecoder":
        _decoder(cls, [0, 1, -1])._check_options({})
