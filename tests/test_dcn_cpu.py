"""CPU checks of the deformable convolution: the restatement of tests/helpers_dcn.py earns its place as the yardstick
(against F.conv2d, against an index-by-index gather, against its own numerical derivative), the module classes keep the
reference's names and shapes, what the kernels do not take is refused by name, the C ABI rejects bad arguments without
a device, the kernels do not spill, and every case the GPU tests use meets its input conditions."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import helpers_dcn as HD

GEOMETRIES = sorted({(str(kw.get("stride", 1)), str(kw.get("padding", 0)), str(kw.get("dilation", 1)), kw["R"])
                     for kw in HD.gpu_cases().values()})


@pytest.mark.parametrize("stride,padding,dilation,R", GEOMETRIES)
def test_zero_offsets_unit_mask_is_conv2d(stride, padding, dilation, R):
    stride, padding, dilation = eval(stride), eval(padding), eval(dilation)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 6, 9, 11, generator=gen, dtype=torch.float64)
    w = torch.randn(5, 6, R, R, generator=gen, dtype=torch.float64)
    b = torch.randn(5, generator=gen, dtype=torch.float64)
    Ho, Wo = HD.out_hw(9, 11, R, R, stride, padding, dilation)
    for dg in (1, 2):
        off = torch.zeros(2, dg * 2 * R * R, Ho, Wo, dtype=torch.float64)
        one = torch.ones(2, dg * R * R, Ho, Wo, dtype=torch.float64)
        want = F.conv2d(x, w, b, stride, padding, dilation)
        assert (HD.dcn_ref(x, off, one, w, b, stride, padding, dilation, dg) - want).abs().max() < 1e-12
        assert (HD.dcn_ref(x, off, None, w, None, stride, padding, dilation, dg) - (want - b[None, :, None, None])).abs().max() < 1e-12


def test_integer_offsets_are_a_shifted_gather():
    gen = torch.Generator().manual_seed(12)
    N, Ci, H, W, R, S = 1, 2, 5, 6, 3, 3
    x = torch.randn(N, Ci, H, W, generator=gen, dtype=torch.float64)
    off = torch.randint(-3, 4, (N, 2 * R * S, H, W), generator=gen).double()
    col = HD.dcn_columns(x, off, None, R, S, 1, 1, 1, 1)
    for tap in range(R * S):
        r, s = divmod(tap, S)
        for ho in range(H):
            for wo in range(W):
                h = ho - 1 + r + int(off[0, 2 * tap, ho, wo])
                w = wo - 1 + s + int(off[0, 2 * tap + 1, ho, wo])
                want = x[0, :, h, w] if 0 <= h < H and 0 <= w < W else torch.zeros(Ci, dtype=torch.float64)
                assert torch.equal(col[0, :, tap, ho, wo], want), (tap, ho, wo)


@pytest.mark.parametrize("v2", [False, True])
def test_restatement_gradcheck(v2):
    case = HD.make_case(seed=21, N=1, Ci=4, H=4, W=5, Co=3, R=3, S=3, stride=1, padding=1, dg=2, v2=v2, bias=v2)
    assert HD.sample_statistics(case)["min_int_dist"] > 1e-3
    leaves = [case[k].double().requires_grad_() for k in ("x", "offset", "mask", "weight", "bias") if case[k] is not None]

    def fn(*a):
        a = list(a)
        x, off = a.pop(0), a.pop(0)
        mask = a.pop(0) if v2 else None
        w = a.pop(0)
        b = a.pop(0) if v2 else None
        return HD.dcn_ref(x, off, mask, w, b, 1, 1, 1, 2)
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_bf16_hook_rounds_operands_and_passes_gradients():
    t = torch.tensor([1.0 + 2.0 ** -10, 3.0], dtype=torch.float64, requires_grad=True)
    r = HD.bf16_round(t)
    assert r[0].item() == 1.0 and r[1].item() == 3.0
    r.sum().backward()
    assert torch.equal(t.grad, torch.ones(2, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------------- module classes
def test_module_state_dict_keys_and_shapes():
    from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import (DeformConv, DeformConvPack, ModulatedDeformConv,
                                                        ModulatedDeformConvPack)
    sd = {k: tuple(v.shape) for k, v in DeformConv(8, 6, 3, padding=1).state_dict().items()}
    assert sd == {"weight": (6, 8, 3, 3)}
    sd = {k: tuple(v.shape) for k, v in DeformConvPack(8, 6, 3, padding=1, deformable_groups=2).state_dict().items()}
    assert sd == {"weight": (6, 8, 3, 3), "conv_offset.weight": (36, 8, 3, 3), "conv_offset.bias": (36,)}
    sd = {k: tuple(v.shape) for k, v in ModulatedDeformConv(8, 6, (3, 3), padding=1).state_dict().items()}
    assert sd == {"weight": (6, 8, 3, 3), "bias": (6,)}
    m = ModulatedDeformConvPack(8, 6, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sd == {"weight": (6, 8, 3, 3), "bias": (6,), "conv_offset.weight": (27, 8, 3, 3), "conv_offset.bias": (27,)}
    assert m._version == 2 and DeformConvPack._version == 2
    assert float(m.conv_offset.weight.detach().abs().max()) == 0.0
    assert float(m.conv_offset.bias.detach().abs().max()) == 0.0 and float(m.bias.detach().abs().max()) == 0.0
    bound = 1.0 / (8 * 9) ** 0.5
    assert 0.5 * bound < float(m.weight.detach().abs().max()) <= bound
    assert list(ModulatedDeformConv(8, 6, 3, bias=False).state_dict()) == ["weight"]


@pytest.mark.parametrize("cls", ["DeformConvPack", "ModulatedDeformConvPack"])
def test_legacy_offset_keys_load(cls):
    """the rename of deform_conv.py:344-359 / :469-485: `<module>_offset.*` becomes `<module>.conv_offset.*` when the
    state dict carries no version (or one below 2).  The hook itself is checked with a nested prefix; the whole
    load_state_dict path with the module as the root, where torch hands the hook the complete dictionary (it filters a
    child's dictionary by the child's prefix before the child's hook runs)."""
    from fsnet_amd.vision_base.networks.ops.dcn import deform_conv as dcn
    m = getattr(dcn, cls)(4, 4, 3, padding=1)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    nested ={"layer.conv2." + k: v for k, v in sd.items() if not k.startswith("conv_offset.")}
    nested["layer.conv2_offset.weight"] = torch.full_like(sd["conv_offset.weight"], 0.25)
    nested["layer.conv2_offset.bias"] = torch.full_like(sd["conv_offset.bias"], 0.25)
    missing, unexpected, errors = [], [], []
    m._load_from_state_dict(nested, "layer.conv2.", {}, True, missing, unexpected, errors)
    assert "layer.conv2.conv_offset.weight" in nested and "layer.conv2_offset.weight" not in nested
    assert "layer.conv2.conv_offset.bias" in nested and not errors
    versioned = {"layer.conv2_offset.weight": sd["conv_offset.weight"]}
    m._load_from_state_dict(versioned, "layer.conv2.", {"version": 2}, False, [], [], [])
    assert "layer.conv2_offset.weight" in versioned          # version 2 checkpoints are left alone
    legacy = {k.replace("conv_offset.", "_offset."): torch.full_like(v, 0.25) for k, v in sd.items()}
    assert "_offset.weight" in legacy and "conv_offset.weight" not in legacy
    m.load_state_dict(legacy)                       # a plain dict carries no version metadata: the old naming
    assert float(m.conv_offset.weight.detach().min()) == 0.25 and float(m.conv_offset.bias.detach().min()) == 0.25
    m.load_state_dict(sd)                           # the current naming still loads
    assert float(m.conv_offset.weight.detach().abs().max()) == 0.0


def test_unsupported_options_are_refused_by_name():
    from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import deform_conv, modulated_deform_conv
    x = torch.zeros(1, 8, 6, 6)
    with pytest.raises(NotImplementedError, match="groups"):
        deform_conv(x, torch.zeros(1, 18, 6, 6), torch.zeros(4, 4, 3, 3), 1, 1, 1, 2, 1)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        modulated_deform_conv(x, torch.zeros(1, 50, 6, 6), torch.zeros(1, 25, 6, 6), torch.zeros(4, 8, 5, 5), None, 1, 2, 1, 1, 1)
    with pytest.raises(NotImplementedError, match="stride"):
        deform_conv(x, torch.zeros(1, 18, 2, 2), torch.zeros(4, 8, 3, 3), 3, 1, 1, 1, 1)
    with pytest.raises(NotImplementedError, match="deformable_groups"):
        deform_conv(x, torch.zeros(1, 4 * 18, 6, 6), torch.zeros(4, 8, 3, 3), 1, 1, 1, 1, 4)
    with pytest.raises(NotImplementedError, match="padding"):
        deform_conv(x, torch.zeros(1, 18, 134, 134), torch.zeros(4, 8, 3, 3), 1, 65, 1, 1, 1)
    with pytest.raises(NotImplementedError, match="dilation"):
        deform_conv(x, torch.zeros(1, 18, 6, 6), torch.zeros(4, 8, 3, 3), 1, 1, 65, 1, 1)
    with pytest.raises(NotImplementedError, match="GPU"):
        deform_conv(x, torch.zeros(1, 18, 6, 6), torch.zeros(4, 8, 3, 3), 1, 1, 1, 1, 1)
    with pytest.raises(AssertionError, match="im2col"):
        deform_conv(torch.zeros(3, 8, 6, 6), torch.zeros(3, 18, 6, 6), torch.zeros(4, 8, 3, 3), 1, 1, 1, 1, 1, 2)


# --------------------------------------------------------------------------------------------------------------- C ABI
def _args(**kw):
    from fsnet_amd.hip.binding import FsDcnArgs
    a = FsDcnArgs()
    base = dict(N=1, H=6, W=6, Ho=6, Wo=6, Ci=8, Ci_p=8, Co=16, Co_p=16, R=3, S=3, stride_h=1, stride_w=1, pad_h=1,
                pad_w=1, dil_h=1, dil_w=1, groups=1, deformable_groups=1)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_abi_rejects_bad_arguments_without_a_device():
    from fsnet_amd.hip import lib
    for fn in (lib.fs_dcn_fwd, lib.fs_dcn_bwd_data, lib.fs_dcn_bwd_weight):
        assert fn(None, 0, None) == 1
        assert fn(C.byref(_args()), 0, None) == 1                    # NULL tensors
        assert fn(C.byref(_args()), 7, None) == 1                    # unknown dtype
    assert lib.fs_dcn_workspace_bytes(None, 0) == -1 and lib.fs_dcn_fwd_channels(None, 0) == -1
    assert lib.fs_dcn_fwd_channels(C.byref(_args()), 0) == 64 and lib.fs_dcn_fwd_channels(C.byref(_args(R=5)), 0) == -1
    assert lib.fs_dcn_fwd_channels(C.byref(_args(N=512, Co=300, Co_p=304)), 1) == 256      # 288 pixel tiles x 2
    assert lib.fs_dcn_fwd_channels(C.byref(_args(N=200, Co=300, Co_p=304)), 1) == 128      # 113 x 2 -> 113 x 3
    good = lib.fs_dcn_workspace_bytes(C.byref(_args()), 0)
    assert good >= 16 * 9 * 8 * 4 and good % 4 == 0
    for bad in (dict(groups=2), dict(R=5), dict(S=4), dict(stride_h=3), dict(stride_w=0), dict(pad_h=-1), dict(dil_w=0),
                dict(deformable_groups=0), dict(deformable_groups=3), dict(deformable_groups=4), dict(Ho=5),
                dict(Co_p=20), dict(Ci_p=6), dict(Ci=9), dict(N=0), dict(H=1, pad_h=0, Ho=1)):
        assert lib.fs_dcn_workspace_bytes(C.byref(_args(**bad)), 0) == -1, bad
    assert lib.fs_dcn_workspace_bytes(C.byref(_args(Ci_p=12, Ci=12)), 1) == -1       # bf16 channels come in eights
    assert lib.fs_dcn_workspace_bytes(C.byref(_args(deformable_groups=2)), 0) > 0    # 4 fp32 channels per group: a unit
    assert lib.fs_dcn_workspace_bytes(C.byref(_args(deformable_groups=2)), 1) == -1  # ... but half a bf16 unit
    px, ch = C.c_int32(), C.c_int32()
    assert lib.fs_dcn_tile(3, C.byref(px), C.byref(ch)) == 1 and lib.fs_dcn_tile(0, None, C.byref(ch)) == 1
    for which in (0, 1, 2):
        assert lib.fs_dcn_tile(which, C.byref(px), C.byref(ch)) == 0
        assert px.value in (32, 64) and ch.value % 64 == 0
    from fsnet_amd.hip import ops
    assert ops.dcn_tile(0)[0] == ops.dcn_tile(1)[0] == 64       # the pixel tile helpers_dcn.gpu_cases is written for


def test_dcn_kernels_do_not_spill(tmp_path):
    """dcn.hip compiled to assembly with the library's flags: no spilled register and (next to) no scratch in any of the
    13 kernels (forward, data backward, weight gradient x {bf16, fp32} x {v1, v2}, and the slab reduce); the float
    atomics are hardware adds, not compare-and-swap loops"""
    from fsnet_amd.csrc import build as Bd
    src = os.path.join(Bd.HERE, "dcn.hip")
    out = str(tmp_path / "dcn.s")
    cmd = [Bd.HIPCC] + Bd.FLAGS + Bd.extra_flags(src) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)]
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", asm)]
    assert len(spills) == 13 and len(scratch) == 13, (spills, scratch)
    assert all(v == 0 for v in spills), spills
    assert all(v <= 128 for v in scratch), scratch
    for k in ("dcn_fwd_kernel", "dcn_bwd_data_kernel", "dcn_bwd_weight_kernel", "dcn_wgrad_reduce_kernel"):
        assert k in asm, k
    assert "global_atomic_add_f32" in asm and "cmpswap" not in asm


# ------------------------------------------------------------------------------- the inputs of the GPU tests' cases
@pytest.mark.parametrize("name", sorted(HD.gpu_cases()))
def test_gpu_case_input_conditions(name):
    case = HD.make_case(**HD.gpu_cases()[name])
    st = HD.sample_statistics(case)
    assert st["min_int_dist"] > 1e-3, st      # floor and the -1 / H range tests are decided alike in f64, fp32, on the device
    assert st["outside"] >= 0.05 and st["partial"] >= 0.05 and st["full"] >= 0.5, st
    assert 0.0 < st["mask_min"] and st["mask_max"] < 1.0, st


def test_gpu_cases_cover_the_seams():
    kws = HD.gpu_cases().values()
    Ms = set()
    for kw in kws:
        Ho, Wo = HD.out_hw(kw["H"], kw["W"], kw["R"], kw["S"], kw.get("stride", 1), kw.get("padding", 0), kw.get("dilation", 1))
        Ms.add(kw["N"] * Ho * Wo)
    assert {1, 63, 64, 65, 131} <= Ms and max(Ms) > 3 * 131
    assert {16, 24, 64, 72, 128, 3} <= {kw["Ci"] for kw in kws} and {16, 24, 64, 72, 128, 5} <= {kw["Co"] for kw in kws}
    assert {1, 2} <= {kw.get("dg", 1) for kw in kws} and {True, False} <= {kw.get("v2", True) for kw in kws}
    assert {True, False} <= {kw.get("bias", True) for kw in kws}


def test_gpu_cases_reach_every_forward_channel_tile():
    """the forward owns fs_dcn_tile(0)'s 256 output channels per block only where the grid stays full without splitting
    them (fs_dcn_fwd_channels): some case must run at each of 256, 128 and 64, for both compute dtypes, with a
    part-filled last 64-channel tile at 128 and 256 and a second block along the channels at 256"""
    from fsnet_amd.hip import ops
    P, C = ops.dcn_tile(0)
    assert HD.gpu_cases(P, C) == HD.gpu_cases()
    for dtype in (torch.float32, torch.bfloat16):
        seen = {}
        for name, kw in HD.gpu_cases(P, C).items():
            geo = ops.DcnGeometry((kw["N"], kw["Ci"], kw["H"], kw["W"]), (kw["Co"], kw["Ci"], kw["R"], kw["S"]),
                                  kw.get("stride", 1), kw.get("padding", 0), kw.get("dilation", 1), 1, kw.get("dg", 1), dtype)
            seen.setdefault(geo.forward_channels(), []).append(geo)
        assert set(seen) == {C, C // 2, C // 4}, sorted(seen)
        for blk in (C, C // 2):
            assert any(g.Co_p % 64 != 0 and g.Co_p % blk != 0 for g in seen[blk]), blk     # a part-filled last tile
            assert any(g.N * g.Ho * g.Wo > 64 * P for g in seen[blk])                      # many pixel tiles
        assert any(g.Co_p > C for g in seen[C]) and any(C // 2 < g.Co_p <= C for g in seen[C])
        assert any(g.Co_p > C // 2 for g in seen[C // 2])
