"""The ConvNeXt backbone without a GPU: the module (keys, initialisation, the reference's quirks), its torch path against
tests/golden/convnext.npz — the reference's real classes run in f64 — and the new library entry points (declared, bound,
exported, refusing bad arguments, compiled without spills)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import helpers_convnext as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "convnext.npz")
SYMBOLS = ("fs_dwconv7_fwd", "fs_dwconv7_bwd_weight", "fs_dwconv7_workspace_bytes", "fs_dwconv7_tile", "fs_layernorm_fwd",
           "fs_layernorm_bwd", "fs_layernorm_workspace_bytes", "fs_gelu_fwd", "fs_gelu_bwd", "fs_scale_residual_fwd",
           "fs_scale_residual_bwd", "fs_scale_residual_workspace_bytes", "fs_bias_grad", "fs_patch_gather", "fs_patch_scatter")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLD) < (1 << 20)
    return np.load(GOLD)


@pytest.fixture(scope="module")
def cn():
    from fsnet_amd.vision_base.networks.models.backbone import convnext as mod
    return mod


def expected_keys(depths, dims, in_chans=3, layer_scale=True):
    """(key, shape) in registration order, written down independently of the module"""
    out = [("downsample_layers.0.0.weight", (dims[0], in_chans, 4, 4)), ("downsample_layers.0.0.bias", (dims[0],)),
           ("downsample_layers.0.1.weight", (dims[0],)), ("downsample_layers.0.1.bias", (dims[0],))]
    for i in range(1, 4):
        p = "downsample_layers.%d." % i
        out += [(p + "0.weight", (dims[i - 1],)), (p + "0.bias", (dims[i - 1],)),
                (p + "1.weight", (dims[i], dims[i - 1], 2, 2)), (p + "1.bias", (dims[i],))]
    for i in range(4):
        d = dims[i]
        for j in range(depths[i]):
            p = "stages.%d.%d." % (i, j)
            out += ([(p + "gamma", (d,))] if layer_scale else []) + [
                (p + "dwconv.weight", (d, 1, 7, 7)), (p + "dwconv.bias", (d,)), (p + "norm.weight", (d,)), (p + "norm.bias", (d,)),
                (p + "pwconv1.weight", (4 * d, d)), (p + "pwconv1.bias", (4 * d,)),
                (p + "pwconv2.weight", (d, 4 * d)), (p + "pwconv2.bias", (d,))]
    return out + [("norm.weight", (dims[3],)), ("norm.bias", (dims[3],))]


@pytest.mark.parametrize("name", list(HC.FACTORIES))
def test_factory_keys_shapes_and_order(cn, name):
    depths, dims = HC.FACTORIES[name]
    with torch.device("meta"):
        m = getattr(cn, name)(num_classes=5, head_init_scale=2.0, something_unknown=1)       # (swallowed)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == expected_keys(depths, dims)
    assert [k for k, _ in got] == [k for k, _ in m.named_parameters()]          # no buffers


def test_tiny_keys_match_the_reference_and_the_dispatcher(cn, gold):
    with torch.device("meta"):
        m = cn.convNext("ConvNeXt-T", pretrained=False, in_chans=6)
        xl = cn.convNext("convnext-xt", pretrained=False)
    assert list(m.state_dict()) == [str(k) for k in gold["init/keys"]]
    assert xl.downsample_layers[0][0].out_channels == 256
    with pytest.raises(KeyError):
        cn.convNext("convnext-xl", pretrained=False)
    import inspect
    assert inspect.signature(cn.convNext).parameters["pretrained"].default is True
    assert len(cn.model_urls) == 7 and all(v.startswith("https://dl.fbaipublicfiles.com/convnext/") for v in cn.model_urls.values())


def test_initial_state_under_the_fixture_seed(cn, gold):
    torch.manual_seed(HC.INIT_SEED)
    m = cn.convnext_tiny(in_chans=6)
    sums = np.array([float(v.double().sum()) for v in m.state_dict().values()])
    np.testing.assert_allclose(sums, gold["init/sums"], rtol=0, atol=1e-9)
    for mod in m.modules():
        if isinstance(mod, (nn.Conv2d, nn.Linear)):
            assert float(mod.bias.abs().max()) == 0.0 and float(mod.weight.abs().max()) <= 2.0
            assert 0.015 < float(mod.weight.std()) < 0.025
    assert all(float(b.gamma[0]) == pytest.approx(1e-6) for s in m.stages for b in s)


@pytest.fixture(scope="module")
def runs(cn):
    out = {}
    for which in HC.NETS:
        m = HC.build_net(cn, which)
        m.load_state_dict(HC.net_state(m, which), strict=True)
        x, cots = HC.net_inputs(which)
        out[which] = HC.run_net(m, x, cots, torch.float64) + (m,)
    return out


@pytest.mark.parametrize("which", list(HC.NETS))
def test_torch_path_reproduces_the_reference(gold, runs, which):
    feats, grads, none, m = runs[which]
    assert list(m.state_dict()) == [str(k) for k in gold[which + "/keys"]]
    assert none == [str(k) for k in gold[which + "/none_names"]] == ["norm.bias", "norm.weight"]
    assert m.norm.weight.grad is None and m.norm.bias.grad is None
    assert [tuple(f.shape) for f in feats] == HC.feature_shapes(which)
    for i, f in enumerate(feats):
        assert HC.deviation(f, torch.from_numpy(gold["%s/feat%d" % (which, i)]))[0] <= 1e-9, i
    full, gemm = [str(k) for k in gold[which + "/full_names"]], [str(k) for k in gold[which + "/gemm_names"]]
    assert sorted(full + gemm) == sorted(grads)
    for k in full:
        assert HC.deviation(grads[k], torch.from_numpy(gold["%s/grad/%s" % (which, k)]))[0] <= 1e-9, k
    proj = HC.projection_vectors([(k, tuple(grads[k].shape)) for k in gemm])
    for k, n, p in zip(gemm, gold[which + "/gemm_norm"], gold[which + "/gemm_proj"]):
        assert abs(float(grads[k].norm()) - n) <= 1e-9 and abs(float((grads[k] * proj[k]).sum()) - p) <= 1e-9, k


def test_quirks_kept_from_the_reference(cn):
    m = HC.build_net(cn, "odd")
    assert all(b.gamma is None and isinstance(b.drop_path, nn.Identity) for s in m.stages for b in s)
    assert m.forward_features(torch.zeros(1, 6, 32, 32)) is None
    assert isinstance(m.norm, nn.LayerNorm) and m.norm.eps == 1e-6
    d = HC.build_net(cn, "small", drop_path_rate=0.3)
    rates = [b.drop_path.drop_prob if not isinstance(b.drop_path, nn.Identity) else 0.0 for s in d.stages for b in s]
    assert rates == [r.item() for r in torch.linspace(0, 0.3, 6)] and isinstance(d.stages[0][0].drop_path, nn.Identity)
    with pytest.raises(NotImplementedError):
        cn.LayerNorm(8, data_format="nchw")
    # the two data formats are the same arithmetic
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, 24, generator=gen, dtype=torch.float64)
    a, b = cn.LayerNorm(24).double(), cn.LayerNorm(24, data_format="channels_first").double()
    w, bias = torch.randn(24, generator=gen, dtype=torch.float64), torch.randn(24, generator=gen, dtype=torch.float64)
    for ln in (a, b):
        ln.weight.data.copy_(w); ln.bias.data.copy_(bias)
    assert HC.deviation(a(x), b(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))[0] <= 1e-12
    # any size: the patch convolutions floor
    assert [tuple(f.shape[2:]) for f in HC.build_net(cn, "small")(torch.zeros(1, 3, 37, 50))] == [(9, 12), (4, 6), (2, 3), (1, 1)]


def test_out_indices_stop_the_stage_loop(cn):
    m = HC.build_net(cn, "small", out_indices=(1, 0))
    ran = []
    for i, s in enumerate(m.stages):
        s.register_forward_hook(lambda mod, a, o, i=i: ran.append(i))
    x = torch.randn(1, 3, 32, 32)
    feats = m(x)
    assert ran == [0, 1] and [f.shape[1] for f in feats] == [24, 40]        # (in stage order, whatever the tuple's)
    sum(f.sum() for f in feats).backward()
    for k, p in m.named_parameters():
        beyond = k.startswith(("stages.2", "stages.3", "downsample_layers.2", "downsample_layers.3", "norm."))
        assert (p.grad is None) == beyond, k


def test_drop_path_expression_under_a_seed(cn):
    from fsnet_amd.vision_base.networks.blocks.blocks import DropPath
    x = torch.randn(16, 3, 2, 2)
    dp = DropPath(0.3).train()
    torch.manual_seed(7)
    got = dp(x)
    torch.manual_seed(7)
    mask = (0.7 + torch.rand((16, 1, 1, 1))).floor_()
    assert torch.equal(got, x.div(0.7) * mask) and 0 < int(mask.sum()) < 16
    assert dp.eval()(x) is x and DropPath(0.).train()(x) is x


def test_library_declares_binds_and_exports_the_entry_points():
    from fsnet_amd.csrc import build as B
    from fsnet_amd.hip import binding
    from fsnet_amd.hip.signatures import SIGNATURES
    lib = C.CDLL(B.build(verbose=False))
    header = open(os.path.join(ROOT, "include", "fsnet_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        assert name in SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define FS_ABI_VERSION (\d+)", header).group(1)) == binding.ABI_VERSION == 15
    lib.fs_abi_version.restype = C.c_int
    assert lib.fs_abi_version() == 15


def test_bad_arguments_are_refused_without_a_device():
    from fsnet_amd.hip import binding as Bn, lib as L
    for fn in (L.fs_dwconv7_fwd, L.fs_dwconv7_bwd_weight, L.fs_layernorm_fwd, L.fs_layernorm_bwd, L.fs_scale_residual_fwd,
               L.fs_scale_residual_bwd):
        assert fn(None, 1, None) == 1
    d = Bn.FsDwconv7Args()
    d.x, d.wtab, d.out, d.dy, d.workspace, d.dw, d.workspace_bytes = 16, 32, 48, 64, 80, 96, 1 << 30
    d.N, d.H, d.W, d.C, d.Cp = 1, 4, 4, 24, 24
    assert L.fs_dwconv7_fwd(C.byref(d), 7, None) == 1                      # unknown dtype
    d.Cp = 20
    assert L.fs_dwconv7_fwd(C.byref(d), 1, None) == 1                      # Cp < C
    d.Cp = 28
    assert L.fs_dwconv7_fwd(C.byref(d), 1, None) == 1 and L.fs_dwconv7_bwd_weight(C.byref(d), 1, None) == 1   # no whole bf16 unit
    d.Cp, d.out = 32, 50
    assert L.fs_dwconv7_fwd(C.byref(d), 1, None) == 1                      # misaligned
    d.out, d.workspace_bytes = 48, 16
    assert L.fs_dwconv7_bwd_weight(C.byref(d), 1, None) == 1               # workspace too small
    assert L.fs_dwconv7_workspace_bytes(0, 4, 4, 32) == -1 and L.fs_dwconv7_workspace_bytes(1, 4, 4, 32) > 0
    assert L.fs_dwconv7_tile(7, None, None, None) == 1
    n = Bn.FsLayerNormArgs()
    n.x, n.y, n.gamma, n.beta, n.mean, n.rstd, n.dy, n.dx = 16, 32, 48, 64, 80, 96, 112, 128
    n.M, n.C, n.Cp, n.eps = 4, 24, 28, 1e-6
    assert L.fs_layernorm_fwd(C.byref(n), 1, None) == 1 and L.fs_layernorm_bwd(C.byref(n), 1, None) == 1
    n.Cp, n.M = 32, 0
    assert L.fs_layernorm_fwd(C.byref(n), 1, None) == 1
    n.M, n.C, n.Cp = 4, 4100, 4112
    assert L.fs_layernorm_fwd(C.byref(n), 1, None) == 1                    # more than 64 lanes x 8 units
    n.C, n.Cp, n.dgamma = 24, 32, 144
    assert L.fs_layernorm_bwd(C.byref(n), 1, None) == 1                    # a parameter gradient without a workspace
    assert L.fs_layernorm_workspace_bytes(0, 32) == -1 and L.fs_scale_residual_workspace_bytes(5, 0) == -1
    s = Bn.FsScaleResidualArgs()
    s.inp, s.z, s.out, s.dout, s.dz = 16, 32, 48, 64, 80
    s.N, s.HW, s.C, s.Cp = 2, 0, 24, 32
    assert L.fs_scale_residual_fwd(C.byref(s), 1, None) == 1 and L.fs_scale_residual_bwd(C.byref(s), 1, None) == 1
    s.HW, s.dgamma = 4, 96
    assert L.fs_scale_residual_bwd(C.byref(s), 1, None) == 1               # dgamma without gamma / workspace
    s.dgamma, s.dbias = None, 96
    assert L.fs_scale_residual_bwd(C.byref(s), 1, None) == 1               # dbias without workspace
    assert L.fs_gelu_fwd(None, 16, 8, 1, None) == 1 and L.fs_gelu_fwd(16, 32, 0, 1, None) == 1
    assert L.fs_gelu_bwd(16, None, 48, 8, 1, None) == 1 and L.fs_gelu_bwd(16, 32, 50, 8, 1, None) == 1
    assert L.fs_patch_gather(16, 32, 1, 8, 8, 12, 2, 1, None) == 1         # 12 channels: no whole bf16 unit
    assert L.fs_patch_gather(16, 32, 1, 8, 8, 16, 9, 1, None) == 1 and L.fs_patch_scatter(16, 32, 1, 1, 8, 16, 2, 1, None) == 1
    assert L.fs_patch_scatter(None, 32, 1, 8, 8, 16, 2, 1, None) == 1
    assert L.fs_bias_grad(16, 32, 48, 1 << 20, 4, 24, 28, 0, 0, 1, None) == 1 and L.fs_bias_grad(16, 32, None, 0, 4, 24, 32, 0, 0, 1, None) == 1
    assert L.fs_bias_grad(16, 32, 48, 8, 4, 24, 32, 0, 0, 1, None) == 1        # workspace too small


def test_convnext_kernels_do_not_spill(tmp_path):
    """convnext.hip compiled to assembly with the library's flags: no spilled register and (next to) no scratch in any
    kernel; in particular the weight gradient does not hold 49 x 8 accumulators per thread"""
    from fsnet_amd.csrc import build as Bd
    src = os.path.join(Bd.HERE, "convnext.hip")
    out = str(tmp_path / "convnext.s")
    cmd = [Bd.HIPCC] + Bd.FLAGS + Bd.extra_flags(src) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)]
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", asm)]
    assert len(spills) == len(scratch) == 36, (len(spills), len(scratch))
    assert all(v == 0 for v in spills), spills
    assert all(v <= 128 for v in scratch), scratch
    for k in ("dwconv7_fwd_kernel", "dwconv7_wgrad_kernel", "dwconv7_wgrad_reduce_kernel", "ln_fwd_kernel", "ln_bwd_kernel",
              "ln_bwd_param_kernel", "slab_reduce_kernel", "gelu_kernel", "scale_residual_fwd_kernel",
              "scale_residual_bwd_kernel", "bias_grad_kernel", "patch_kernel"):
        assert k in asm, k
