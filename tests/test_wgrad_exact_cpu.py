"""The exact-integer weight-gradient helper against float64 autograd of F.conv2d (the ATen op the reference calls), its
2^24 guard, and the launchers' geometry for every case of the GPU sweep (tests/test_wgrad_exact_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_wgrad_exact as WX

SMALL = [WX.Case(3, 64, 7, 2, 3, 2, 32, 64), WX.Case(24, 64, 3, 1, 1, 3, 11, 13), WX.Case(16, 16, 3, 1, 0, 2, 13, 19),
         WX.Case(64, 128, 1, 2, 0, 2, 16, 32), WX.Case(32, 64, 3, 1, 1, 3, 23, 37), WX.Case(40, 96, 3, 2, 1, 3, 11, 13)]


def autograd_dw(x_nchw, dy_nchw, case, dtype=torch.float64):
    w = torch.zeros(case.Co, case.Ci, case.k, case.k, dtype=dtype, requires_grad=True)
    F.conv2d(x_nchw.to(dtype), w, None, stride=case.stride, padding=case.pad).backward(dy_nchw.to(dtype))
    return w.grad


@pytest.mark.parametrize("case", SMALL)
def test_reference_equals_autograd_on_random_normal_inputs(case):
    d = WX.dims(case, torch.bfloat16)
    g = torch.Generator().manual_seed(5 + case.Ci)
    x = torch.randn(case.N, case.Ci, case.H, case.W, generator=g, dtype=torch.float64)
    dy = torch.randn(case.N, case.Co, d.Ho, d.Wo, generator=g, dtype=torch.float64)
    got, ref = WX.wgrad_f64(x, dy, case.k, case.stride, case.pad), autograd_dw(x, dy, case)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", SMALL)
def test_integer_case_is_exact(case, dtype):
    ic = WX.integer_case(case, dtype, 3)
    d = ic.d
    # non-zero integers everywhere, the padded channels included; exact in the compute type
    for t, amax in ((ic.x, WX.X_MAX), (ic.dy, WX.DY_MAX)):
        assert bool((t != 0).all()) and bool((t == t.round()).all()) and float(t.abs().max()) == amax
        assert torch.equal(t.to(dtype).float(), t)
    assert ic.x.shape[3] == d.Ci_p and ic.dy.shape[3] == d.Co_p
    assert bool((ic.dw0 == ic.dw0.round()).all()) and float(ic.dw0.abs().max()) <= WX.DW0_MAX
    ref = autograd_dw(ic.x[..., :case.Ci].permute(0, 3, 1, 2), ic.dy[..., :case.Co].permute(0, 3, 1, 2), case)
    assert torch.equal(ic.dw, ref)
    # fp32 arithmetic on these integers is exact as well, in torch's own summation order
    ref32 = autograd_dw(ic.x[..., :case.Ci].permute(0, 3, 1, 2), ic.dy[..., :case.Co].permute(0, 3, 1, 2), case, torch.float32)
    assert ref32.dtype == torch.float32 and torch.equal(ref32.double(), ic.dw)
    for calls in (1, 2):
        assert torch.equal(ic.expected(calls).double(), ic.dw0.double() + calls * ref)


@pytest.mark.parametrize("case", WX.PROLOGUE_CASES)
@pytest.mark.parametrize("G,relu", [(1, False), (1, True), (2, False), (2, True)])
def test_prologue_form_equals_autograd_through_affine_and_relu(case, G, relu):
    ic = WX.integer_case(case, torch.bfloat16, 11, (G, relu))
    scale, shift, r = ic.pro
    assert r == relu and bool((shift != 0).any()) and scale.shape == (G, ic.d.Ci_p)
    n = case.N // G
    x = ic.x.double()
    w = torch.zeros(case.Co, case.Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    for g in range(G):
        xa = x[g * n:(g + 1) * n] * scale[g].double() + shift[g].double()
        xa = F.relu(xa) if relu else xa
        y = F.conv2d(xa.permute(0, 3, 1, 2), w, None, stride=1, padding=case.pad)       # the padding is zero, not `shift`
        y.backward(ic.dy[g * n:(g + 1) * n].permute(0, 3, 1, 2).double())
    assert torch.equal(ic.dw, w.grad)
    xe = WX.apply_prologue(ic.x, scale, shift, relu)
    assert torch.equal(xe.to(torch.bfloat16).double(), xe)               # x' is exact in bf16 as well


def test_guard_fires_on_an_oversized_case():
    WX.assert_exact(1 << 20, WX.X_MAX, WX.DY_MAX, WX.DW0_MAX, 2)
    with pytest.raises(AssertionError, match="2\\^24"):
        WX.assert_exact(1 << 21, WX.X_MAX, WX.DY_MAX, WX.DW0_MAX, 2)
    with pytest.raises(AssertionError, match="2\\^24"):                 # (raised before anything is generated)
        WX.IntCase(WX.Case(8, 16, 1, 1, 0, 1, 1200, 1250), torch.bfloat16, 0)


def test_geometry_of_every_table_case():
    rows = WX.all_table_cases()
    assert len(rows) > 50
    for path, case, dtype in rows:
        d, m = WX.dims(case, dtype), WX.path_model(case, dtype)
        assert m.path == path, (path, case, m)
        assert case.N >= 1 and d.Ho >= 1 and d.Wo >= 1
        # whole slabs: integer rows x columns that cover the padded gradient, columns in whole float4
        assert isinstance(m.slab, int) and m.slab == m.ws_rows * m.ws_cols and m.slab > 0
        assert m.ws_rows >= d.Co_p and m.ws_cols >= d.ncols and m.ws_cols % 4 == 0
        assert (m.tiles >= 1) == (path != "stem")
        if m.chunk:
            assert m.ws_rows % 16 == 0 and m.ws_cols % 64 == 0
        WX.assert_exact(d.M, 2 * WX.X_MAX + 1, WX.DY_MAX, WX.DW0_MAX, 2)
        # the sweep's largest forced count fits the 32 MB workspace
        assert 129 * m.slab <= (1 << 23) or path not in ("narrow",)
    # pixel counts that are no multiple of 64 wherever a kernel splits by chunks, so the last split is short
    for sw in WX.SWEEP_CASES:
        m = WX.path_model(sw.case, sw.dtype)
        if m.chunk:
            assert WX.dims(sw.case, sw.dtype).M % 64 != 0
        assert set(sw.reductions) <= {"reduce3x3", "flat", "reduce4", "reduce"}
    assert {r for sw in WX.SWEEP_CASES for r in sw.reductions} == {"reduce3x3", "flat", "reduce4", "reduce"}
    assert [WX.stem_blocks(WX.Case(6, 64, 7, 2, 3, 3, 64, 96), k) for k in (1, 7, 8, 16, 33, 36)] == [1, 6, 8, 12, 18, 36]
    # a stem without a workspace is not the stem kernel's
    assert WX.path_model(WX.Case(6, 64, 7, 2, 3, 3, 64, 96), torch.bfloat16, workspace=False).path == "tile64w"


def test_reduce_rule_and_forced_args():
    assert WX.reduce_kernel(1, 576, 3) == "none" and WX.reduce_kernel(1, 392, 7, always=True) == "flat"
    assert [WX.reduce_kernel(n, 288, 3) for n in (2, 8, 9, 16, 17, 31, 32)] == ["flat"] * 2 + ["reduce4"] * 4 + ["reduce"]
    assert [WX.reduce_kernel(n, 576, 3) for n in (2, 16, 17, 32)] == ["reduce3x3", "reduce3x3", "reduce4", "reduce"]
    assert [WX.reduce_kernel(n, 144, 3) for n in (2, 31, 129)] == ["reduce4", "reduce4", "reduce"]
    assert WX.chunked_splits(9063, 32, 33) == 32 and WX.chunked_splits(9063, 32, 17) == 17
    case, dt = WX.Case(24, 64, 3, 1, 1, 3, 11, 13), torch.float32
    ic = WX.integer_case(case, dt, 1)
    ws = torch.zeros(1 << 16)
    buf, dw = WX.guarded(ic.dw0, "cpu")
    sp = WX.make_spec(case, dt, ic.x, ic.dy, dw, WX.make_ktab(case, dt), ws)
    assert torch.equal(dw, ic.dw0) and WX.guards_intact(buf) and buf.numel() == ic.dw0.numel() + 2 * WX.GUARD
    a = WX.forced_split_args(sp, 3)
    assert a.workspace == ws.data_ptr() and a.workspace_elems == 3 * sp.model.slab and sp.a.workspace_elems == ws.numel()
    a = WX.forced_split_args(sp, 0)
    assert not a.workspace and a.workspace_elems == 0 and a.dw == sp.a.dw and a.x_bytes == sp.a.x_bytes
    assert WX.forced_split_args(sp, "full").workspace_elems == ws.numel()
    buf[0] = 0.0
    assert not WX.guards_intact(buf)
