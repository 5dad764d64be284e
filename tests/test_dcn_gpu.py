"""Deformable convolution on the GPU against the f64 restatement of tests/helpers_dcn.py.

Every quantity (out, d_x, d_offset, d_mask, dW, d_bias) of every case is held to F * e, where e is the deviation from
the f64 restatement of the SAME restatement run in fp32 on the CPU (fp32 compute), or run in f64 with the bf16 rounding
hook on its GEMM operands (bf16 compute).  A deviation is measured twice, as the largest absolute difference and as
the root mean square, and the ratio of a quantity is the larger of the two ratios.  bf16 compute also stores `out` in
bf16: that one rounding (half an ulp, 2^-9 relative) is no part of e, so it is taken off |out - reference| element by
element before the ratio is formed — the allowance of the storage format, nothing else.

F per quantity is twice the worst ratio measured on an MI355X, rounded up (the margin is for the summation order of
the MFMA accumulators and of the float atomics behind d_x).  Measured worst ratios (RATIO lines of this file):
            out    d_x       d_offset  d_mask  dW     d_bias
    fp32    2.83   1.60      1.35      1.32    1.24   1.99      (out: 5x7_c128_c72_d2_p2_v1_dg2, K = 1152; dW: integer offsets;
                                                                 d_bias: co_full_tile_part, 16384 pixels)
    bf16    2.74   1.00012   1.95      1.47    1.68   1.00003   (out: m63_c24_k3_p1; d_offset: co_full_tile_part)
(bf16 d_x and d_bias are dominated by the rounding of dY, which the yardstick shares: their ratios sit a hair above 1, so
twice the worst is a hair above 2 and rounds up to 3.)  Typical ratios are 1.0 - 1.2; the zero-offset, integer-offset,
public-function and graph-replay tests stay below these.
Without the storage allowance the bf16 `out` ratio ("out_raw" in the RATIO lines, printed and not bounded) is 1.4 - 5.7,
worst 5.68 (m63_c24_k3_p1): the plain rule would need F = 12 for that one quantity, all of it the half ulp of the bf16
store on outputs of size |bias| ~ 1.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_dcn as HD

pytestmark = pytest.mark.gpu

FACTOR = {
    "fp32": {"out": 6, "d_x": 4, "d_offset": 3, "d_mask": 3, "dW": 3, "d_bias": 4},
    "bf16": {"out": 6, "d_x": 3, "d_offset": 4, "d_mask": 3, "dW": 4, "d_bias": 3},
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAMES = sorted(HD.gpu_cases())
BF16_HALF_ULP = 2.0 ** -9


def gpu_run(case, dtype, dev):
    """the three kernels through the host wrappers, every output buffer pre-filled with NaN -> ({quantity: f64 CPU
    tensor in the restatement's layout}, raw device buffers)"""
    from fsnet_amd.hip import ops
    nan = float("nan")
    w = case["weight"].to(dev)
    geo = ops.DcnGeometry(case["x"].shape, w.shape, case["stride"], case["padding"], case["dilation"], 1, case["dg"], dtype)
    x = ops.nchw_to_nhwc(case["x"].to(dev), None, geo.Ci_p, dtype)
    dy = ops.nchw_to_nhwc(case["dy"].to(dev), None, geo.Co_p, dtype)
    off = case["offset"].to(dev)
    mask = case["mask"].to(dev) if case["mask"] is not None else None
    bias = case["bias"].to(dev) if case["bias"] is not None else None
    out = torch.full((geo.N, geo.Ho, geo.Wo, geo.Co_p), nan, dtype=dtype, device=dev)
    ops.dcn_forward(geo, x, off, mask, ops.dcn_pack(geo, w, 0), bias, out=out)
    dx = torch.full((geo.N, geo.H, geo.W, geo.Ci_p), nan, dtype=torch.float32, device=dev)
    d_off = torch.full_like(off, nan)
    d_mask = torch.full_like(mask, nan) if mask is not None else None
    ops.dcn_backward_data(geo, x, off, mask, ops.dcn_pack(geo, w, 1), dy, dx=dx, d_offset=d_off, d_mask=d_mask)
    dw = torch.full_like(w, nan)
    d_bias = torch.full_like(bias, nan) if bias is not None else None
    ops.dcn_backward_weight(geo, x, off, mask, dy, want_bias=bias is not None, dw=dw, d_bias=d_bias)
    torch.cuda.synchronize()
    raw = {"out": out, "d_x": dx, "d_offset": d_off, "d_mask": d_mask, "dW": dw, "d_bias": d_bias}
    # the padded channels: exact zeros in the forward output and in d_x
    assert float(out[..., geo.Co:].float().abs().sum()) == 0.0 and float(dx[..., geo.Ci:].abs().sum()) == 0.0
    got = {"out": out[..., :geo.Co].permute(0, 3, 1, 2), "d_x": dx[..., :geo.Ci].permute(0, 3, 1, 2), "d_offset": d_off,
           "d_mask": d_mask, "dW": dw, "d_bias": d_bias}
    return {k: (v.double().cpu() if v is not None else None) for k, v in got.items()}, raw


def ratios(got, ref64, yard, bf16):
    """{quantity: (ratio, e_max)}: the deviation of `got` from the f64 reference over the yardstick's deviation;
    "out_raw" (bf16 only, printed, not bounded): the ratio of `out` without the storage-rounding allowance"""
    res = {}
    for q in HD.QUANTITIES:
        if ref64[q] is None:
            assert got[q] is None
            continue
        assert got[q].shape == ref64[q].shape, (q, got[q].shape, ref64[q].shape)
        assert bool(torch.isfinite(got[q]).all()), "%s: a cell was never written (NaN pre-fill) or is not finite" % q
        d = (got[q] - ref64[q].double()).abs()
        e_max, e_rms = HD.deviation(yard[q], ref64[q])
        if bf16 and q == "out":
            res["out_raw"] = (max(float(d.max()) / e_max, float(d.pow(2).mean().sqrt()) / e_rms), e_max)
            d = (d - BF16_HALF_ULP * ref64[q].double().abs()).clamp(min=0)
        d_max, d_rms = float(d.max()), float(d.pow(2).mean().sqrt())
        if e_max == 0.0:
            res[q] = (0.0 if d_max == 0.0 else float("inf"), e_max)
        else:
            res[q] = (max(d_max / e_max, d_rms / e_rms), e_max)
    return res


def check(name, tag, got, ref64, yard):
    r = ratios(got, ref64, yard, tag == "bf16")
    print("RATIO %-28s %s %s" % (name, tag, " ".join("%s %.2f (e %.1e)" % (q, v[0], v[1]) for q, v in r.items())))
    bad = {q: v for q, v in r.items() if q != "out_raw" and not v[0] <= FACTOR[tag][q]}
    assert not bad, "%s %s: ratio above F for %s" % (name, tag, bad)
    return r


@pytest.mark.parametrize("tag", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_against_f64_restatement(dev, name, tag):
    case, ref64, ref32, refbf = HD.case_and_refs(name)
    got, _ = gpu_run(case, DTYPES[tag], dev)
    check(name, tag, got, ref64, ref32 if tag == "fp32" else refbf)


@pytest.mark.parametrize("tag", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["n3_13x29_c64_c16_dg2", "m65_c72_k3_v1", "co_full_tile_two_blocks"])
def test_two_runs_are_bit_identical(dev, name, tag):
    """out, d_offset, d_mask, dW and d_bias bit for bit; d_x is summed with float atomics: within its bound both times"""
    case, ref64, ref32, refbf = HD.case_and_refs(name)
    a, _ = gpu_run(case, DTYPES[tag], dev)
    b, _ = gpu_run(case, DTYPES[tag], dev)
    for q in ("out", "d_offset", "d_mask", "dW", "d_bias"):
        if a[q] is not None:
            assert torch.equal(a[q], b[q]), q
    check(name, tag, a, ref64, ref32 if tag == "fp32" else refbf)
    check(name, tag, b, ref64, ref32 if tag == "fp32" else refbf)


def test_zero_offsets_are_the_plain_convolution(dev):
    kw = dict(HD.gpu_cases()["n3_33x20_c16_c128_s2"])
    case = HD.make_case(**kw)
    case["offset"] = torch.zeros_like(case["offset"])
    case["mask"] = torch.ones_like(case["mask"])
    want64 = F.conv2d(case["x"].double(), case["weight"].double(), None, case["stride"], case["padding"], case["dilation"])
    want32 = F.conv2d(case["x"], case["weight"], None, case["stride"], case["padding"], case["dilation"])
    got, _ = gpu_run(case, torch.float32, dev)
    e_max, e_rms = HD.deviation(want32, want64)
    d_max, d_rms = HD.deviation(got["out"], want64)
    ratio = max(d_max / e_max, d_rms / e_rms)
    print("RATIO zero_offsets fp32 out %.2f (e %.1e)" % (ratio, e_max))
    assert ratio <= FACTOR["fp32"]["out"]


def _integer_case():
    """every sample at an integer position, the edge positions -1, 0, H-1 and H (W likewise) included many times over"""
    kw = dict(seed=31, N=2, Ci=16, H=6, W=7, Co=16, R=3, S=3, stride=1, padding=1, dilation=1, dg=1)
    case = HD.make_case(**kw)
    gen = torch.Generator().manual_seed(32)
    Ho, Wo = case["offset"].shape[2:]
    zero = torch.zeros(2, 18, Ho, Wo, dtype=torch.float64)
    bh, bw = HD.sample_coords(zero, 6, 7, 3, 3, 1, 1, 1, 1)
    th = torch.tensor([-1.0, 0.0, 5.0, 6.0, 2.0, 3.0])[torch.randint(0, 6, bh.shape, generator=gen)].double()
    tw = torch.tensor([-1.0, 0.0, 6.0, 7.0, 1.0, 4.0])[torch.randint(0, 6, bw.shape, generator=gen)].double()
    case["offset"] = torch.stack([th - bh, tw - bw], dim=3).reshape(2, 18, Ho, Wo).float()
    return case


def test_exact_integer_offsets(dev):
    case = _integer_case()
    h, w = HD.sample_coords(case["offset"].double(), 6, 7, 3, 3, 1, 1, 1, 1)
    assert bool((h == h.round()).all()) and bool((w == w.round()).all())
    for v in (-1.0, 0.0, 5.0, 6.0):
        assert int((h == v).sum()) > 20
    for v in (-1.0, 0.0, 6.0, 7.0):
        assert int((w == v).sum()) > 20
    ref64, ref32 = HD.run_ref(case, torch.float64), HD.run_ref(case, torch.float32)
    got, _ = gpu_run(case, torch.float32, dev)
    check("integer_offsets", "fp32", got, ref64, ref32)


@pytest.mark.parametrize("tag", ["fp32", "bf16"])
def test_all_samples_outside(dev, tag):
    case = HD.make_case(seed=41, N=2, Ci=24, H=7, W=9, Co=24, R=3, S=3, padding=1)
    case["offset"] = torch.full_like(case["offset"], 1000.0)
    got, raw = gpu_run(case, DTYPES[tag], dev)
    bias = case["bias"].to(DTYPES[tag]).double()
    assert torch.equal(got["out"], bias[None, :, None, None].expand_as(got["out"]))
    assert float(raw["d_x"].abs().sum()) == 0.0              # every cell of the buffer, padded channels included
    for q in ("d_x", "d_offset", "d_mask", "dW"):
        assert float(got[q].abs().sum()) == 0.0, q
    want = case["dy"].to(DTYPES[tag]).double().sum(dim=(0, 2, 3))
    assert (got["d_bias"] - want).abs().max() <= 1e-5 * want.abs().max()


def _public(case, dev, tag, frozen=()):
    """forward and backward through the public autograd functions -> (out, {name: leaf})"""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import deform_conv, modulated_deform_conv
    RT.set_compute_dtype(tag)
    t = {k: case[k].to(dev).requires_grad_(k not in frozen) for k in ("x", "offset", "mask", "weight", "bias")
         if case[k] is not None}
    if case["mask"] is not None:
        out = modulated_deform_conv(t["x"], t["offset"], t["mask"], t["weight"], t.get("bias"), case["stride"],
                                    case["padding"], case["dilation"], 1, case["dg"])
    else:
        out = deform_conv(t["x"], t["offset"], t["weight"], case["stride"], case["padding"], case["dilation"], 1, case["dg"])
    return out, t


@pytest.fixture
def restore_dtype():
    from fsnet_amd.engine.runtime import RT
    before = RT.compute_dtype
    yield
    RT.set_compute_dtype(before)


@pytest.mark.parametrize("name", ["n3_13x29_c64_c16_dg2", "m65_c72_k3_v1", "5x7_c3_c5_padded"])
def test_public_functions(dev, name, restore_dtype):
    """modulated_deform_conv / deform_conv on logical-NCHW tensors (channels_last input included) give what the wrappers give"""
    case, ref64, ref32, _ = HD.case_and_refs(name)
    case = dict(case)
    case["x"] = case["x"].contiguous(memory_format=torch.channels_last)
    out, t = _public(case, dev, "fp32")
    assert out.dtype == torch.float32 and out.shape == ref64["out"].shape
    out.backward(case["dy"].to(dev))
    got = {"out": out.detach(), "d_x": t["x"].grad, "d_offset": t["offset"].grad,
           "d_mask": t["mask"].grad if "mask" in t else None, "dW": t["weight"].grad,
           "d_bias": t["bias"].grad if "bias" in t else None}
    got = {k: (v.double().cpu() if v is not None else None) for k, v in got.items()}
    check(name + "/public", "fp32", got, ref64, ref32)


def test_frozen_weight_skips_the_weight_gradient(dev, restore_dtype, monkeypatch):
    from fsnet_amd.hip import ops
    case, ref64, ref32, _ = HD.case_and_refs("m63_c24_k3_p1")
    calls = []
    real = ops.dcn_backward_weight
    monkeypatch.setattr(ops, "dcn_backward_weight", lambda *a, **k: calls.append(1) or real(*a, **k))
    out, t = _public(case, dev, "fp32", frozen=("weight", "bias"))
    out.backward(case["dy"].to(dev))
    assert calls == [] and t["weight"].grad is None and t["bias"].grad is None
    assert t["x"].grad is not None and t["offset"].grad is not None and t["mask"].grad is not None
    # ... and a weight that does ask for its gradient, with a gradient already there: accumulated, by one launch
    out, t = _public(case, dev, "fp32", frozen=("x", "offset", "mask"))
    t["weight"].grad = torch.ones_like(t["weight"])
    out.backward(case["dy"].to(dev))
    assert calls == [1] and t["x"].grad is None
    d_max, _ = HD.deviation((t["weight"].grad - 1).cpu(), ref64["dW"])
    added = 2.0 ** -23 * (1.0 + float(ref64["dW"].abs().max()))          # the fp32 rounding of 1 + dW itself
    assert d_max <= FACTOR["fp32"]["dW"] * HD.deviation(ref32["dW"], ref64["dW"])[0] + added


def test_graph_capture_and_replay(dev, restore_dtype):
    """forward and backward captured on one stream, replayed with changed inputs, against the eager result"""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.ops.dcn.deform_conv import modulated_deform_conv
    RT.set_compute_dtype("fp32")
    a = HD.make_case(seed=51, N=2, Ci=24, H=7, W=9, Co=24, R=3, S=3, padding=1)
    b = HD.make_case(seed=52, N=2, Ci=24, H=7, W=9, Co=24, R=3, S=3, padding=1)
    keys = ("x", "offset", "mask", "weight", "bias")
    static = {k: a[k].to(dev).requires_grad_() for k in keys}
    dy = a["dy"].to(dev)

    def step():
        out = modulated_deform_conv(static["x"], static["offset"], static["mask"], static["weight"], static["bias"], 1, 1, 1, 1, 1)
        return (out,) + torch.autograd.grad(out, [static[k] for k in keys], dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for k in keys:
            static[k].copy_(b[k].to(dev))
        dy.copy_(b["dy"].to(dev))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.detach().clone() for t in captured]
    eager = step()
    torch.cuda.synchronize()
    ref64, ref32 = HD.run_ref(b, torch.float64), HD.run_ref(b, torch.float32)
    names = ("out", "d_x", "d_offset", "d_mask", "dW", "d_bias")
    for q, r, e in zip(names, replayed, eager):
        if q != "d_x":
            assert torch.equal(r, e), q
    got = {q: r.double().cpu() for q, r in zip(names, replayed)}
    check("graph_replay", "fp32", got, ref64, ref32)
