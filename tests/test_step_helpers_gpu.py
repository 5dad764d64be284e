"""The training step's one-launch helper kernels, element for element: the weight re-pack of every convolution
(fs_pack_weights_multi), the batched copy / zero (fs_copy_multi, fs_zero_multi), the image layout change
(fs_nchw_to_nhwc), the bias-gradient column sums (fs_channel_sum, fs_channel_sum_multi), MaxPool2d(3, 2, 1) and the
upsample + concat + replicate pad with their gradients — each against the plain-torch restatement of
tests/helpers_layout.py (held against torch itself in test_layout_restatement_cpu.py, which also shows which branch
every case below reaches).

Every assertion is exact.  Copies, packs and layout changes are exact by nature (bf16: torch's round-to-nearest-even
`.bfloat16()`); the summing kernels get small integers, so that every partial sum is an integer below 2^24 (fp32) and every
stored bf16 value one below 2^8: any summation order gives the bits of the float64 reference.  Each test asserts that
bound on its own reference first."""
import pytest
import torch

from tests import helpers_layout as L

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def nchw64(x):
    return x.permute(0, 3, 1, 2).double().cpu()


def ints(g, shape, lo, hi):
    """integers in [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def spy(monkeypatch, name):
    """count the calls of one entry point of the kernel library"""
    from fsnet_amd.hip import binding
    handle = binding.load_library()
    orig = getattr(handle, name)
    calls = []

    def counted(*a):
        calls.append(name)
        return orig(*a)
    monkeypatch.setattr(handle, name, counted)
    return calls


# ---------------------------------------------------------------- A. fs_pack_weights_multi through ConvLayer.ready()
PACK_NO_DGRAD = (64, 40, 3, 1, 1)      # full and ragged 3x3 tiles with a NULL dgrad operand


def _s2_order(k, stride, pad):
    return 1 if (k == 3 and stride == 2 and pad == 1) else 0


@pytest.mark.parametrize("arena", [False, True], ids=["module", "arena"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_repack_equals_the_operand_layout(dev, monkeypatch, dtype, arena):
    """every layer's forward and dgrad operand after the step's one-launch re-pack == the restated layout, padding
    included, == what ConvOp.pack (the packer of the conv unit tests) writes.  arena: the master weights are views into
    one flat buffer at 16-byte (and no better) alignment, what the parameter arena guarantees."""
    from fsnet_amd.engine.nets import ConvLayer
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip.conv import ConvOp
    g = torch.Generator().manual_seed(17)
    specs = [(c, True) for c in L.PACK_LAYERS] + [(PACK_NO_DGRAD, False)]
    convs = [torch.nn.Conv2d(Ci, Co, k, stride=s, padding=p, bias=False).to(dev) for (Ci, Co, k, s, p), _ in specs]
    if arena:
        flat = torch.zeros(sum(c.weight.numel() + 16 for c in convs), device=dev)
        assert flat.data_ptr() % 32 == 0
        o = 4
        for c in convs:
            n = c.weight.numel()
            c.weight.data = flat[o: o + n].view_as(c.weight)
            assert c.weight.data_ptr() % 32 == 16
            o = (o + n + 7) // 8 * 8 + 4
    for c in convs:
        c.weight.data.copy_(torch.randn(c.weight.shape, generator=g))
    layers = [ConvLayer(c, need_dgrad=nd) for c, (_, nd) in zip(convs, specs)]
    ops_ = [cl.ready(dtype, dev) for cl in layers]
    for op in ops_:                                  # (zeroed, not filled: the padding is zero from allocation and stays)
        op.w_f.zero_()
        if op.need_dgrad:
            op.w_d.zero_()
    calls = spy(monkeypatch, "fs_pack_weights_multi")
    RT.bump_weights()
    assert layers[0].ready(dtype, dev) is ops_[0]
    assert len(calls) == 1 and all(cl._packed == cl._version() for cl in layers)        # one launch took them all
    for cl, op in zip(layers, ops_):
        assert cl.ready(dtype, dev) is op
    assert len(calls) == 1
    torch.cuda.synchronize()
    for ((Ci, Co, k, s, p), nd), conv, op in zip(specs, convs, ops_):
        w = conv.weight.detach().cpu()
        order = _s2_order(k, s, p) if nd else 0
        assert bool(op.s2_classes) == bool(order), (Ci, Co, k, s)
        assert torch.equal(op.w_f.cpu(), L.packed_forward(w, op.Co_p, op.Ci_p, op.kf_p).to(dtype)), (Ci, Co, k, s, "w_f")
        op2 = ConvOp(Ci, Co, k, k, s, p, dtype, dev, need_dgrad=nd)
        op2.pack(conv.weight.data)
        assert torch.equal(op2.w_f, op.w_f), (Ci, Co, k, s, "w_f against ConvOp.pack")
        if nd:
            want = L.packed_dgrad(w, op.rows_d, op.Co_p, op.kd_p, order).to(dtype)
            assert torch.equal(op.w_d.cpu(), want), (Ci, Co, k, s, "w_d")
            assert torch.equal(op2.w_d, op.w_d), (Ci, Co, k, s, "w_d against ConvOp.pack")
        else:
            assert not hasattr(op, "w_d")


# ---------------------------------------------------------------- B. fs_copy_multi / fs_zero_multi
SENTINEL = 0xA5
COPY16 = [1, 15, 16, 17] + L.COPY_SIZES[4:] + [4101, 1, 49159, 15, 16, 17, 4101, 1]     # the large ones in the middle
COPY17 = [17, 1, 4101, 16, 15, 49159] * 2 + [1, 4101, 17, 16, 15]


def _slots(sizes, dev, shift=()):
    """one sentinel-filled byte buffer with a 16-byte aligned slot per size (shift: those slots start one byte later), at
    least 64 sentinel bytes before, between and after"""
    offs, cur = [], 0
    for i, n in enumerate(sizes):
        cur = (cur + 64 + 15) // 16 * 16 + (1 if i in shift else 0)
        offs.append(cur)
        cur += n
    buf = torch.full((cur + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, [buf[o: o + n] for o, n in zip(offs, sizes)], offs


def _sources(sizes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(dev) for n in sizes]


@pytest.mark.parametrize("sizes,launches", [(COPY16, 1), (COPY17, 2)], ids=["16", "17"])
def test_copy_multi_and_zero_multi_write_the_payload_and_nothing_else(dev, monkeypatch, sizes, launches):
    from fsnet_amd.hip import ops
    assert len(sizes) == 16 * (launches - 1) + (16 if launches == 1 else 1)
    buf, dsts, offs = _slots(sizes, dev)
    srcs = _sources(sizes, dev, 23)
    want = torch.full_like(buf, SENTINEL)
    for o, s in zip(offs, srcs):
        want[o: o + s.numel()] = s
    calls = spy(monkeypatch, "fs_copy_multi")
    ops.copy_multi(list(zip(dsts, srcs)))
    torch.cuda.synchronize()
    assert len(calls) == launches
    for o, s, d in zip(offs, srcs, dsts):
        assert torch.equal(d, s), ("payload", s.numel())
    assert torch.equal(buf, want)                                # every sentinel byte around and between the slots
    calls = spy(monkeypatch, "fs_zero_multi")
    ops.zero_multi(dsts)
    torch.cuda.synchronize()
    assert len(calls) == launches
    for o, n in zip(offs, sizes):
        want[o: o + n] = 0
        assert int(buf[o: o + n].max()) == 0, ("zeroed", n)
    assert torch.equal(buf, want)


def test_copy_multi_and_zero_multi_fall_back_for_what_the_kernel_cannot_take(dev, monkeypatch):
    """a misaligned destination, a misaligned source and a non-contiguous source go through Tensor.copy_ / zero_; the
    aligned pairs of the same call still go through the kernel, in one launch"""
    from fsnet_amd.hip import ops
    sizes = [4101, 33, 17, 1000, 49159, 64]
    buf, dsts, offs = _slots(sizes, dev, shift=(1,))
    assert dsts[1].data_ptr() % 16 == 1
    srcs = _sources(sizes, dev, 29)
    g = torch.Generator().manual_seed(31)
    srcs[2] = torch.randint(0, 256, (32 + 17,), dtype=torch.uint8, generator=g).to(dev)[3: 3 + 17]      # misaligned source
    srcs[3] = torch.randint(0, 256, (2000,), dtype=torch.uint8, generator=g).to(dev)[::2]              # strided source
    assert srcs[2].data_ptr() % 16 == 3 and not srcs[3].is_contiguous()
    want = torch.full_like(buf, SENTINEL)
    for o, s in zip(offs, srcs):
        want[o: o + s.numel()] = s
    calls = spy(monkeypatch, "fs_copy_multi")
    ops.copy_multi(list(zip(dsts, srcs)))
    torch.cuda.synchronize()
    assert len(calls) == 1 and torch.equal(buf, want)
    calls = spy(monkeypatch, "fs_zero_multi")
    ops.zero_multi(dsts)
    torch.cuda.synchronize()
    for o, n in zip(offs, sizes):
        want[o: o + n] = 0
    assert len(calls) == 1 and torch.equal(buf, want)


# ---------------------------------------------------------------- C. fs_nchw_to_nhwc
@pytest.mark.parametrize("case,dtype", [((2, 3, 0, 5, 7, 8), torch.float32), ((2, 3, 0, 5, 7, 8), torch.bfloat16),
                                        ((3, 3, 3, 9, 11, 8), torch.float32), ((3, 3, 3, 9, 11, 8), torch.bfloat16),
                                        ((2, 3, 3, 4, 6, 16), torch.float32), ((2, 3, 3, 4, 6, 16), torch.bfloat16),
                                        ((2, 3, 0, 5, 7, 4), torch.float32)])
def test_nchw_to_nhwc_concatenates_rounds_and_zero_fills(dev, case, dtype):
    from fsnet_amd.hip import ops
    N, Ca, Cb, H, W, Cp = case
    g = torch.Generator().manual_seed(37 + Cb + Cp)
    a = torch.randn(N, Ca, H, W, generator=g)
    b = torch.randn(N, Cb, H, W, generator=g) if Cb else None
    want = torch.zeros(N, H, W, Cp)
    want[..., :Ca] = a.permute(0, 2, 3, 1)
    if Cb:
        want[..., Ca: Ca + Cb] = b.permute(0, 2, 3, 1)
    out = torch.full((N, H, W, Cp), -7.0, dtype=dtype, device=dev)            # the padded channels must be written
    got = ops.nchw_to_nhwc(a.to(dev), b.to(dev) if Cb else None, Cp, dtype, out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(out.cpu(), want.to(dtype))


# ---------------------------------------------------------------- D. fs_channel_sum / fs_channel_sum_multi
CSUM_CREAL = {(1100, 16, 4): 12, (1100, 24, 2): 20, (4100, 520, 2): 515, (1, 12, 4): 9, (5000, 512, 4): 500}
_CSUM = {}


def _csum_case(dev, M, C, eb):
    """(x on the device, its float64 column sums): computed once and shared, never modified"""
    key = (M, C, eb)
    if key not in _CSUM:
        g = torch.Generator().manual_seed(41 + M + C)
        xi = torch.randint(-3, 4, (M, C), generator=g, dtype=torch.int8)
        ref = xi.double().sum(0)
        assert float(ref.abs().max()) + 8 < 2 ** 24 and 3 * M + 8 < 2 ** 24     # every partial sum too (|x| <= 3, M rows)
        _CSUM[key] = (xi.to(torch.float32 if eb == 4 else torch.bfloat16).to(dev), ref)
    return _CSUM[key]


def _csum_want(ref, pre, creal):
    want = pre.double().clone()
    want[:creal] += ref[:creal]
    return want.float()


def _preload(C, seed):
    return torch.randint(-5, 6, (C,), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("case", L.CSUM_CASES, ids=lambda c: "%dx%d-%s" % (c[0], c[1], "f32" if c[2] == 4 else "bf16"))
def test_channel_sum_adds_the_exact_column_sums_to_out(dev, case):
    from fsnet_amd.hip import ops
    M, C, eb = case
    x, ref = _csum_case(dev, M, C, eb)
    creal = CSUM_CREAL.get(case, C)
    pre = _preload(C, 43 + C)
    out = pre.to(dev)
    ops.channel_sum(x, out, creal)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _csum_want(ref, pre, creal))      # channels from creal on keep their preload


def _csum_batch(dev, shapes, eb):
    items, wants, singles = [], [], []
    for i, (M, C) in enumerate(shapes):
        x, ref = _csum_case(dev, M, C, eb)
        creal = C - (i % 3) if i % 2 else C
        pre = _preload(C, 47 + i)
        items.append((x, pre.to(dev), creal))
        singles.append((x, pre.to(dev), creal))
        wants.append(_csum_want(ref, pre, creal))
    return items, singles, wants


SHAPES = [(m, c) for m, c, _ in L.CSUM_CASES]
SMALL = [(297, 16), (1100, 16), (1, 12), (3, 256), (1100, 24), (1100, 12)]
CSUM_BATCHES = {  # name -> (bytes per element, shapes, launches)
    "f32-16": (4, (SHAPES + SHAPES)[:16], 1),
    "bf16-16-narrow": (2, (SHAPES + SHAPES)[:16], 1),                        # (1100, 12) and (1, 12): C % 8 != 0
    "bf16-16-wide": (2, ([s for s in SHAPES if s[1] % 8 == 0] * 2)[:16], 1),
    "f32-17": (4, (SMALL * 3)[:17], 2),
    "bf16-17": (2, (SMALL * 3)[:17], 2),
}


@pytest.mark.parametrize("name", list(CSUM_BATCHES))
def test_channel_sum_multi_gives_every_member_its_own_sums(dev, monkeypatch, name):
    from fsnet_amd.hip import ops
    eb, shapes, launches = CSUM_BATCHES[name]
    assert len(shapes) in (16, 17)
    if name == "bf16-16-narrow":
        assert any(c % 8 for _, c in shapes)
    if name == "bf16-16-wide":
        assert all(c % 8 == 0 for _, c in shapes)
    items, singles, wants = _csum_batch(dev, shapes, eb)
    calls = spy(monkeypatch, "fs_channel_sum_multi")
    ops.channel_sum_multi(items)
    for it in singles:
        ops.channel_sum(*it)
    torch.cuda.synchronize()
    assert len(calls) == launches
    for (x, out, creal), (_, out1, _), want in zip(items, singles, wants):
        assert torch.equal(out.cpu(), want), (name, tuple(x.shape), creal)
        assert torch.equal(out, out1)


# ---------------------------------------------------------------- E. MaxPool2d(3, 2, 1)
POOL_SHAPES = [(2, 16, 12, 20), (2, 8, 13, 21), (1, 8, 1, 1), (1, 16, 2, 3), (2, 24, 7, 1), (3, 8, 1, 9)]


@pytest.mark.parametrize("lo,hi", [(-8, -1), (-3, 3)], ids=["negative", "mixed"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_and_gradient_are_exact(dev, shape, dtype, lo, hi):
    """all-negative input: every maximum is below zero, many are tied, and a border padded with anything but -inf would
    win; the gradient goes to the first maximum in window order"""
    from fsnet_amd.hip import ops
    N, C, H, W = shape
    g = torch.Generator().manual_seed(53 + H * W + hi)
    x = ints(g, shape, lo, hi)
    y_ref, first = L.maxpool_ref(x)
    dy = ints(g, tuple(y_ref.shape), -3, 3)
    add = ints(g, shape, -3, 3)
    dx_ref, dx_add_ref = L.maxpool_grad_ref(first, dy, H, W), L.maxpool_grad_ref(first, dy, H, W, add)
    for r in (x, y_ref, dx_ref, dx_add_ref):
        assert float(r.abs().max()) < 256                       # exact in bf16, sums in any order
    y, idx = ops.maxpool_fwd(nhwc(x, dtype).to(dev))
    dyd = nhwc(dy, dtype).to(dev)
    dx = ops.maxpool_bwd(dyd, idx, H, W)
    dx_add = ops.maxpool_bwd(dyd, idx, H, W, addend=nhwc(add, dtype).to(dev))
    torch.cuda.synchronize()
    assert y.dtype == dtype and torch.equal(nchw64(y), y_ref)
    assert torch.equal(nchw64(dx), dx_ref)
    assert torch.equal(nchw64(dx_add), dx_add_ref)


# ---------------------------------------------------------------- F. upsample + concat + replicate pad
UPCAT_SHAPES = [(2, 5, 7, 8, 12), (2, 1, 1, 8, 8), (1, 1, 3, 16, 0), (2, 3, 1, 32, 64), (3, 6, 5, 16, 24)]
_UPCAT = {}


def _upcat_case(shape):
    """integer inputs and the float64 autograd reference of one shape: computed once, shared by the dtypes"""
    if shape not in _UPCAT:
        N, h, w, Ca, Cb = shape
        g = torch.Generator().manual_seed(59 + h * w + Ca)
        a = ints(g, (N, Ca, h, w), -3, 3).requires_grad_(True)
        b = ints(g, (N, Cb, 2 * h, 2 * w), -3, 3).requires_grad_(True) if Cb else None
        out = L.upcat_pad_ref(a, b)
        gp = ints(g, tuple(out.shape), -3, 3)
        out.backward(gp)
        y = ints(g, (N, Ca, h, w), -2, 2).clamp_min(0)                        # the activation behind the ReLU mask
        xraw = torch.randn(N, Ca, h, w, generator=g)
        mean, invstd = torch.randn(Ca, generator=g) * 0.2, torch.rand(Ca, generator=g) + 0.5
        for r in (out.detach(), a.grad) + ((b.grad,) if Cb else ()):
            assert float(r.abs().max()) < 256
        _UPCAT[shape] = dict(a=a.detach(), b=b.detach() if Cb else None, out=out.detach(), gp=gp, da=a.grad,
                             db=b.grad if Cb else None, y=y, xraw=xraw, mean=mean, invstd=invstd)
    return _UPCAT[shape]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", UPCAT_SHAPES)
def test_upcat_pad_forward_backward_and_bn_backward_equal_autograd(dev, shape, dtype):
    """bf16: (8, 12) and (16, 24) run the 4-channel lanes, the others the 8-channel lanes; h or w = 1 makes a pixel the
    first and the last row / column of the fold"""
    from fsnet_amd.hip import ops
    N, h, w, Ca, Cb = shape
    c = _upcat_case(shape)
    ad = nhwc(c["a"], dtype).to(dev)
    bd = nhwc(c["b"], dtype).to(dev) if Cb else None
    gpd = nhwc(c["gp"], dtype).to(dev)
    out = ops.upcat_pad_fwd(ad, bd)
    da, db = ops.upcat_pad_bwd(gpd, h, w, Ca, Cb)
    yd, xd = nhwc(c["y"], dtype).to(dev), nhwc(c["xraw"], dtype).to(dev)
    st = ops.BnState(Ca, dev, 1)
    st.mean.copy_(c["mean"])
    st.invstd.copy_(c["invstd"])
    st.count = float(N * h * w)
    sums = torch.zeros(ops.STAT_SLOTS, 2, Ca, dtype=torch.float64, device=dev)
    da_bn, db_bn = ops.upcat_pad_bwd(gpd, h, w, Ca, Cb, bn=(yd, xd, st, sums))
    torch.cuda.synchronize()
    assert torch.equal(nchw64(out), c["out"])
    assert torch.equal(nchw64(da), c["da"])
    masked = c["da"] * (c["y"] > 0)
    assert torch.equal(nchw64(da_bn), masked)
    if Cb:
        assert torch.equal(nchw64(db), c["db"]) and torch.equal(nchw64(db_bn), c["db"])
    else:
        assert db is None and db_bn is None
    # the sums: xhat is not an integer, so they keep the bound of test_upcat_pad_bwd_with_batchnorm_sums
    xhat = (nchw64(xd) - c["mean"].double().view(1, -1, 1, 1)) * c["invstd"].double().view(1, -1, 1, 1)
    want = torch.stack([masked.sum((0, 2, 3)), (masked * xhat).sum((0, 2, 3))])
    got = sums.sum(0).cpu()
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
