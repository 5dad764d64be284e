"""conv_wgrad.hip against float64 with ZERO tolerance: operands are small non-zero integers (tests/helpers_wgrad_exact.py),
so every path, split count, slab reduction and the two-problem form must give the reference bit for bit.  Every launch
is made twice (the second accumulates: dW0 + 2 dW), dW sits between two sentinel runs that must stay intact, and
fs_conv_wgrad_plan / fs_conv_wgrad2_plan are the witness of which kernel and how many splits actually ran.

Run with -s for the table of split counts reached per path and the slab reduction launch_reduce picks for each."""
import ctypes as C

import pytest
import torch

from tests import helpers_wgrad_exact as WX

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    from fsnet_amd.hip.binding import lib
    return lib


def _code(dtype):
    from fsnet_amd.hip.binding import FS_DTYPE_BF16, FS_DTYPE_F32
    return FS_DTYPE_BF16 if dtype == BF16 else FS_DTYPE_F32


def _workspace(dev):
    from fsnet_amd.hip.conv import wgrad_workspace
    return wgrad_workspace(dev)


class Problem:
    """an integer case on the device: x in one of its forms, dY, the guarded dW and the argument struct"""

    def __init__(self, ic, dev, x_form="dense"):
        self.ic, case, dt, d = ic, ic.case, ic.dtype, ic.d
        if x_form == "dense":
            self.x_base = ic.x.to(dev).to(dt)
            x = self.x_base
        elif x_form == "slice":          # a channel slice of a buffer twice as wide
            wide = WX.filler((case.N, case.H, case.W, 2 * d.Ci_p), 91)
            wide[..., :d.Ci_p] = ic.x
            self.x_base = wide.to(dev).to(dt)
            x = self.x_base[..., :d.Ci_p]
        else:                            # the interior of a spatially padded buffer
            assert x_form == "interior"
            big = WX.filler((case.N, case.H + 2, case.W + 2, d.Ci_p), 92)
            big[:, 1:-1, 1:-1] = ic.x
            self.x_base = big.to(dev).to(dt)
            x = self.x_base[:, 1:-1, 1:-1]
        assert torch.equal(x.float().cpu(), ic.x)
        self.x, self.dy = x, ic.dy.to(dev).to(dt)
        self.buf, self.dw = WX.guarded(ic.dw0.to(dev), dev)
        self.ktab = WX.make_ktab(case, dt).to(dev)
        self.pro = None
        if ic.pro is not None:
            scale, shift, relu = ic.pro
            self.pro = (scale.to(dev).contiguous(), shift.to(dev).contiguous(), relu, scale.shape[0])
        self.spec = WX.make_spec(case, dt, x, self.dy, self.dw, self.ktab, _workspace(dev), self.pro)
        self.exp = [None, ic.expected(1).to(dev), ic.expected(2).to(dev)]

    def reset(self):
        self.dw.copy_(self.ic.dw0)

    def check(self, calls, what):
        torch.cuda.synchronize()
        bad = self.dw != self.exp[calls]
        if bool(bad.any()):
            i = bad.nonzero()[0].tolist()
            raise AssertionError("%s, call %d: %d of %d elements differ, first at %s: got %r, expected %r" % (
                what, calls, int(bad.sum()), bad.numel(), i, float(self.dw[tuple(i)]), float(self.exp[calls][tuple(i)])))
        assert torch.equal(self.dw, self.exp[calls])
        assert WX.guards_intact(self.buf), "%s, call %d: a sentinel next to dW was overwritten" % (what, calls)


def plan_of(a, dtype, a1=None):
    p = (C.c_int32 * 4)()
    if a1 is None:
        assert _lib().fs_conv_wgrad_plan(C.byref(a), _code(dtype), p) == 0
    else:
        assert _lib().fs_conv_wgrad2_plan(C.byref(a), C.byref(a1), _code(dtype), p) == 0
    return list(p)       # kind, blocks, threads, resident


def launch(a, dtype, a1=None):
    from fsnet_amd.hip.binding import stream_ptr
    if a1 is None:
        st = _lib().fs_conv_wgrad(C.byref(a), _code(dtype), stream_ptr())
    else:
        st = _lib().fs_conv_wgrad2(C.byref(a), C.byref(a1), _code(dtype), stream_ptr())
    assert st == 0, "launch refused with status %d" % st


def splits_of(prob, a):
    """the split count the library plans for these arguments, witnessed by the plan entry: blocks over the blocks of the
    unsplit launch (the stem kernel: its persistent blocks, each leaves a slab); the plan's kernel and block size are
    the model's"""
    m = prob.spec.model
    kind, blocks, threads, resident = plan_of(a, prob.ic.dtype)
    if m.path == "stem" and not a.workspace:        # without a workspace the stem is the generic kernel's: unsplit
        m = WX.path_model(prob.ic.case, prob.ic.dtype, workspace=False)
        assert (kind, blocks, threads) == (m.kind, m.tiles, m.threads)
        return 1
    assert (kind, threads) == (m.kind, m.threads), (m, kind, threads)
    assert resident >= 128
    if m.path == "stem":
        return blocks
    assert blocks % m.tiles == 0, (m, blocks)
    if not a.workspace:
        assert blocks == m.tiles, (m, blocks)        # unsplit: one block per output tile
    return blocks // m.tiles


def run_twice(prob, a, what):
    prob.reset()
    for calls in (1, 2):
        launch(a, prob.ic.dtype)
        prob.check(calls, what)


def reduce_name(prob, ns):
    m = prob.spec.model
    return WX.reduce_kernel(ns, prob.ic.d.ncols, prob.ic.case.k, always=m.path == "stem")


# ---------------------------------------------------------------------------------------------------------------------
PATH_ROWS = [(p, c, BF16) for p, c in WX.BF16_PATH_CASES] + [(p, c, F32) for p, c in WX.F32_PATH_CASES]


@pytest.mark.parametrize("path,case,dtype", PATH_ROWS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
def test_every_path(dev, path, case, dtype):
    """1. every launch path at the smallest shape that reaches it: the natural launch (full workspace) and the
    unsplit one (no workspace)"""
    prob = Problem(WX.integer_case(case, dtype, 1), dev)
    assert prob.spec.model.path == path
    full, none = WX.forced_split_args(prob.spec, "full"), WX.forced_split_args(prob.spec, 0)
    ns = splits_of(prob, full)
    assert splits_of(prob, none) == 1
    print("\n  %-8s %-40s natural splits %3d -> %s" % (path, tuple(case), ns, reduce_name(prob, ns)))
    if case == WX.Case(16, 16, 3, 1, 1, 4, 130, 130):
        assert ns >= 129, ns
    if case == WX.Case(32, 64, 3, 1, 1, 5, 45, 53):
        assert ns >= 32, ns
    run_twice(prob, full, "%s full workspace (%d splits)" % (path, ns))
    run_twice(prob, none, "%s no workspace" % path)


@pytest.mark.parametrize("sw", WX.SWEEP_CASES, ids=lambda s: "%s-%s-%s" % (s.path, "-".join(map(str, s.case)), str(s.dtype).replace("torch.", "")))
def test_forced_split_counts(dev, sw):
    """2. a workspace with room for exactly k slabs: every slab reduction and each of its unrolled tails"""
    path, case, dtype = sw.path, sw.case, sw.dtype
    prob = Problem(WX.integer_case(case, dtype, 2), dev)
    m = prob.spec.model
    assert m.path == path
    natural = splits_of(prob, WX.forced_split_args(prob.spec, "full"))
    assert natural >= sw.min_natural, natural
    ks = list(WX.SWEEP_KS) + (list(WX.NARROW_EXTRA_KS) if path == "narrow" else [])
    reached = {}
    for k in ks:
        if k != "full" and k > natural:
            continue                                   # (above the path's natural count the plan does not change)
        a = WX.forced_split_args(prob.spec, k)
        ns = splits_of(prob, a)
        if path == "stem" and k == 0:                  # no workspace: the generic kernel's, unsplit
            run_twice(prob, a, "stem shape without a workspace")
            continue
        room = natural if k == "full" else max(k, 1)
        assert 1 <= ns <= room, (k, ns)
        if k == "full":
            assert ns == natural
        elif path == "stem":
            assert ns == WX.stem_blocks(case, room), (k, ns)
        elif m.chunk == 0:
            assert ns == room, (k, ns)                 # pixel tiles dealt round-robin: exactly the room
        else:
            assert ns == WX.chunked_splits(prob.ic.d.M, m.chunk, room), (k, ns)
        run_twice(prob, a, "%s room for %s slabs (%d splits, %s)" % (path, k, ns, reduce_name(prob, ns)))
        reached.setdefault(ns, reduce_name(prob, ns))
    print("\n  %-8s %s %s natural %d; splits reached -> reduction: %s" % (
        path, tuple(case), str(dtype).replace("torch.", ""), natural, ", ".join("%d %s" % kv for kv in sorted(reached.items()))))
    got = set(reached)
    for lo, hi in [(1, 1), (2, 2), (3, 8), (9, 16), (17, 31), (32, 1 << 30)]:
        if natural >= lo:
            assert any(lo <= n <= hi for n in got), "no split count in %d..%d was run: %s" % (lo, hi, sorted(got))
    assert set(sw.reductions) <= set(reached.values()), reached
    if path == "narrow":
        # 113 or more: the general reduction's 128-slab step; 47-49: its 32-slab step with and without a 16-slab tail
        assert max(got) >= 129 and {47, 48, 49, 112, 113, 128, 129} <= got


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,c0,c1", WX.PAIR_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pairs(dev, path, c0, c1):
    """3. fs_conv_wgrad2: two problems in one launch and one slab arena (the first problem's workspace), at the full
    workspace and at room for fewer than 2, for 2, 3 and 5 slabs"""
    p0, p1 = Problem(WX.integer_case(c0, BF16, 3), dev), Problem(WX.integer_case(c1, BF16, 4), dev)
    m = p0.spec.model
    assert m.path == path and p1.spec.model.path == path and m.slab == p1.spec.model.slab
    # each problem alone, natural launch: the pair must give the same bits
    single = []
    for p in (p0, p1):
        run_twice(p, p.spec.a, "%s single" % path)
        single.append(p.dw.clone())
    for room in WX.PAIR_ROOMS:
        a0, a1 = WX.forced_split_args(p0.spec, room), WX.forced_split_args(p1.spec, room)
        kind, blocks, threads, _ = plan_of(a0, BF16, a1)
        assert (kind, threads) == (m.kind, m.threads)
        if path == "narrow":
            z = None                                   # two launches: the plan is the second one's
        elif path == "stem" and room == 1:
            # every persistent stem block leaves a slab, so one slab of room cannot hold a shared launch: two launches
            # of one block each, one after the other through the same slab (the plan is the second one's)
            assert blocks == 1
            z = None
        elif path == "stem":
            z = blocks
        else:
            assert blocks % m.tiles == 0
            z = blocks // m.tiles
        if z is not None:
            n_room = (1 << 30) if room == "full" else room
            assert 2 <= z <= max(2, n_room), (room, z)
            if room in (1, 2):
                assert z == 2                          # both unsplit (the stem: one persistent block each)
            if room in (3, 5) and m.chunk == 0:
                assert z == room, (room, z)            # the proportional share uses the whole room
            if room == "full" and c0.N > 1:
                assert z > 5, z
            if room == "full" and c0.N == 1:
                # the first problem cannot split (cap 1) and writes dW directly, the second goes through slabs
                chunks0 = (WX.dims(c0, BF16).M + m.chunk - 1) // m.chunk
                assert chunks0 // (256 // m.chunk) <= 1 and z >= 3, z
        print("\n  pair %-8s room %-4s -> %s blocks along the split axis" % (path, room, z))
        for p in (p0, p1):
            p.reset()
        for calls in (1, 2):
            launch(a0, BF16, a1)
            for p in (p0, p1):
                p.check(calls, "%s pair, room %s" % (path, room))
        for p, s in zip((p0, p1), single):
            assert torch.equal(p.dw, s)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["slice", "interior"])
@pytest.mark.parametrize("path,case", WX.STRIDED_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_strided_x(dev, path, case, form):
    """4. x as a channel slice of a buffer twice as wide, and as the interior of a spatially padded buffer (the
    convolution's own padding still reads as zero): the bytes around the view hold non-zero integers"""
    prob = Problem(WX.integer_case(case, BF16, 5), dev, x_form=form)
    assert prob.spec.model.path == path and not prob.x.is_contiguous()
    assert prob.spec.a.x_bytes == WX.span_bytes(prob.x) < prob.x_base.numel() * 2
    natural = splits_of(prob, prob.spec.a)
    for k in ("full", 0, 2):
        a = WX.forced_split_args(prob.spec, k)
        ns = splits_of(prob, a)
        assert ns == {"full": natural, 0: 1, 2: min(2, natural)}[k], (k, ns)
        run_twice(prob, a, "%s x as %s, room %s (%d splits)" % (path, form, k, ns))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,relu", [(1, False), (1, True), (2, False), (2, True)])
@pytest.mark.parametrize("case", WX.PROLOGUE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_prologue(dev, case, G, relu):
    """5. the operand prologue x' = relu?(scale x + shift) inside the image, zero in the padding, per statistics group;
    the planner sends it to the halo kernel whatever the pixel count"""
    prob = Problem(WX.integer_case(case, BF16, 6, (G, relu)), dev)
    assert prob.spec.model.path == "halo" and prob.ic.d.M < 1024
    for k, want in ((2, 2), (0, 1), ("full", None)):
        a = WX.forced_split_args(prob.spec, k)
        ns = splits_of(prob, a)
        assert want is None or ns == want, (k, ns)
        run_twice(prob, a, "prologue G=%d relu=%d, room %s (%d splits)" % (G, relu, k, ns))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,case,dtype", [(s.path, s.case, s.dtype) for s in WX.SWEEP_CASES if s.path in ("halo", "narrow", "stem", "w1x1", "tile64w")],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))
def test_run_to_run_identity(dev, path, case, dtype):
    """6. no atomics anywhere: two launches with identical arguments give identical bits (random-normal operands, so
    the summation order matters)"""
    d = WX.dims(case, dtype)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(case.N, case.H, case.W, d.Ci_p, generator=g).to(dev).to(dtype)
    dy = torch.randn(case.N, d.Ho, d.Wo, d.Co_p, generator=g).to(dev).to(dtype)
    ktab = WX.make_ktab(case, dtype).to(dev)
    outs = []
    for _ in range(2):
        buf, dw = WX.guarded(torch.zeros(case.Co, case.Ci, case.k, case.k), dev)
        sp = WX.make_spec(case, dtype, x, dy, dw, ktab, _workspace(dev))
        launch(sp.a, dtype)
        torch.cuda.synchronize()
        assert WX.guards_intact(buf)
        outs.append(dw.clone())
    assert torch.equal(outs[0], outs[1]) and bool(outs[0].abs().max() > 0)
