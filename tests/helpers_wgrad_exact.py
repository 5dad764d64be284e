"""Exact-integer cases for the convolution weight gradient (conv_wgrad.hip).

Both operands are small non-zero integers (x in {-3..3} \\ {0}, dY in {-2, -1, 1, 2}; all exact in bf16), the starting
gradient is an integer in [-5, 5].  Every product and every partial sum, in any order, is then an integer of magnitude at
most max|x| * max|dY| * M * calls + max|dW0|; below 2^24 every such integer is an fp32 value, so the MFMA's fp32
accumulation, the slab stores, any reduction tree and the final `dW +=` give the float64 result bit for bit.  The
tolerance of the GPU tests is therefore zero, and because no operand is zero a pixel, tap or channel that is dropped,
doubled or taken from the wrong place changes some element.

This module is CPU only: the case generator, the float64 reference (an unfold / einsum of the defining sum), the
launchers' published geometry (which kernel a problem runs on, its output tiles, the floats of one split-K slab), the
rule by which launch_reduce picks a slab reduction, and the argument structs.  The GPU tests read what actually ran from
fs_conv_wgrad_plan / fs_conv_wgrad2_plan."""
import collections
import ctypes as C
import functools

import torch
import torch.nn.functional as F

EXACT_LIMIT = 1 << 24
GUARD = 4096                 # floats of sentinel on each side of dW
SENTINEL = 1234567.0
X_MAX, DY_MAX, DW0_MAX = 3, 2, 5

Case = collections.namedtuple("Case", "Ci Co k stride pad N H W")

# ---------------------------------------------------------------------------------------------------------------------
# the cases of the sweep: every launch path of conv_wgrad.hip at the smallest shape that reaches it
BF16_PATH_CASES = [
    # LDS-halo: M >= 1024, Cd % 64 == 0, Cs % 32 == 0
    ("halo", Case(32, 64, 3, 1, 1, 3, 23, 37)),       # ragged tiles in both directions
    ("halo", Case(64, 64, 3, 1, 0, 2, 26, 42)),       # the decoder's pad-0 form
    ("halo", Case(64, 128, 3, 1, 1, 2, 24, 40)),      # 2 x 2 output tiles
    ("halo", Case(32, 64, 3, 1, 1, 5, 45, 53)),       # about 100 pixel tiles: 32 or more splits
    # narrow: M >= 4096, Cd 16 or 32
    ("narrow", Case(16, 16, 3, 1, 0, 2, 50, 66)),
    ("narrow", Case(32, 16, 3, 1, 1, 3, 37, 41)),
    ("narrow", Case(96, 32, 3, 1, 0, 2, 50, 50)),
    ("narrow", Case(16, 16, 3, 1, 1, 4, 130, 130)),   # natural split count of 129 or more
    # 7x7 / stride-2 stem, M >= 4096 (needs a workspace)
    ("stem", Case(3, 64, 7, 2, 3, 2, 70, 122)),       # ragged 8 x 16 tiles
    ("stem", Case(6, 64, 7, 2, 3, 3, 64, 96)),
    # LDS-DMA 1x1: M >= 2048, all four tile pairs, and the strided projection
    ("w1x1", Case(64, 64, 1, 1, 0, 3, 27, 31)),       # ragged last stage
    ("w1x1", Case(128, 64, 1, 1, 0, 3, 27, 31)),
    ("w1x1", Case(64, 128, 1, 1, 0, 3, 27, 31)),
    ("w1x1", Case(128, 128, 1, 1, 0, 3, 27, 31)),
    ("w1x1", Case(64, 64, 1, 2, 0, 3, 54, 62)),
    # generic tiles
    ("tile128", Case(512, 512, 3, 1, 1, 3, 17, 20)),  # 1020 pixels: below the halo threshold
    ("tile128", Case(512, 512, 3, 2, 1, 3, 34, 50)),
    ("tile64w", Case(64, 64, 3, 2, 1, 3, 30, 46)),
    ("tile64w", Case(3, 64, 7, 2, 3, 2, 32, 64)),     # the stem below 4096 pixels
    ("tile64", Case(24, 64, 3, 1, 1, 3, 11, 13)),     # Ci not a multiple of 16, part-filled column tile
    ("tile64", Case(64, 64, 1, 1, 0, 2, 9, 13)),
    ("tile32", Case(40, 96, 3, 1, 1, 3, 11, 13)),
    ("tile16", Case(256, 12, 1, 1, 0, 2, 6, 20)),
    ("tile16", Case(128, 72, 1, 1, 0, 3, 17, 23)),
    ("tile16", Case(16, 16, 3, 1, 0, 2, 13, 19)),
    # maps narrower than the smallest tile
    ("tile64w", Case(64, 64, 3, 1, 1, 3, 1, 2)),
    ("tile128", Case(512, 512, 3, 1, 1, 4, 2, 3)),
]
F32_PATH_CASES = [   # the generic kernel only, EG = 4
    ("tile64", Case(64, 64, 3, 1, 1, 3, 11, 13)),
    ("tile32", Case(32, 32, 3, 1, 0, 2, 14, 18)),
    ("tile16", Case(20, 12, 3, 1, 1, 3, 9, 11)),
    ("tile64", Case(64, 128, 1, 2, 0, 2, 16, 32)),
    ("tile64", Case(3, 64, 7, 2, 3, 2, 32, 64)),
]
# forced split counts: one shape per path, large enough that the path's own cap (pixels per block) does not end the
# sweep early where the path can split 32 ways at all.  (tile128: at least 96 output tiles, so the planner never wants
# more than ceil(640 / 96) = 7 splits.)
SWEEP_KS = (0, 1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, "full")
NARROW_EXTRA_KS = (47, 48, 49, 112, 113, 128, 129)
Sweep = collections.namedtuple("Sweep", "path case dtype min_natural reductions")
_R3, _RF, _R4, _RG = "reduce3x3", "flat", "reduce4", "reduce"
# min_natural: the split count the full workspace must reach on the device; reductions: the slab reductions the sweep
# must have gone through (launch_reduce's rule applied to the counts the plan reports).  Together the rows walk all four
# reductions: reduce3x3 (tap-major 3x3 slabs of 64 or more channels, up to 16 slabs), flat (256 or more columns, up to
# 8), reduce4 (below 32) and the general kernel with its 128-, 32- and 16-slab steps.
SWEEP_CASES = [
    Sweep("halo", Case(32, 64, 3, 1, 1, 5, 45, 53), torch.bfloat16, 32, (_RF, _R4, _RG)),
    Sweep("halo", Case(64, 64, 3, 1, 1, 3, 45, 53), torch.bfloat16, 17, (_R3, _R4)),
    Sweep("narrow", Case(16, 16, 3, 1, 1, 4, 130, 130), torch.bfloat16, 129, (_R4, _RG)),
    Sweep("stem", Case(6, 64, 7, 2, 3, 3, 64, 96), torch.bfloat16, 32, (_RF, _R4, _RG)),
    Sweep("w1x1", Case(64, 64, 1, 1, 0, 3, 53, 57), torch.bfloat16, 32, (_R4, _RG)),
    Sweep("tile128", Case(512, 512, 3, 2, 1, 3, 34, 50), torch.bfloat16, 3, (_R3,)),
    Sweep("tile64w", Case(64, 64, 3, 2, 1, 3, 114, 118), torch.bfloat16, 32, (_R3, _R4, _RG)),
    Sweep("tile64", Case(24, 64, 3, 1, 1, 3, 53, 61), torch.bfloat16, 32, (_R4, _RG)),
    Sweep("tile32", Case(40, 96, 3, 1, 1, 3, 53, 61), torch.bfloat16, 32, (_RF, _R4, _RG)),
    Sweep("tile16", Case(128, 72, 1, 1, 0, 3, 53, 61), torch.bfloat16, 32, (_R4, _RG)),
    Sweep("tile64", Case(64, 64, 3, 1, 1, 3, 53, 61), torch.float32, 32, (_R3, _R4, _RG)),
]
# two problems per launch: (path, first, second); unequal batches
PAIR_CASES = [
    ("halo", Case(32, 64, 3, 1, 1, 3, 23, 37), Case(32, 64, 3, 1, 1, 5, 23, 37)),
    ("w1x1", Case(64, 64, 1, 1, 0, 3, 27, 31), Case(64, 64, 1, 1, 0, 5, 27, 31)),
    ("tile64", Case(24, 64, 3, 1, 1, 3, 21, 23), Case(24, 64, 3, 1, 1, 5, 21, 23)),
    ("stem", Case(3, 64, 7, 2, 3, 3, 70, 122), Case(6, 64, 7, 2, 3, 5, 70, 122)),
    # the first problem has too few pixels to split (cap 1) while the second splits: one writes dW directly, the
    # other goes through slabs that lie behind the first problem's (unused) one
    ("tile64w", Case(64, 64, 3, 2, 1, 1, 30, 46), Case(64, 64, 3, 2, 1, 5, 30, 46)),
    # narrow problems do not pair: two launches
    ("narrow", Case(16, 16, 3, 1, 0, 2, 50, 66), Case(16, 16, 3, 1, 0, 3, 50, 66)),
]
PAIR_ROOMS = ("full", 1, 2, 3, 5)
STRIDED_CASES = [
    ("halo", Case(32, 64, 3, 1, 1, 3, 23, 37)),
    ("narrow", Case(32, 16, 3, 1, 1, 3, 37, 41)),
    ("w1x1", Case(64, 64, 1, 1, 0, 3, 27, 31)),
    ("tile64", Case(24, 64, 3, 1, 1, 3, 11, 13)),
]
PROLOGUE_CASES = [Case(32, 64, 3, 1, 1, 4, 9, 13), Case(32, 64, 3, 1, 0, 4, 11, 15)]   # pad 1 and its pad-0 form


def all_table_cases():
    """(path, case, dtype) of every row above"""
    rows = [(p, c, torch.bfloat16) for p, c in BF16_PATH_CASES] + [(p, c, torch.float32) for p, c in F32_PATH_CASES]
    rows += [(s.path, s.case, s.dtype) for s in SWEEP_CASES]
    for p, c0, c1 in PAIR_CASES:
        rows += [(p, c0, torch.bfloat16), (p, c1, torch.bfloat16)]
    rows += [(p, c, torch.bfloat16) for p, c in STRIDED_CASES]
    return rows


# ---------------------------------------------------------------------------------------------------------------------
def roundup(a, b):
    return (a + b - 1) // b * b


def eg_of(dtype):
    return 8 if dtype == torch.bfloat16 else 4


Dims = collections.namedtuple("Dims", "Ci_p Co_p Ho Wo M ncols")


def dims(case, dtype):
    """padded channel counts of the activation buffers (ConvOp), the output size and the GEMM's column count"""
    Ci_p, Co_p = roundup(case.Ci, eg_of(dtype)), roundup(case.Co, 16)
    Ho = (case.H + 2 * case.pad - case.k) // case.stride + 1
    Wo = (case.W + 2 * case.pad - case.k) // case.stride + 1
    return Dims(Ci_p, Co_p, Ho, Wo, case.N * Ho * Wo, case.k * case.k * Ci_p)


def assert_exact(M, x_max, dy_max, dw0_max, calls):
    """the largest magnitude any partial sum can take stays an fp32 integer"""
    bound = x_max * dy_max * M * calls + dw0_max
    assert bound < EXACT_LIMIT, "|sum| can reach %d >= 2^24: fp32 would round (M = %d, %d calls)" % (bound, M, calls)
    return bound


def _nonzero_ints(shape, amax, gen):
    v = torch.randint(-amax, amax, shape, generator=gen)      # -amax .. amax - 1
    return torch.where(v >= 0, v + 1, v).float()               # -amax .. -1, 1 .. amax


def wgrad_f64(x_nchw, dy_nchw, k, stride, pad):
    """dW[co][ci][r][s] = sum over n, y, x of dY[n][co][y][x] * X[n][ci][y*stride - pad + r][x*stride - pad + s] with
    zeros outside X, in float64: the defining sum as an unfold and one contraction"""
    x_nchw, dy_nchw = x_nchw.double(), dy_nchw.double()
    Co, Ci = dy_nchw.shape[1], x_nchw.shape[1]
    cols = F.unfold(x_nchw, k, padding=pad, stride=stride)                   # [N][Ci*k*k][Ho*Wo]
    return torch.einsum("nol,nkl->ok", dy_nchw.flatten(2), cols).reshape(Co, Ci, k, k)


def apply_prologue(x_nhwc, scale, shift, relu):
    """x' = relu?(scale[g][c] * x + shift[g][c]), g = image // (N / G); the padding of the convolution stays zero (the
    caller pads x' with zeros, never x)"""
    N, G = x_nhwc.shape[0], scale.shape[0]
    assert N % G == 0
    g = torch.arange(N) // (N // G)
    y = x_nhwc.double() * scale.double()[g][:, None, None, :] + shift.double()[g][:, None, None, :]
    return y.clamp_min(0) if relu else y


class IntCase:
    """x [N][H][W][Ci_p] and dy [N][Ho][Wo][Co_p] as fp32 tensors of non-zero integers (padded channels included), dw0
    [Co][Ci][k][k] integers in [-5, 5], dw the float64 gradient; pro = (scale [G][Ci_p], shift [G][Ci_p], relu) or None"""

    def __init__(self, case, dtype, seed, pro=None):
        self.case, self.dtype, self.d = case, dtype, dims(case, dtype)
        d = self.d
        gen = torch.Generator().manual_seed(seed)
        x_max = X_MAX
        self.pro = None
        if pro is not None:
            G, relu = pro
            scale = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (G, d.Ci_p), generator=gen)]
            shift = torch.tensor([-1.0, 0.0, 1.0])[torch.randint(0, 3, (G, d.Ci_p), generator=gen)]
            shift[:, 0] = 1.0                                   # never all zero: padding that received the shift shows
            self.pro = (scale, shift, bool(relu))
            x_max = 2 * X_MAX + 1
        self.bound = assert_exact(d.M, x_max, DY_MAX, DW0_MAX, 2)    # (every GPU test launches twice)
        self.x = _nonzero_ints((case.N, case.H, case.W, d.Ci_p), X_MAX, gen)
        self.dy = _nonzero_ints((case.N, d.Ho, d.Wo, d.Co_p), DY_MAX, gen)
        self.dw0 = torch.randint(-DW0_MAX, DW0_MAX + 1, (case.Co, case.Ci, case.k, case.k), generator=gen).float()
        xe = self.x if self.pro is None else apply_prologue(self.x, *self.pro)
        self.dw = wgrad_f64(xe[..., :case.Ci].permute(0, 3, 1, 2), self.dy[..., :case.Co].permute(0, 3, 1, 2),
                            case.k, case.stride, case.pad)
        assert float(self.dw.abs().max()) * 2 + DW0_MAX <= self.bound

    def expected(self, calls):
        """dW0 + calls * dW as fp32 (exact: asserted)"""
        e = self.dw0.double() + calls * self.dw
        assert torch.equal(e.float().double(), e) and float(e.abs().max()) < EXACT_LIMIT
        return e.float()


@functools.lru_cache(maxsize=None)
def integer_case(case, dtype, seed=0, pro=None):
    """computed once per (case, dtype, seed, prologue) and shared; callers leave it unchanged"""
    return IntCase(case, dtype, seed, pro)


def filler(shape, seed):
    """non-zero integers for the bytes around a strided view: never data"""
    return _nonzero_ints(shape, X_MAX, torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' published geometry
PathModel = collections.namedtuple("PathModel", "path kind threads tiles ws_rows ws_cols slab chunk")


def path_model(case, dtype, workspace=True, pro=False):
    """wgrad_path() and the launchers' tiles: which kernel takes the problem, the plan's `kind` and `threads`, the
    blocks of the unsplit launch (= output tiles; the stem kernel has no unsplit form: 0), the slab [ws_rows][ws_cols]
    one split writes, and the pixels per chunk of the kernels that split by chunks (0: by pixel tiles)"""
    d = dims(case, dtype)
    bf16 = dtype == torch.bfloat16
    Cd, Cs, M, k = d.Co_p, d.Ci_p, d.M, case.k
    if bf16:
        halo3x3 = k == 3 and case.stride == 1
        if k == 7 and case.stride == 2 and case.pad == 3 and Cs == 8 and Cd == 64 and case.Co == 64 and workspace and M >= 4096:
            return PathModel("stem", 3, 256, 0, 64, 392, 64 * 392, 0)
        if halo3x3 and Cd % 64 == 0 and Cs % 32 == 0 and (M >= 1024 or pro):
            return PathModel("halo", 1, 512, (Cd // 64) * (Cs // 32), Cd, 9 * Cs, Cd * 9 * Cs, 0)
        assert not pro, "only the halo kernel stages x through the prologue"
        if k == 1 and case.pad == 0 and Cd % 64 == 0 and Cs % 64 == 0 and M >= 2048:
            cot, cit = (128 if Cd % 128 == 0 else 64), (128 if Cs % 128 == 0 else 64)
            rt, ct = Cd // cot, Cs // cit
            return PathModel("w1x1", 0, 256, rt * ct, rt * cot, ct * cit, rt * cot * ct * cit, 32)
        if halo3x3 and ((Cd == 16 and Cs % 16 == 0) or (Cd == 32 and Cs % 32 == 0)) and M >= 4096:
            cit = 32 if Cs % 32 == 0 else 16
            return PathModel("narrow", 2, 256, Cs // cit, Cd, 9 * Cs, Cd * 9 * Cs, 0)
    ncols = d.ncols
    if bf16 and Cd % 128 == 0 and ncols >= 1024 and (Cd // 128) * ((ncols + 127) // 128) >= 96:
        name, cot, clt = "tile128", 128, 128
    elif bf16 and Cd % 64 == 0 and ncols >= 256:
        name, cot, clt = "tile64w", 64, 128
    elif Cd % 64 == 0:
        name, cot, clt = "tile64", 64, 64
    elif Cd % 32 == 0:
        name, cot, clt = "tile32", 32, 128
    else:
        assert Cd % 16 == 0
        name, cot, clt = "tile16", 16, (256 if bf16 else 128)
    rt, ct = (Cd + cot - 1) // cot, (ncols + clt - 1) // clt
    chunk = 64 if (bf16 and cot + clt <= 192) else 32
    return PathModel(name, 0, 256, rt * ct, rt * cot, ct * clt, rt * cot * ct * clt, chunk)


def chunked_splits(M, chunk, s):
    """wg_split_chunks: `s` wanted splits of a pixel range of whole chunks -> the splits that are not empty"""
    chunks = (M + chunk - 1) // chunk
    cps = (chunks + s - 1) // s
    return (chunks + cps - 1) // cps


def stem_blocks(case, room):
    """launch_wgrad_stem: persistent blocks (one slab each) for a workspace with room for `room` slabs, while `room` is
    below the blocks the device holds at once: the 8 x 16-pixel tiles dealt in equal runs, no run empty"""
    d = dims(case, torch.bfloat16)
    ntiles = case.N * ((d.Wo + 15) // 16) * ((d.Ho + 7) // 8)
    per = (ntiles + room - 1) // room
    return (ntiles + per - 1) // per


def reduce_kernel(ns, ncols, k, always=False):
    """launch_reduce's rule: which slab reduction adds `ns` slabs of `ncols` columns into dW"""
    if ns <= 1 and not always:
        return "none"
    tapmajor3x3 = k == 3 and ncols % 9 == 0 and (ncols // 9) % 32 == 0
    if tapmajor3x3 and ns <= 16 and ncols >= 9 * 64:
        return "reduce3x3"
    if ns <= 8 and ncols >= 256:
        return "flat"
    if ns < 32:
        return "reduce4"
    return "reduce"


# ---------------------------------------------------------------------------------------------------------------------
# argument structs (pointers of tensors on any device; nothing is launched here)
def span_bytes(t):
    n, h, w, c = t.shape
    return ((n - 1) * t.stride(0) + (h - 1) * t.stride(1) + (w - 1) * t.stride(2) + c) * t.element_size()


def make_ktab(case, dtype):
    from fsnet_amd.hip.conv import make_ktab as mk
    d = dims(case, dtype)
    eg = eg_of(dtype)
    return torch.from_numpy(mk(case.k, case.k, d.Ci_p, eg, d.ncols // eg))


class Spec:
    """one weight-gradient problem: its case, the launchers' geometry for it and the argument struct"""

    def __init__(self, case, dtype, a, model):
        self.case, self.dtype, self.a, self.model = case, dtype, a, model


def make_spec(case, dtype, x, dy, dw, ktab, ws, pro=None):
    """x: the NHWC view the kernel reads (any n/h/w strides), dy dense, dw fp32 OIHW, ws the fp32 workspace;
    pro = (scale, shift, relu, G) device tensors of the operand prologue"""
    from fsnet_amd.hip.binding import FsWgradArgs
    d = dims(case, dtype)
    assert x.stride(3) == 1 and dy.is_contiguous() and tuple(x.shape) == (case.N, case.H, case.W, d.Ci_p)
    assert tuple(dy.shape) == (case.N, d.Ho, d.Wo, d.Co_p) and dw.dtype == torch.float32
    a = FsWgradArgs()
    a.dy, a.x, a.dw, a.ktab = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ktab.data_ptr()
    a.sN, a.sH, a.sW = x.stride(0), x.stride(1), x.stride(2)
    a.Hs, a.Ws, a.Hd, a.Wd = case.H, case.W, d.Ho, d.Wo
    a.M, a.Cd = d.M, d.Co_p
    a.Co, a.Ci, a.R, a.S = case.Co, case.Ci, case.k, case.k
    a.stride, a.pad, a.ncolgroups = case.stride, case.pad, d.ncols // eg_of(dtype)
    a.workspace, a.workspace_elems = ws.data_ptr(), ws.numel()
    a.x_bytes, a.use_halo = span_bytes(x), 1
    if pro is not None:
        scale, shift, relu, G = pro
        a.pro_a, a.pro_b, a.pro_relu = scale.data_ptr(), shift.data_ptr(), int(relu)
        a.pro_group_imgs = case.N // G if G > 1 else 0
    return Spec(case, dtype, a, path_model(case, dtype, True, pro is not None))


def copy_args(a):
    return type(a).from_buffer_copy(a)


def forced_split_args(spec, k):
    """a copy of the spec's arguments whose workspace has room for exactly `k` slabs of the spec's kernel (same
    pointer); k = 0: no workspace at all; k = "full": the spec's own workspace"""
    a = copy_args(spec.a)
    if k == "full":
        return a
    if k == 0:
        a.workspace, a.workspace_elems = None, 0
        return a
    assert k * spec.model.slab <= spec.a.workspace_elems, "the workspace is smaller than %d slabs" % k
    a.workspace_elems = k * spec.model.slab
    return a


def guarded(dw0, device):
    """dW in the middle of a longer buffer with GUARD sentinel floats on each side -> (buffer, the dW view)"""
    n = dw0.numel()
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float32, device=device)
    view = buf[GUARD:GUARD + n].view(dw0.shape)
    view.copy_(dw0)
    return buf, view


def guards_intact(buf):
    n = buf.numel() - 2 * GUARD
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
