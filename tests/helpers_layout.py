"""Plain-torch restatements of the training step's helper kernels (layout.hip, pool_upsample.hip): the packed MFMA
operand layouts, MaxPool2d(3, 2, 1) with its gradient, the upsample + concat + replicate pad, and the host-side grid
arithmetic of the one-launch copy / zero / column-sum kernels.  No kernel code is involved: the CPU tests
(test_layout_restatement_cpu.py) hold these against torch's own convolution, pooling and autograd, the GPU tests
(test_step_helpers_gpu.py) hold the kernels against these."""
import torch
import torch.nn.functional as F

# K position -> tap of a 3x3 kernel in the dgrad operand of a stride-2 convolution: the taps of each output-parity class
# (y % 2, x % 2) are contiguous, classes (0,0) (0,1) (1,0) (1,1)
S2_TAP_ORDER = (4, 3, 5, 1, 7, 0, 2, 6, 8)
# class (py, px) -> its K positions with the dY offset each reads: dx[2y'+py, 2x'+px] += W[pos]^T dy[y'+dr, x'+ds]
S2_CLASSES = {(0, 0): ((0, 0, 0),),
              (0, 1): ((1, 0, 1), (2, 0, 0)),
              (1, 0): ((3, 1, 0), (4, 0, 0)),
              (1, 1): ((5, 1, 1), (6, 1, 0), (7, 0, 1), (8, 0, 0))}


# ---- the cases of the GPU tests (the CPU tests show from the grid arithmetic below which branches they reach) ----
MiB = 1 << 20
COPY_SIZES = [1, 15, 16, 17, 4101, 49159, 8 * MiB + 16003, 24 * MiB + 9]
CSUM_CASES = [  # M, C, bytes per element
    (297, 16, 4), (1100, 16, 4), (1100, 24, 2), (1100, 12, 2), (70001, 16, 2), (5000, 512, 4), (5000, 1024, 2),
    (4100, 520, 2), (8300, 512, 4), (1, 12, 4), (3, 256, 2)]
PACK_LAYERS = [  # Ci, Co, k, stride, pad
    (64, 64, 3, 1, 1), (40, 48, 3, 1, 1), (33, 32, 3, 1, 1), (16, 16, 3, 1, 1), (96, 32, 3, 1, 1), (64, 128, 3, 2, 1),
    (256, 64, 1, 1, 0), (192, 12, 1, 1, 0), (64, 128, 1, 2, 0), (3, 64, 7, 2, 3), (6, 64, 7, 2, 3)]


def tap_of(pos, order, RS):
    return S2_TAP_ORDER[pos] if (order == 1 and RS == 9) else pos


def packed_forward(w, Co_p, Ci_p, kf_p):
    """w OIHW -> [Co_p, kf_p] with w_f[co, tap * Ci_p + ci] = w[co, ci, r, s], tap = r * S + s; zeros elsewhere"""
    Co, Ci, R, S = w.shape
    out = torch.zeros(Co_p, kf_p, dtype=w.dtype)
    for tap in range(R * S):
        out[:Co, tap * Ci_p: tap * Ci_p + Ci] = w[:, :, tap // S, tap % S]
    return out


def packed_dgrad(w, rows_d, Co_p, kd_p, order):
    """w OIHW -> [rows_d, kd_p] with w_d[ci, pos * Co_p + co] = w[co, ci, tap(pos)]; zeros elsewhere"""
    Co, Ci, R, S = w.shape
    out = torch.zeros(rows_d, kd_p, dtype=w.dtype)
    for pos in range(R * S):
        tap = tap_of(pos, order, R * S)
        out[:Ci, pos * Co_p: pos * Co_p + Co] = w[:, :, tap // S, tap % S].t()
    return out


def im2col_forward(x, R, S, stride, pad, Ci_p, kf_p):
    """x NCHW -> [N, kf_p, Ho * Wo], K ordered (tap, ci) with ci padded to Ci_p and K padded to kf_p"""
    N, Ci, H, W = x.shape
    cols = F.unfold(x, (R, S), padding=pad, stride=stride)                  # [N, Ci * R * S, L], ci major
    L = cols.shape[-1]
    cols = cols.view(N, Ci, R * S, L).permute(0, 2, 1, 3)                   # [N, tap, ci, L]
    out = torch.zeros(N, kf_p, L, dtype=x.dtype)
    out[:, : R * S * Ci_p].view(N, R * S, Ci_p, L)[:, :, :Ci] = cols
    return out


def _shifted_dy(dy, H, W, r, s, stride, pad):
    """[N, Co, H, W]: dy at ((y + pad - r) / stride, (x + pad - s) / stride) where that is a pixel of dy, else zero — the
    dgrad kernels' tap-to-offset convention (make_unit_table with sgn = -1: the tap (r, s) reads at -(r, s))"""
    N, Co, Ho, Wo = dy.shape
    out = torch.zeros(N, Co, H, W, dtype=dy.dtype)
    for y in range(H):
        u = y + pad - r
        if u % stride or not 0 <= u // stride < Ho:
            continue
        for x in range(W):
            v = x + pad - s
            if v % stride or not 0 <= v // stride < Wo:
                continue
            out[:, :, y, x] = dy[:, :, u // stride, v // stride]
    return out


def im2col_dgrad(dy, H, W, R, S, stride, pad, Co_p, kd_p, order):
    """dy NCHW -> [N, kd_p, H * W], K ordered (pos, co) with co padded to Co_p"""
    N, Co = dy.shape[:2]
    out = torch.zeros(N, kd_p, H * W, dtype=dy.dtype)
    for pos in range(R * S):
        tap = tap_of(pos, order, R * S)
        out[:, pos * Co_p: pos * Co_p + Co] = _shifted_dy(dy, H, W, tap // S, tap % S, stride, pad).reshape(N, Co, H * W)
    return out


def dgrad_by_classes(w_d, dy, H, W, Ci, Co_p):
    """3x3 / stride 2 / pad 1 input gradient from the class-ordered operand, one parity class at a time: each class is a
    K slice of w_d and a stride-1 problem over dY with the offsets of S2_CLASSES (H, W even)"""
    N, Co, Ho, Wo = dy.shape
    dyp = F.pad(dy, (0, 1, 0, 1))                                           # dr, ds in {0, 1}: one zero row / column
    dx = torch.zeros(N, Ci, H, W, dtype=dy.dtype)
    for (py, px), taps in S2_CLASSES.items():
        for pos, dr, ds in taps:
            wt = w_d[:Ci, pos * Co_p: pos * Co_p + Co]                      # [ci, co]
            src = dyp[:, :, dr: dr + H // 2, ds: ds + W // 2]
            dx[:, :, py::2, px::2] += torch.einsum("ic,nchw->nihw", wt, src)
    return dx


# ---- MaxPool2d(3, 2, 1) ----
def maxpool_ref(x):
    """x NCHW -> (y, first): y the pooled tensor, first a bool [N, C, 9, Ho * Wo] one-hot of the first maximum of each
    window in row-major window order (padding is -inf and never wins)"""
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, C, 9, Ho * Wo)
    mx = win.max(dim=2, keepdim=True).values
    eq = win == mx
    first = eq & (eq.cumsum(2) == 1)
    return mx.view(N, C, Ho, Wo), first


def maxpool_grad_ref(first, dy, H, W, addend=None):
    """scatter of dy to the argmax positions (+ addend)"""
    N, C, Ho, Wo = dy.shape
    cols = first.to(dy.dtype) * dy.reshape(N, C, 1, Ho * Wo)
    # (an even H leaves the last padded row outside every window: fold over the rows the windows span)
    dx = F.fold(cols.view(N, C * 9, Ho * Wo), (2 * Ho + 1, 2 * Wo + 1), 3, stride=2)[:, :, 1: 1 + H, 1: 1 + W]
    return dx + addend if addend is not None else dx


# ---- nearest x2 upsample + concat + replicate pad ----
def upcat_pad_ref(a, b):
    up = F.interpolate(a, scale_factor=2, mode="nearest")
    return F.pad(torch.cat([up, b], 1) if b is not None else up, (1, 1, 1, 1), mode="replicate")


# ---- host-side grid arithmetic, restated ----
def copy_grid(nbytes):
    """fs_copy_multi / fs_zero_multi for one buffer -> dict: blocks, whether the 512-block cap holds, the numbers of
    4x-unrolled rounds and of single-lane iterations the threads run (sets over all threads), the byte tail"""
    n16, tail = nbytes // 16, nbytes % 16
    want = (n16 + 1023) // 1024
    blocks = max(1, min(want, 512))
    step = blocks * 256
    rounds, rest = set(), set()
    for i0 in {0, step - 1, max(0, n16 % step - 1), n16 % step}:
        if i0 >= step:
            continue
        i, k = i0, 0
        while i + 3 * step < n16:
            i, k = i + 4 * step, k + 1
        rounds.add(k)
        rest.add(len(range(i, n16, step)))
    return dict(blocks=blocks, capped=want > 512, rounds=rounds, rest=rest, tail=tail, n16=n16)


def csum_grid(M, C, elem_bytes, wide=None):
    """fs_channel_sum (wide None) / one member of fs_channel_sum_multi (wide: the batch's lane width decision) -> dict:
    VL channels per lane, CG lanes, CGB lanes per block, PL rows per block and round, gx, gy, and over all threads the
    sets of 4x-unrolled rounds and of tail rows"""
    VW = 16 // elem_bytes
    if wide is None:
        wide = C % VW == 0 and VW != 4
    VL = VW if wide else 4
    CG = C // VL
    CGB = 1
    while CGB < CG and CGB < 64:
        CGB *= 2
    PL = 256 // CGB
    gx = max(1, min((M + 4 * PL - 1) // (4 * PL), 256))
    gy = (CG + CGB - 1) // CGB
    stride = gx * PL
    rounds, tails = set(), set()
    for m0 in range(stride):
        m, k = m0, 0
        while m + 3 * stride < M:
            m, k = m + 4 * stride, k + 1
        rounds.add(k)
        tails.add(len(range(m, M, stride)))
    return dict(VL=VL, CG=CG, CGB=CGB, PL=PL, gx=gx, gy=gy, rounds=rounds, tails=tails, last_slab=CG - (gy - 1) * CGB)


def pack_tiles(Co, Ci, RS):
    """fs_pack_weights_multi's tiling of one layer -> set of branch names its blocks take"""
    ib = 288 // RS
    IB = 1
    while IB * 2 <= ib and IB < 128:
        IB *= 2
    out = set()
    for co0 in range(0, Co, 32):
        for ci0 in range(0, Ci, IB):
            nco, nci = min(32, Co - co0), min(IB, Ci - ci0)
            if RS == 9 and nci == 32 and nco == 32:
                out.add("3x3 full float4" if (Ci * RS) % 4 == 0 and (ci0 * RS) % 4 == 0 else "3x3 full scalar")
            elif RS == 9:
                out.add("3x3 ragged")
            elif RS == 1 and nci == IB and nco == 32 and IB == 128:
                out.add("1x1 full")
            elif RS == 1:
                out.add("1x1 ragged")
            else:
                out.add("generic")
    return out
