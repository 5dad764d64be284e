"""Thin host wrappers (ctypes -> libfsnet_hip.so) for the non-conv kernels.  torch tensors are used
only as device memory + stream ordering; every arithmetic step runs in the HIP library."""
import ctypes as C
import os

import torch
from torch.nn.modules.utils import _pair

from .binding import (lib, check, stream_ptr, FS_CAT_MAX, FsBnApplyArgs, FsBnBwdArgs, FsCatArgs, FsDcnArgs, FsDistillUnscaledArgs, FsFlowArgs,
                      FsDwconv7Args, FsLayerNormArgs, FsScaleResidualArgs, FsMotionMaskArgs, FsPhotoArgs, FsPhotoMeiMultiArgs, FsPhotoMultiArgs, FsPostOptArgs, FsSmoothArgs)
from .conv import dtype_code, roundup, _timed, BN_EPS, BN_MOMENTUM, Spec, run_specs

STAT_SLOTS = 8   # FS_STAT_SLOTS in include/fsnet_hip.h


def _p(t):
    return t.data_ptr() if t is not None else None


def nchw_to_nhwc(a, b, cp, dtype, out=None):
    """a (and optionally b, concatenated along C): NCHW fp32 -> NHWC [N,H,W,cp] in `dtype`."""
    a = a.contiguous()
    N, Ca, H, W = a.shape
    Cb = 0
    if b is not None:
        b = b.contiguous()
        Cb = b.shape[1]
    if out is None:
        out = torch.empty(N, H, W, cp, dtype=dtype, device=a.device)
    assert out.shape == (N, H, W, cp) and out.is_contiguous() and out.dtype == dtype
    check(lib.fs_nchw_to_nhwc(a.data_ptr(), _p(b), out.data_ptr(), N, Ca, Cb, H, W, cp, dtype_code(dtype),
                              stream_ptr()), "nchw_to_nhwc")
    return out


class BnState:
    """Device-side state of one BatchNorm invocation (saved for backward)."""
    __slots__ = ("mean", "invstd", "count", "groups", "scale", "shift")

    def __init__(self, C, device, groups=1, affine=False):
        self.mean = torch.empty(groups * C, dtype=torch.float32, device=device)
        self.invstd = torch.empty(groups * C, dtype=torch.float32, device=device)
        self.count = 0.0          # rows per statistics group (x world size)
        self.groups = groups
        # folded BatchNorm (bn_finalize): y = scale * x + shift per (group, channel), applied by the consumer
        self.scale = torch.empty(groups * C, dtype=torch.float32, device=device) if affine else None
        self.shift = torch.empty(groups * C, dtype=torch.float32, device=device) if affine else None


def bn_finalize(stats, bn, st, Cc, count, track=True, groups=1):
    """the statistics half of bn_apply (fs_bn_finalize): fills st.mean / invstd / scale / shift ([groups][C]) and
    updates the running statistics; the activation is normalised by the kernels that read it."""
    a = FsBnApplyArgs()
    a.groups = groups
    assert st.groups == groups and st.scale is not None
    a.stats = _p(stats)
    a.gamma, a.beta = bn["weight"].data_ptr(), bn["bias"].data_ptr()
    if track or stats is None:
        a.running_mean, a.running_var = bn["running_mean"].data_ptr(), bn["running_var"].data_ptr()
        a.num_batches_tracked = bn["num_batches_tracked"].data_ptr() if track else None
    a.save_mean, a.save_invstd = st.mean.data_ptr(), st.invstd.data_ptr()
    st.count = float(count)
    a.count, a.eps, a.momentum = float(count), BN_EPS, BN_MOMENTUM
    a.C = Cc
    check(lib.fs_bn_finalize(C.byref(a), st.scale.data_ptr(), st.shift.data_ptr(), stream_ptr()), "bn_finalize")
    return st


def bn_apply(x, stats, bn, st, y, H, W, count, **kw):
    """one BatchNorm (+ residual, + ReLU) forward pass, issued now (see bn_apply_spec)"""
    run_specs([bn_apply_spec(x, stats, bn, st, y, H, W, count, **kw)])
    return y


def bn_apply_spec(x, stats, bn, st, y, H, W, count, relu=True, pad_out=False, res=None, stats2=None, bn2=None, st2=None,
                  track=True, groups=1, pool=None):
    """-> Spec (conv.run_specs issues it, alone or sharing a launch with another network's BatchNorm of the same width).
    x: dense [N,H,W,C] raw conv output.  bn/bn2: dict(weight,bias,running_mean,running_var,nbt).
    groups G > 1: G stacked invocations of the module (count is per group; stats are [G][SLOTS][2][C])."""
    a = FsBnApplyArgs()
    a.groups = groups
    assert st.groups == groups and (st2 is None or st2.groups == groups)
    Cc = x.shape[-1]
    a.x, a.res, a.y = x.data_ptr(), _p(res), _p(y)
    if pool is not None:
        # pool = (pooled [N,H/2,W/2,C], argmax codes uint8): the stem's MaxPool2d(3, 2, 1) in the same pass; y may be None
        assert pool[0].is_contiguous() and pool[1].is_contiguous() and pool[0].shape == (x.shape[0], H // 2, W // 2, Cc)
        assert stats is not None and res is None and bn2 is None and not pad_out and H % 2 == 0 and W % 2 == 0
        a.pool_y, a.pool_idx = pool[0].data_ptr(), pool[1].data_ptr()
    else:
        assert y is not None
    a.stats, a.stats2 = _p(stats), _p(stats2)
    a.gamma, a.beta = bn["weight"].data_ptr(), bn["bias"].data_ptr()
    if track or stats is None:
        a.running_mean, a.running_var = bn["running_mean"].data_ptr(), bn["running_var"].data_ptr()
        a.num_batches_tracked = bn["num_batches_tracked"].data_ptr()
    a.save_mean, a.save_invstd = st.mean.data_ptr(), st.invstd.data_ptr()
    st.count = float(count)
    if bn2 is not None:
        a.gamma2, a.beta2 = bn2["weight"].data_ptr(), bn2["bias"].data_ptr()
        if track or stats2 is None:
            a.running_mean2, a.running_var2 = bn2["running_mean"].data_ptr(), bn2["running_var"].data_ptr()
            a.num_batches_tracked2 = bn2["num_batches_tracked"].data_ptr() if track else None
        a.save_mean2, a.save_invstd2 = st2.mean.data_ptr(), st2.invstd.data_ptr()
        st2.count = float(count)
    a.count, a.eps, a.momentum = float(count), BN_EPS, BN_MOMENTUM
    if pad_out:
        assert y.shape[1] == H + 2 and y.shape[2] == W + 2
    if y is not None:
        a.yN, a.yH, a.yW = y.stride(0), y.stride(1), y.stride(2)
    a.M, a.C, a.H, a.W = x.shape[0] * H * W, Cc, H, W
    a.relu, a.pad_out = int(relu), int(pad_out)
    nb = x.numel() * x.element_size() * (1 + (y is not None) + (res is not None))
    if pool is not None:
        nb += pool[0].numel() * pool[0].element_size() + pool[1].numel()
    return Spec(["bn_apply"], a, dtype_code(x.dtype), "bn_apply_pool" if pool is not None else "bn_apply", nb,
                lambda: "[%d,%d,%d,%d]%s%s%s" % (x.shape[0], H, W, Cc, " +res" if res is not None else "",
                                                 " pad" if pad_out else "", " +pool" if pool is not None else ""),
                y, "bn_apply")


def bn_backward(dout, y, x, gamma, st, dx, dgamma, dbeta, H, W, relu=True, fold=False, g_out=None, sums=None,
                allreduce=None, sums_zeroed=False, reduced=False, phase="all", glob=None, pool=None):
    """Two-pass BN backward.  dout: grad w.r.t. the block output (strided view, or the padded buffer
    when fold=True); y: saved output activation (interior view) for the ReLU mask.
    reduced=True: the first pass already happened in the epilogue of the convolution that produced dout
    (ConvOp.dgrad(bn_fuse=...)): dout is ReLU-masked and `sums` holds (sum g, sum g*xhat)."""
    bn_backward_multi([dict(dout=dout, y=y, x=x, gamma=gamma, st=st, dx=dx, dgamma=dgamma, dbeta=dbeta, H=H, W=W, relu=relu,
                            fold=fold, g_out=g_out, sums=sums, sums_zeroed=sums_zeroed, reduced=reduced, glob=glob, pool=pool)],
                      allreduce=allreduce, phase=phase)
    return None if phase == "reduce" else dx


def _bn_bwd_call(dout, y, x, gamma, st, dx, dgamma, dbeta, H, W, relu=True, fold=False, g_out=None, sums=None,
                 sums_zeroed=False, reduced=False, glob=None, pool=None):
    """argument struct of one BatchNorm backward -> dict(a=, code=, nb=, shp=, sums=, reduced=, glob=, y=, g_out=).
    pool = (pooled gradient [N,H/2,W/2,C], argmax codes, beta): the gradient w.r.t. the activation is the max-pool backward
    of the pooled gradient (+ dout, which may be None) gathered inside both passes (FsBnBwdArgs.pool_dy); with y None the
    ReLU mask is the sign of the forward's own scale * x + shift."""
    if reduced:
        assert sums is not None and not fold and g_out is None
        relu, y = False, None
    Cc = x.shape[-1]
    a = FsBnBwdArgs()
    if sums is None:
        sums = torch.zeros(st.groups * STAT_SLOTS, 2, Cc, dtype=torch.float64, device=x.device)
    elif not sums_zeroed and not reduced:
        sums.zero_()
    a.dout, a.y, a.x, a.dx, a.g_out = _p(dout), _p(y), x.data_ptr(), _p(dx), _p(g_out)
    if pool is not None:
        assert not reduced and not fold and g_out is None and pool[0].is_contiguous() and pool[1].is_contiguous()
        assert (dout is None or dout.is_contiguous()) and (y is None or y.is_contiguous())
        a.pool_dy, a.pool_idx, a.beta = pool[0].data_ptr(), pool[1].data_ptr(), pool[2].data_ptr()
    else:
        assert dout is not None
    a.sums = sums.data_ptr()
    a.gamma, a.save_mean, a.save_invstd = gamma.data_ptr(), st.mean.data_ptr(), st.invstd.data_ptr()
    a.dgamma, a.dbeta = _p(dgamma), _p(dbeta)
    a.count = st.count
    a.groups = st.groups
    if dout is not None:
        a.gN, a.gH, a.gW = dout.stride(0), dout.stride(1), dout.stride(2)
    if y is not None:
        a.yN, a.yH, a.yW = y.stride(0), y.stride(1), y.stride(2)
    a.M, a.C, a.H, a.W = x.shape[0] * H * W, Cc, H, W
    a.relu, a.fold = int(relu), int(fold)
    shape = (x.shape[0], H, W, Cc)
    return dict(a=a, code=dtype_code(x.dtype), nb=x.numel() * x.element_size(), sums=sums, reduced=reduced, glob=glob,
                has_y=y is not None, has_g=g_out is not None, has_dout=dout is not None,
                shp=lambda: "[%d,%d,%d,%d]%s%s" % (shape + (" fold" if fold else "", " pool" if pool is not None else "")))


def bn_backward_multi(calls, allreduce=None, phase="all", span=None):
    """The BatchNorm backwards of one or two networks' layers of the same width; each pass is ONE launch for all of them
    (fs_bn_bwd_reduce2 / fs_bn_bwd_apply2).  calls: keyword dicts of bn_backward (above) without allreduce / phase.
    allreduce(sums, out=): SyncBN exchange of the sums between the passes — dgamma / dbeta come from the local sums, dx
    from the global ones; span(a, b) -> one contiguous view over two sums buffers taken back to back (or None): the
    exchange of two lanes is then one collective.
    phase "reduce": only the first pass (the caller exchanges the sums of several BatchNorms in one collective and comes
    back with phase "apply", glob = the exchanged sums in each call; `sums` then holds the local ones)."""
    cs = [_bn_bwd_call(**c) for c in calls]
    if phase != "apply":
        run_specs([Spec(["bn_bwd_reduce"], c["a"], c["code"], "bn_bwd_reduce", c["nb"] * (1 + c["has_dout"] + c["has_y"]), c["shp"], None,
                        "bn_bwd_reduce") for c in cs if not c["reduced"]])
    if phase == "reduce":
        return
    pending = [c for c in cs if c["glob"] is None] if allreduce is not None else []
    if len(pending) == 2 and span is not None:
        both = span(pending[0]["sums"], pending[1]["sums"])
        if both is not None:
            out = torch.empty_like(both)
            allreduce(both, out=out)
            n0 = pending[0]["sums"].numel()
            pending[0]["glob"] = out[:n0].view(pending[0]["sums"].shape)
            pending[1]["glob"] = out[n0:].view(pending[1]["sums"].shape)
            pending = []
    for c in pending:
        # SyncBN: reduce out of place instead of cloning the local copy first (one device copy per BatchNorm and step)
        c["glob"] = torch.empty_like(c["sums"])
        allreduce(c["sums"], out=c["glob"])
    for c in cs:
        if c["glob"] is not None:
            c["a"].sums_local, c["a"].sums = c["sums"].data_ptr(), c["glob"].data_ptr()
    run_specs([Spec(["bn_bwd_apply"], c["a"], c["code"], "bn_bwd_apply", c["nb"] * (2 + c["has_dout"] + c["has_y"] + c["has_g"]), c["shp"],
                    None, "bn_bwd_apply") for c in cs])


def maxpool_fwd(x):
    return maxpool_fwd_multi([x])[0]


def maxpool_fwd_multi(xs):
    """[x NHWC] (one tensor, or two with the same H, W, C: ONE launch) -> [(y, idx)]"""
    outs = []
    for x in xs:
        N, H, W, Cc = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        outs.append((torch.empty(N, Ho, Wo, Cc, dtype=x.dtype, device=x.device),
                     torch.empty(N, Ho, Wo, Cc, dtype=torch.uint8, device=x.device)))
    if len(xs) == 2 and xs[0].shape[1:] == xs[1].shape[1:] and xs[0].dtype == xs[1].dtype:
        x, x1 = xs
        (y, idx), (y1, idx1) = outs
        N, H, W, Cc = x.shape
        _timed("maxpool_fwd", sum(t.numel() * t.element_size() * 1.25 + o[1].numel() for t, o in zip(xs, outs)),
               lambda: check(lib.fs_maxpool_fwd2(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, x1.data_ptr(), y1.data_ptr(),
                                                 idx1.data_ptr(), x1.shape[0], H, W, Cc, dtype_code(x.dtype), stream_ptr()),
                             "maxpool_fwd"), tag=str(tuple(x.shape)) + " || " + str(tuple(x1.shape)))
        return outs
    for x, (y, idx) in zip(xs, outs):
        N, H, W, Cc = x.shape
        _timed("maxpool_fwd", x.numel() * x.element_size() * 1.25 + idx.numel(),
               lambda: check(lib.fs_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, dtype_code(x.dtype),
                                                stream_ptr()), "maxpool_fwd"), tag=str(tuple(x.shape)))
    return outs


def maxpool_bwd(dy, idx, H, W, addend=None):
    return maxpool_bwd_multi([dy], [idx], H, W, [addend])[0]


def maxpool_bwd_multi(dys, idxs, H, W, addends):
    """gradients of maxpool_fwd_multi's inputs (+ addend): one launch for two tensors of the same H, W, C"""
    dxs = [torch.empty(dy.shape[0], H, W, dy.shape[3], dtype=dy.dtype, device=dy.device) for dy in dys]
    work = lambda dx, idx, ad: dx.numel() * dx.element_size() * (1.25 + (ad is not None)) + idx.numel()
    if len(dys) == 2 and dys[0].shape[1:] == dys[1].shape[1:] and dys[0].dtype == dys[1].dtype:
        dy, dy1 = dys
        Cc = dy.shape[3]
        _timed("maxpool_bwd", sum(work(dx, i, a) for dx, i, a in zip(dxs, idxs, addends)),
               lambda: check(lib.fs_maxpool_bwd2(dy.data_ptr(), idxs[0].data_ptr(), _p(addends[0]), dxs[0].data_ptr(),
                                                 dy.shape[0], dy1.data_ptr(), idxs[1].data_ptr(), _p(addends[1]),
                                                 dxs[1].data_ptr(), dy1.shape[0], H, W, Cc, dtype_code(dy.dtype),
                                                 stream_ptr()), "maxpool_bwd"),
               tag=str(tuple(dxs[0].shape)) + " || " + str(tuple(dxs[1].shape)))
        return dxs
    for dy, idx, ad, dx in zip(dys, idxs, addends, dxs):
        _timed("maxpool_bwd", work(dx, idx, ad),
               lambda: check(lib.fs_maxpool_bwd(dy.data_ptr(), idx.data_ptr(), _p(ad), dx.data_ptr(), dy.shape[0], H, W,
                                                dy.shape[3], dtype_code(dy.dtype), stream_ptr()), "maxpool_bwd"),
               tag=str(tuple(dx.shape)))
    return dxs


def upcat_pad_fwd(a, b):
    N, h, w, Ca = a.shape
    Cb = b.shape[3] if b is not None else 0
    out = torch.empty(N, 2 * h + 2, 2 * w + 2, Ca + Cb, dtype=a.dtype, device=a.device)
    _timed("upcat_pad_fwd", (a.numel() + (b.numel() if b is not None else 0) + out.numel()) * a.element_size(),
           lambda: check(lib.fs_upcat_pad_fwd(a.data_ptr(), _p(b), out.data_ptr(), N, h, w, Ca, Cb, dtype_code(a.dtype),
                                              stream_ptr()), "upcat_pad_fwd"), tag=str(tuple(out.shape)))
    return out


def upcat_pad_bwd(dpad, h, w, Ca, Cb, bn=None):
    """bn = (y, x, BnState, sums): also the first pass of the BatchNorm backward the `da` half feeds (fs_upcat_pad_bwd_bn):
    da comes back masked by y > 0 and `sums` (zeroed f64 [SLOTS][2][Ca]) holds (sum g, sum g * xhat)"""
    N = dpad.shape[0]
    da = torch.empty(N, h, w, Ca, dtype=dpad.dtype, device=dpad.device)
    db = torch.empty(N, 2 * h, 2 * w, Cb, dtype=dpad.dtype, device=dpad.device) if Cb else None
    nbytes = (da.numel() + (db.numel() if db is not None else 0) + dpad.numel()) * da.element_size()
    if bn is not None:
        y, x, st, sums = bn
        assert y.is_contiguous() and x.is_contiguous() and y.shape == da.shape == x.shape and st.groups == 1
        assert sums.dtype == torch.float64 and sums.numel() == STAT_SLOTS * 2 * Ca
        _timed("upcat_pad_bwd", nbytes + 2 * da.numel() * da.element_size(),
               lambda: check(lib.fs_upcat_pad_bwd_bn(dpad.data_ptr(), da.data_ptr(), _p(db), N, h, w, Ca, Cb, y.data_ptr(),
                                                     x.data_ptr(), st.mean.data_ptr(), st.invstd.data_ptr(), sums.data_ptr(),
                                                     dtype_code(dpad.dtype), stream_ptr()), "upcat_pad_bwd_bn"),
               tag=str(tuple(dpad.shape)) + " bn")
        return da, db
    _timed("upcat_pad_bwd", nbytes,
           lambda: check(lib.fs_upcat_pad_bwd(dpad.data_ptr(), da.data_ptr(), _p(db), N, h, w, Ca, Cb,
                                              dtype_code(dpad.dtype), stream_ptr()), "upcat_pad_bwd"),
           tag=str(tuple(dpad.shape)))
    return da, db


def channel_sum(x, out, creal):
    """out[c] += sum over rows of dense x [..., C]."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    _timed("channel_sum", x.numel() * x.element_size(),
           lambda: check(lib.fs_channel_sum(x.data_ptr(), out.data_ptr(), M, Cc, creal, dtype_code(x.dtype),
                                            stream_ptr()), "channel_sum"), tag=str(tuple(x.shape)))


def channel_sum_multi(items):
    """[(x, out, creal)]: out[c] += column sums of dense x [..., C] — one launch per 16 (same dtype)"""
    items = list(items)
    if len(items) == 1:
        return channel_sum(*items[0])
    for i in range(0, len(items), 16):
        chunk = items[i:i + 16]
        n = len(chunk)
        code = dtype_code(chunk[0][0].dtype)
        assert all(dtype_code(x.dtype) == code for x, _, _ in chunk)
        xs = (C.c_void_p * n)(*[x.data_ptr() for x, _, _ in chunk])
        outs = (C.c_void_p * n)(*[o.data_ptr() for _, o, _ in chunk])
        Ms = (C.c_int64 * n)(*[x.numel() // x.shape[-1] for x, _, _ in chunk])
        Cs = (C.c_int32 * n)(*[x.shape[-1] for x, _, _ in chunk])
        Cr = (C.c_int32 * n)(*[int(cr) for _, _, cr in chunk])
        _timed("channel_sum", sum(x.numel() * x.element_size() for x, _, _ in chunk),
               lambda: check(lib.fs_channel_sum_multi(xs, outs, Ms, Cs, Cr, n, code, stream_ptr()), "channel_sum_multi"),
               tag="%d tensors" % n)


def depth_head_fwd(logits, bins, K, min_depth, max_depth):
    N, H, W, Cl = logits.shape
    depth = torch.empty(N, 1, H, W, dtype=torch.float32, device=logits.device)
    disp = torch.empty(N, 1, H, W, dtype=torch.float32, device=logits.device)
    check(lib.fs_depth_head_fwd(logits.data_ptr(), bins.data_ptr(), depth.data_ptr(), disp.data_ptr(), N * H * W, K,
                                Cl, float(min_depth), float(max_depth), stream_ptr()), "depth_head_fwd")
    return depth, disp


def depth_head_bwd(logits, bins, d_depth, d_disp, K, min_depth, max_depth, dtype):
    N, H, W, Cl = logits.shape
    dl = torch.empty(N, H, W, Cl, dtype=dtype, device=logits.device)
    check(lib.fs_depth_head_bwd(logits.data_ptr(), bins.data_ptr(), _p(d_depth), _p(d_disp), dl.data_ptr(),
                                N * H * W, K, Cl, float(min_depth), float(max_depth), dtype_code(dtype),
                                stream_ptr()), "depth_head_bwd")
    return dl


def _head_scale(hb, logits_list, P2, base_fx):
    if P2 is None or base_fx is None:
        return
    assert P2.is_cuda and P2.dtype == torch.float32 and P2.is_contiguous() and P2.shape[1:] == (3, 4)
    assert P2.shape[0] == logits_list[0].shape[0]
    hb.P2, hb.base_fx, hb.nimg = P2.data_ptr(), float(base_fx), P2.shape[0]


def depth_head_fwd_multi(logits_list, bins, K, min_depth, max_depth, P2=None, base_fx=None):
    """[logits [N,H,W,Cl] fp32 per scale] -> [(depth, disp)] in one launch (<= 4 scales, same Cl).
    P2 + base_fx: focal-length depth scaling (depth_encoder.py:36-43)"""
    from .binding import FsHeadBatch
    hb = FsHeadBatch()
    _head_scale(hb, logits_list, P2, base_fx)
    hb.n = len(logits_list)
    Cl = logits_list[0].shape[3]
    outs = []
    for s, lg in enumerate(logits_list):
        N, H, W, c = lg.shape
        assert c == Cl and lg.dtype == torch.float32 and lg.is_contiguous()
        depth = torch.empty(N, 1, H, W, dtype=torch.float32, device=lg.device)
        disp = torch.empty(N, 1, H, W, dtype=torch.float32, device=lg.device)
        hb.logits[s], hb.depth[s], hb.disp[s], hb.M[s] = lg.data_ptr(), depth.data_ptr(), disp.data_ptr(), N * H * W
        outs.append((depth, disp))
    check(lib.fs_depth_head_fwd_multi(C.byref(hb), bins.data_ptr(), K, Cl, float(min_depth), float(max_depth),
                                      stream_ptr()), "depth_head_fwd_multi")
    return outs


def depth_head_bwd_multi(logits_list, bins, d_depths, d_disps, K, min_depth, max_depth, dtype, P2=None, base_fx=None):
    """gradients of all scales' logits in one launch; d_depths / d_disps entries may be None"""
    from .binding import FsHeadBatch
    hb = FsHeadBatch()
    _head_scale(hb, logits_list, P2, base_fx)
    hb.n = len(logits_list)
    Cl = logits_list[0].shape[3]
    outs = []
    for s, lg in enumerate(logits_list):
        N, H, W, c = lg.shape
        assert c == Cl
        dl = torch.empty(N, H, W, Cl, dtype=dtype, device=lg.device)
        hb.logits[s], hb.dlogits[s], hb.M[s] = lg.data_ptr(), dl.data_ptr(), N * H * W
        hb.d_depth[s], hb.d_disp[s] = _p(d_depths[s]), _p(d_disps[s])
        outs.append(dl)
    check(lib.fs_depth_head_bwd_multi(C.byref(hb), bins.data_ptr(), K, Cl, float(min_depth), float(max_depth),
                                      dtype_code(dtype), stream_ptr()), "depth_head_bwd_multi")
    return outs


def pose_tail_fwd(x, nframes, invert, scale=0.01):
    B, h, w, Cx = x.shape
    aa = torch.empty(B, nframes, 1, 3, dtype=torch.float32, device=x.device)
    tr = torch.empty(B, nframes, 1, 3, dtype=torch.float32, device=x.device)
    T = torch.empty(B, 4, 4, dtype=torch.float32, device=x.device)
    check(lib.fs_pose_tail_fwd(x.data_ptr(), aa.data_ptr(), tr.data_ptr(), T.data_ptr(), B, h * w, Cx, nframes,
                               int(invert), float(scale), stream_ptr()), "pose_tail_fwd")
    return aa, tr, T


def pose_tail_bwd(x, dT, nframes, invert, dtype, scale=0.01, out=None):
    B, h, w, Cx = x.shape
    dx = torch.empty(B, h, w, Cx, dtype=dtype, device=x.device) if out is None else out
    assert dx.shape == x.shape and dx.is_contiguous() and dx.dtype == dtype and x.is_contiguous()
    check(lib.fs_pose_tail_bwd(x.data_ptr(), dT.data_ptr(), dx.data_ptr(), B, h * w, Cx, nframes, int(invert),
                               float(scale), dtype_code(dtype), stream_ptr()), "pose_tail_bwd")
    return dx


class _PhotoBackend:
    """What differs between the two sets of loss kernels: the argument struct, the launches and the names the profile
    tools key on.  setup(pl, P2, Ts, seed, st) and pose_grad(pl, st) take the engine; the rest take (args, stream)."""

    def __init__(self, name, args, geo_floats, setup, identity, fwd, bwd, pose_grad, bwd_tiles):
        self.name, self.args, self.geo_floats = name, args, geo_floats
        self.setup, self.identity, self.fwd, self.bwd, self.pose_grad, self.bwd_tiles = setup, identity, fwd, bwd, pose_grad, bwd_tiles


def _photo_backend(multi, fisheye=False):
    if not multi:        # frame_ids = [0, a, b], pinhole and fisheye: fs_photo_*
        return _PhotoBackend(
            "photo_fused", FsPhotoArgs, lambda n: 48,
            lambda pl, P2, Ts, seed, st: lib.fs_photo_setup(P2.data_ptr(), Ts[0].data_ptr(), Ts[1].data_ptr(),
                                                            pl.geo.data_ptr(), pl.B, seed, int(pl.fisheye), st),
            lib.fs_photo_identity_rows, lib.fs_photo_fused_fwd, lib.fs_photo_fused_bwd,
            lambda pl, st: lib.fs_photo_pose_grad(pl.geo.data_ptr(), pl.dP.data_ptr(), pl.dT[0].data_ptr(),
                                                  pl.dT[1].data_ptr(), pl.B, pl.S, pl.bwd_tiles, st),
            lib.fs_photo_fused_bwd_tiles)

    def setup(pl, P2, Ts, seed, st):
        for f in range(4):
            pl._Tp[f] = Ts[f].data_ptr() if f < pl.nsrc else None
        return lib.fs_photo_multi_setup(P2.data_ptr(), pl._Tp, pl.nsrc, pl.geo.data_ptr(), pl.B, seed, st)

    def pose_grad(pl, st):
        return lib.fs_photo_multi_pose_grad(pl.geo.data_ptr(), pl.dP.data_ptr(), pl._dT.data_ptr(), pl.nsrc, pl.B, pl.S,
                                            pl.bwd_tiles, st)

    if fisheye:
        def setup_mei(pl, P2, Ts, seed, st):
            for f in range(4):
                pl._Tp[f] = Ts[f].data_ptr() if f < pl.nsrc else None
            return lib.fs_photo_mei_multi_setup(pl._Tp, pl.nsrc, pl.geo.data_ptr(), pl.B, seed, st)

        return _PhotoBackend(  # one to four sources on the Mei ray tables: fs_photo_mei_multi_* (identity planes, tiles and
            #                    pose gradient have no geometry of their own: the pinhole chain's)
            "photo_mei_multi", FsPhotoMeiMultiArgs, lambda n: 18 + 12 * n, setup_mei,
            lib.fs_photo_multi_identity, lib.fs_photo_mei_multi_fwd, lib.fs_photo_mei_multi_bwd, pose_grad,
            lib.fs_photo_multi_bwd_tiles)
    return _PhotoBackend(      # one to four sources, pinhole: fs_photo_multi_*
        "photo_multi", FsPhotoMultiArgs, lambda n: 18 + 12 * n, setup,
        lib.fs_photo_multi_identity, lib.fs_photo_multi_fwd, lib.fs_photo_multi_bwd, pose_grad,
        lib.fs_photo_multi_bwd_tiles)


class PhotometricLoss:
    """Fused loss chain for one batch geometry (B, H, W, scales) over nsrc = 1..4 source frames.  forward() returns the
    loss vector (f64 [2S+1]: loss/s, smooth_loss/s, total); backward() returns d depth_s and dT_f (nsrc [B,4,4] views).
    nsrc == 2 runs the two-source kernels (fs_photo_*), every other count the N-frame ones (fs_photo_multi_*; after
    stage_fisheye() their ray-table form fs_photo_mei_multi_*); force_multi=True puts nsrc == 2 on those as well (their
    tests).
    want_pred: also materialise the warped images / overlap masks (self.pred, self.ov) — only needed for logging and
    for the ("original_image", f, s) entries the reference leaves in its output dict."""

    def __init__(self, B, H, W, scales, device, min_depth, max_depth, want_pred=True, overlapped_mask=True, nsrc=2,
                 force_multi=False):
        if not 1 <= int(nsrc) <= 4:
            raise ValueError("PhotometricLoss takes 1 to 4 source frames, got %r" % (nsrc,))
        N = self.nsrc = int(nsrc)
        self.multi = bool(force_multi) or N != 2
        be = self._be = _photo_backend(self.multi)
        self.B, self.H, self.W = B, H, W
        # overlapped_mask=False (multi_dataset / nusc configs): reprojection terms are used wherever they are, with
        # border-clamped samples (monodepth2_decoder.py:110-116, 230-235)
        self.overlapped_mask = bool(overlapped_mask)
        self.scales = list(scales)
        S = self.S = len(self.scales)
        self.device = device
        f32, f64, u8 = torch.float32, torch.float64, torch.uint8
        self.geo = torch.zeros(B, be.geo_floats(N), dtype=f32, device=device)
        self.want_pred = bool(want_pred)
        self.pred = self.ov = None
        if self.want_pred:
            self.pred = torch.empty(S, N, B, 3, H, W, dtype=f32, device=device)
            self.ov = torch.empty(S, N, B, H, W, dtype=u8, device=device)
        self.ident = torch.empty(B, N, H, W, dtype=f32, device=device)
        self.sel = torch.empty(S, B, H, W, dtype=u8, device=device)
        # accumulators zeroed every step in one memset: loss_sums[S*B] mask_sum[B] disp_sum[S*B] sm_sums[2*S*B] dot[S*B]
        self.n_acc = S * B + B + S * B + 2 * S * B + S * B
        self.acc = torch.zeros(self.n_acc, dtype=f64, device=device)
        o = 0
        self.loss_sums = self.acc[o:o + S * B]; o += S * B
        self.mask_sum = self.acc[o:o + B]; o += B
        self.disp_sum = self.acc[o:o + S * B]; o += S * B
        self.sm_sums = self.acc[o:o + 2 * S * B]; o += 2 * S * B
        self.dot = self.acc[o:o + S * B]
        self.out = torch.zeros(2 * S + 1, dtype=f64, device=device)
        self.hw = [(H >> s, W >> s) for s in self.scales]
        self.color = [None] * S
        self.bwd_tiles = int(be.bwd_tiles(H, W))
        self.dP = torch.zeros(self.S * B * self.bwd_tiles, N, 12, dtype=f32, device=device)   # per-tile partials
        # one flat buffer behind the per-scale depth gradients: a single memset per backward instead of one per scale
        sizes = [B * h * w for (h, w) in self.hw]
        self._dd_flat = torch.zeros(sum(sizes), dtype=f32, device=device)
        self.d_depth, o = [], 0
        for n_el, (h, w) in zip(sizes, self.hw):
            self.d_depth.append(self._dd_flat[o:o + n_el].view(B, 1, h, w))
            o += n_el
        self.d_disp = [torch.empty(B, 1, h, w, dtype=f32, device=device) for (h, w) in self.hw]
        self._dT = torch.zeros(N, B, 4, 4, dtype=f32, device=device)
        self.dT = [self._dT[f] for f in range(N)]
        self.pyr = [None if s == 0 else torch.empty(B, 3, H >> s, W >> s, dtype=f32, device=device)
                    for s in self.scales]
        # the levels below full resolution as host arrays for fs_color_pyramid_multi (the buffers are persistent)
        lv = [i for i, s in enumerate(self.scales) if s != 0]
        self._pyr_n = len(lv)
        self._pyr_outs = (C.c_void_p * max(len(lv), 1))(*[self.pyr[i].data_ptr() for i in lv])
        self._pyr_hs = (C.c_int32 * max(len(lv), 1))(*[self.hw[i][0] for i in lv])
        self._pyr_ws = (C.c_int32 * max(len(lv), 1))(*[self.hw[i][1] for i in lv])
        self._pa = be.args()
        self._Tp = (C.c_void_p * 4)()
        self._sa = FsSmoothArgs()
        self.seed_buf = torch.zeros(1, dtype=torch.int32, device=device)   # device-resident tie-break seed
        self._prefetched = None
        # fisheye (Mei model): persistent per-sample table pointers / parameters / mask plane, refreshed per step by
        # stage_fisheye() so that a captured hipGraph keeps reading the same addresses
        self.fisheye = False
        self.motion_mask = None      # [B,H,W] fp32 or None: precomputed motion mask (monodepth2_decoder.py:243-246)
        self.lut_table = self.mei = self.warp_mask = None
        self._lut_keep = None
        self._clean_acc = self._clean_dd = False
        register_prezero(self, lambda o: o._prezero(), device)

    def stage_fisheye(self, tables, mei_rows):
        """tables: B device tensors [4,H,W] (fs_mei_lut); mei_rows: host float32 [B,8] = k1 k2 xi g1 g2 u0 v0 0.
        Copies the pointer table and the parameters into persistent device buffers on the current stream."""
        B, dev = self.B, self.device
        if self.multi and self._be.args is not FsPhotoMeiMultiArgs:
            # the N-frame engine moves to the ray-table entry points: same buffers and layouts, the argument struct grows
            # by the three ray-table fields
            self._be = _photo_backend(True, fisheye=True)
            self._pa = self._be.args()
        if self.lut_table is None:
            self.lut_table = torch.zeros(B, dtype=torch.int64, device=dev)
            self.mei = torch.zeros(B, 8, dtype=torch.float32, device=dev)
            self.warp_mask = torch.empty(B, self.H, self.W, dtype=torch.float32, device=dev)
        assert len(tables) == B and all(t.shape == (4, self.H, self.W) and t.is_contiguous() for t in tables)
        ptrs = [t.data_ptr() for t in tables]
        if self._lut_keep is not None and self._lut_keep[1] == ptrs and bool((self._lut_keep[2] == mei_rows).all()):
            self.fisheye = True
            return                                    # same calibrations as the previous step: nothing to upload
        # fresh pinned staging buffers per upload: the caching host allocator keeps them alive until the asynchronous
        # copy has run (a reused buffer could be overwritten by the next step's staging before that)
        self.lut_table.copy_(torch.tensor(ptrs, dtype=torch.int64).pin_memory(), non_blocking=True)
        self.mei.copy_(torch.from_numpy(mei_rows.copy()).pin_memory(), non_blocking=True)
        self._lut_keep = (list(tables), ptrs, mei_rows.copy())
        self.fisheye = True

    @staticmethod
    def _key(img0, srcs, patched_mask):
        return (img0.data_ptr(),) + tuple(s.data_ptr() for s in srcs) + (_p(patched_mask),)

    def _set_inputs(self, img0, srcs, patched_mask):
        assert len(srcs) == self.nsrc, "expected %d source frames, got %d" % (self.nsrc, len(srcs))
        pa = self._pa
        pa.img0 = img0.data_ptr()
        for f in range(len(pa.img_src)):
            pa.img_src[f] = srcs[f].data_ptr() if f < self.nsrc else None
        pa.patched_mask = _p(patched_mask)
        pa.ident, pa.mask_sum = self.ident.data_ptr(), self.mask_sum.data_ptr()
        pa.geo = self.geo.data_ptr()
        pa.B, pa.H, pa.W, pa.S = self.B, self.H, self.W, self.S
        if self.multi:
            pa.nsrc = self.nsrc

    def prefetch(self, img0, srcs, patched_mask):
        """The part of the chain that only needs the batch (accumulator reset, colour pyramid, identity
        reprojection + mask sum): may run on another stream beside the networks; forward() then skips it."""
        self._set_inputs(img0, srcs, patched_mask)
        self._input_only(img0, C.byref(self._pa), stream_ptr())
        self._prefetched = self._key(img0, srcs, patched_mask)

    def _prezero(self):
        """(ops.prezero_all) the accumulators and the depth-gradient maps are about to be zeroed at the step's head"""
        self._clean_acc = self._clean_dd = True
        return [self.acc, self._dd_flat]

    def _input_only(self, img0, pa, st):
        if getattr(self, "_clean_acc", False):
            _join_pack(img0.device)         # zeroed at the step's head on the pack stream: this stream waits for it
        else:
            self.acc.zero_()
        self._clean_acc = False
        if self._pyr_n:
            check(lib.fs_color_pyramid_multi(img0.data_ptr(), self._pyr_outs, self._pyr_hs, self._pyr_ws, self._pyr_n,
                                             self.B, self.H, self.W, st), "color_pyramid_multi")
        check(self._be.identity(pa, st), "photo_multi_identity" if self.multi else "photo_identity_rows")

    def _fill(self, img0, srcs, patched_mask, depths, disps, noise_seed, gout):
        pa, sa = self._pa, self._sa
        self._set_inputs(img0, srcs, patched_mask)
        pa.no_overlap_mask = 0 if self.overlapped_mask else 1
        pa.pred, pa.ov, pa.sel = _p(self.pred), _p(self.ov), self.sel.data_ptr()
        pa.loss_sums = self.loss_sums.data_ptr()
        pa.dP = self.dP.data_ptr()
        pa.gout = _p(gout)
        pa.noise_seed = -1 if noise_seed is None else int(noise_seed)
        pa.noise_seed_ptr = self.seed_buf.data_ptr() if noise_seed is None else None
        if self.fisheye:
            pa.lut_ptrs, pa.mei, pa.warp_mask = self.lut_table.data_ptr(), self.mei.data_ptr(), self.warp_mask.data_ptr()
        elif not self.multi:
            pa.lut_ptrs = pa.mei = pa.warp_mask = None
        pa.motion_mask = _p(self.motion_mask)
        sa.disp_sum, sa.sm_sums, sa.dot = self.disp_sum.data_ptr(), self.sm_sums.data_ptr(), self.dot.data_ptr()
        sa.gout = _p(gout)
        sa.B, sa.S = self.B, self.S
        for i, (h, w) in enumerate(self.hw):
            pa.depth[i] = depths[i].data_ptr()
            pa.dh[i], pa.dw[i] = h, w
            pa.d_depth[i] = self.d_depth[i].data_ptr()
            sa.disp[i] = disps[i].data_ptr()
            sa.color[i] = (img0 if self.scales[i] == 0 else self.pyr[i]).data_ptr()
            sa.d_disp[i] = self.d_disp[i].data_ptr()
            sa.h[i], sa.w[i], sa.scale_id[i] = h, w, self.scales[i]

    def _bytes(self, depth_passes):
        """algorithmic bytes of the fused forward (depth read once) / backward (depth read + gradient written) (SURVEY
        §8d): per scale, target 12 Npx + nsrc sources 12 nsrc Npx + depth 4 Npx / 4^s per pass + result 4 Npx"""
        N_px = float(self.B * self.H * self.W)
        return sum(12.0 * (self.nsrc + 1) * N_px + 4.0 * N_px + 4.0 * depth_passes * N_px / (4 ** s) for s in self.scales)

    def forward(self, img0, srcs, P2, Ts, patched_mask, depths, disps, noise_seed=-1, motion_mask=None):
        """img0, srcs[nsrc]: NCHW fp32; P2 [B,3,4] fp32; Ts[nsrc]: [B,4,4] fp32; patched_mask f64 [B,H,W] or None;
        depths/disps: per scale [B,1,h,w] fp32 contiguous; motion_mask: fp32 [B,H,W] or None."""
        st = stream_ptr()
        be = self._be
        assert len(srcs) == self.nsrc and len(Ts) == self.nsrc
        if motion_mask is not None:
            assert motion_mask.dtype == torch.float32 and motion_mask.is_contiguous() and motion_mask.shape == (self.B, self.H, self.W)
        self.motion_mask = motion_mask
        assert img0.is_contiguous() and all(s.is_contiguous() for s in srcs) and all(T.is_contiguous() for T in Ts)
        if patched_mask is not None:
            assert patched_mask.dtype == torch.float64 and patched_mask.is_contiguous()
        self._keep = (img0, srcs, patched_mask, depths, disps, noise_seed)
        self._fill(img0, srcs, patched_mask, depths, disps, noise_seed, None)
        pre, self._prefetched = self._prefetched, None
        have_inputs = pre == self._key(img0, srcs, patched_mask)
        pa, sa = C.byref(self._pa), C.byref(self._sa)
        # (noise_seed None: the setup kernel bumps the device seed — fresh noise every step, also on a graph replay)
        check(be.setup(self, P2, Ts, self.seed_buf.data_ptr() if noise_seed is None else None, st),
              "photo_multi_setup" if self.multi else "photo_setup")
        if self.fisheye:
            check(lib.fs_mei_stage_mask(self.lut_table.data_ptr(), _p(patched_mask), self.warp_mask.data_ptr(), self.B,
                                        self.H, self.W, st), "mei_stage_mask")
        if not have_inputs:
            self._input_only(img0, pa, st)
        # the edge-aware smoothness term needs only the disparities and the colour pyramid: on the (by now idle) pose
        # stream beside the photometric kernels instead of after them — this stretch of the step is serial
        fork = self._fork(img0.device)
        if fork is not None:
            fork[1].wait_stream(fork[0])
            with torch.cuda.stream(fork[1]):
                st2 = stream_ptr()
                check(lib.fs_smooth_mean(sa, st2), "smooth_mean")
                check(lib.fs_smooth_fwd(sa, st2), "smooth_fwd")
        else:
            check(lib.fs_smooth_mean(sa, st), "smooth_mean")
            check(lib.fs_smooth_fwd(sa, st), "smooth_fwd")
        _timed(be.name + "_fwd", self._bytes(1), lambda: check(be.fwd(pa, st), be.name + "_fwd"))
        if fork is not None:
            fork[0].wait_stream(fork[1])         # smoothness sums (side stream) before the finalize kernel
        # fresh result tensors per call (the previous step's stay valid for whoever kept them) — the kernel writes
        # the per-scale vector and the scalar the caller differentiates, so nothing has to be cloned on the device
        self.out = torch.empty(2 * self.S + 1, dtype=torch.float64, device=img0.device)
        self.total = torch.empty((), dtype=torch.float64, device=img0.device)
        check(lib.fs_loss_finalize(self.loss_sums.data_ptr(), self.mask_sum.data_ptr(), self.sm_sums.data_ptr(), sa,
                                   self.out.data_ptr(), self.total.data_ptr(), st), "loss_finalize")
        return self.out

    @staticmethod
    def _fork(device):
        """(current stream, pose stream) when the smoothness kernels may run beside the photometric ones"""
        from ..engine.runtime import RT
        if not (RT.overlap and device.type == "cuda"):
            return None
        cur, side = torch.cuda.current_stream(device), RT.side_stream(device)
        return None if cur.cuda_stream == side.cuda_stream else (cur, side)

    def backward(self, gout=None):
        """gout: device f64 scalar (upstream grad of total loss) or None (=1)."""
        st = stream_ptr()
        be = self._be
        img0, srcs, patched_mask, depths, disps, noise_seed = self._keep
        self._fill(img0, srcs, patched_mask, depths, disps, noise_seed, gout)
        pa, sa = C.byref(self._pa), C.byref(self._sa)
        if getattr(self, "_clean_dd", False):
            _join_pack(img0.device)
        else:
            self._dd_flat.zero_()
        self._clean_dd = False
        fork = self._fork(img0.device)
        if fork is not None:                      # smoothness backward beside the photometric backward
            fork[1].wait_stream(fork[0])
            with torch.cuda.stream(fork[1]):
                check(lib.fs_smooth_bwd(sa, stream_ptr()), "smooth_bwd")
        _timed(be.name + "_bwd", self._bytes(2), lambda: check(be.bwd(pa, st), be.name + "_bwd"))
        check(be.pose_grad(self, st), "photo_multi_pose_grad" if self.multi else "photo_pose_grad")
        if fork is not None:
            fork[0].wait_stream(fork[1])
        else:
            check(lib.fs_smooth_bwd(sa, st), "smooth_bwd")
        return self.d_depth, self.d_disp, self.dT


class _OnMultiBackend(type):
    def __instancecheck__(cls, obj):
        return isinstance(obj, PhotometricLoss) and obj.multi


class PhotometricLossMulti(PhotometricLoss, metaclass=_OnMultiBackend):
    """The earlier name of PhotometricLoss(..., nsrc=nsrc, force_multi=True), with nsrc in its old position.  No code
    of its own: the name is kept for callers written against it, and isinstance() answers whether an engine — built
    under either name — runs the N-frame kernels."""

    def __init__(self, B, H, W, scales, device, min_depth, max_depth, nsrc, want_pred=True, overlapped_mask=True):
        super().__init__(B, H, W, scales, device, min_depth, max_depth, want_pred=want_pred,
                         overlapped_mask=overlapped_mask, nsrc=nsrc, force_multi=True)


def sumsq(g, out, step_counter=None):
    """out += sum(g^2); step_counter: device int32 bumped by one in the same launch"""
    check(lib.fs_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), _p(step_counter), stream_ptr()), "sumsq")


def adam_step(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm=0.0, sumsq_buf=None, grad_scale=1.0, step_buf=None,
              lr_buf=None):
    check(lib.fs_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(b1),
                           float(b2), float(eps), float(wd), int(step), float(max_norm or 0.0), _p(sumsq_buf),
                           float(grad_scale), _p(step_buf), _p(lr_buf), stream_ptr()), "adam_step")


def _runs(runs):
    """run table (device int64 [R][2], or None: the whole span) -> (pointer, count)"""
    if runs is None:
        return None, 0
    assert runs.dtype == torch.int64 and runs.is_contiguous() and runs.dim() == 2 and runs.shape[1] == 2
    return runs.data_ptr(), runs.shape[0]


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, decoupled=True, max_norm=0.0, sumsq_buf=None, grad_scale=1.0,
               step_buf=None, lr_buf=None, runs=None):
    """decoupled: torch.optim.AdamW's decay (False: Adam's L2 form, as adam_step); runs: only these [lo, hi) ranges"""
    rp, rn = _runs(runs)
    check(lib.fs_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(b1),
                            float(b2), float(eps), float(wd), int(bool(decoupled)), int(step), float(max_norm or 0.0),
                            _p(sumsq_buf), float(grad_scale), _p(step_buf), _p(lr_buf), rp, rn, stream_ptr()),
          "adamw_step")


def sgd_step(p, g, buf, lr, momentum, dampening, nesterov, wd, step, max_norm=0.0, sumsq_buf=None, grad_scale=1.0,
             step_buf=None, lr_buf=None, runs=None):
    """torch.optim.SGD; buf: the momentum buffer (None with momentum == 0); step == 1 stores the gradient as the buffer"""
    rp, rn = _runs(runs)
    check(lib.fs_sgd_step(p.data_ptr(), g.data_ptr(), _p(buf), p.numel(), float(lr), float(momentum), float(dampening),
                          int(bool(nesterov)), float(wd), int(step), float(max_norm or 0.0), _p(sumsq_buf),
                          float(grad_scale), _p(step_buf), _p(lr_buf), rp, rn, stream_ptr()), "sgd_step")


COPY_MAX = 16


def copy_multi(pairs):
    """[(dst, src)] same-shape/dtype contiguous device tensors -> one launch per 16 copies (current stream);
    pairs the kernel cannot take (unaligned views, dtype change, host source) go through Tensor.copy_."""
    fast = []
    for dst, src in pairs:
        if (src.is_cuda and src.dtype == dst.dtype and src.shape == dst.shape and src.is_contiguous()
                and dst.is_contiguous() and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.numel() > 0):
            fast.append((dst, src))
        else:
            dst.copy_(src, non_blocking=True)
    for i in range(0, len(fast), COPY_MAX):
        chunk = fast[i:i + COPY_MAX]
        n = len(chunk)
        srcs = (C.c_void_p * n)(*[s.data_ptr() for _, s in chunk])
        dsts = (C.c_void_p * n)(*[d.data_ptr() for d, _ in chunk])
        nbytes = (C.c_int64 * n)(*[s.numel() * s.element_size() for _, s in chunk])
        check(lib.fs_copy_multi(srcs, dsts, nbytes, n, stream_ptr()), "copy_multi")


def zero_multi(tensors):
    """contiguous 16-byte aligned device tensors -> zeroed, one launch per 16 (current stream)"""
    fast = []
    for t in tensors:
        if t.numel() == 0:
            continue
        if t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0:
            fast.append(t)
        else:
            t.zero_()
    for i in range(0, len(fast), COPY_MAX):
        chunk = fast[i:i + COPY_MAX]
        n = len(chunk)
        dsts = (C.c_void_p * n)(*[t.data_ptr() for t in chunk])
        nbytes = (C.c_int64 * n)(*[t.numel() * t.element_size() for t in chunk])
        check(lib.fs_zero_multi(dsts, nbytes, n, stream_ptr()), "zero_multi")


# ---- per-step scratch zeroed together at the step's head (engine/nets.py pack_everything_async -> prezero_all) ----
_PREZERO = []          # [(weakref to the owner, fn(owner) -> [tensors to zero]; fn marks them clean)]
PREZERO_EPOCH = [0]    # bumped by every prezero_all: owners can tell "zeroed at the head of the running step" from "some time ago"


def _indexed(device):
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def register_prezero(owner, fn, device):
    """fn(owner) -> tensors on `device` to zero; it marks them clean and is only called for that device's steps"""
    import weakref
    _PREZERO.append((weakref.ref(owner), fn, _indexed(device)))


def _join_pack(device):
    from ..engine.nets import join_pack
    join_pack(device)


def prezero_all(device):
    """zero every registered scratch buffer that was used since its last zeroing, in one launch on the current stream; the
    owners' own zero_() calls are then skipped once (their `clean` flags)"""
    todo, alive = [], []
    device = _indexed(device)
    PREZERO_EPOCH[0] += 1
    for ref, fn, dev in _PREZERO:
        o = ref()
        if o is None:
            continue
        alive.append((ref, fn, dev))
        if dev != device:        # (fn has side effects — clean flags, bump pointers: another device's owners are left alone)
            continue
        todo.extend(fn(o))
    _PREZERO[:] = alive
    if todo:
        zero_multi(todo)


def counter_incr(buf):
    """device int32 counter += 1 on the current stream (replayable from a hipGraph)"""
    check(lib.fs_counter_incr(buf.data_ptr(), stream_ptr()), "counter_incr")


# ---------------------------------------------------------------------------------------------
# evaluation and the sparse-VO post-optimisation
# ---------------------------------------------------------------------------------------------
def resize_linear(src, H, W, invert=False):
    """src: device fp32 [h, w] -> [H, W] with OpenCV's INTER_LINEAR rule (invert: 1 / resize(1 / src))."""
    assert src.is_cuda and src.dtype == torch.float32 and src.dim() == 2
    src = src.contiguous()
    dst = torch.empty(H, W, dtype=torch.float32, device=src.device)
    check(lib.fs_resize_linear(src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], H, W, int(invert),
                               stream_ptr()), "resize_linear")
    return dst


def depth_eval(pred, gt):
    """pred: device fp32 [B, h, w]; gt: device fp32 [B, H, W].  Returns f64 [B, 16] on the device:
    ratio, err[7] (median-scaled), abs_err[7], n_valid  (kitti_unsupervised_eval.py:47-80)."""
    assert pred.is_cuda and gt.is_cuda and pred.dtype == gt.dtype == torch.float32
    assert pred.dim() == 3 and gt.dim() == 3 and pred.shape[0] == gt.shape[0]
    pred, gt = pred.contiguous(), gt.contiguous()
    out = torch.empty(pred.shape[0], 16, dtype=torch.float64, device=pred.device)
    scratch = torch.empty(gt.numel() * 2, dtype=torch.float32, device=pred.device)
    check(lib.fs_depth_eval(pred.data_ptr(), gt.data_ptr(), pred.shape[0], pred.shape[1], pred.shape[2], gt.shape[1],
                            gt.shape[2], scratch.data_ptr(), out.data_ptr(), stream_ptr()), "depth_eval")
    return out


def depth_eval_masked(pred, gt, mask=None, lo=0.3, hi=60.0, crop=False):
    """depth_eval with the valid set as arguments (fs_depth_eval_masked): lo < gt < hi (compared in float32, as numpy
    compares a float32 array with a Python float), the Garg crop when `crop`, and mask != 0 when a uint8 / bool mask
    [B, H, W] is given.  Defaults: the fisheye evaluation (kitti360_fisheye_eval.py:43-72).  Returns f64 [B, 16]."""
    assert pred.is_cuda and gt.is_cuda and pred.dtype == gt.dtype == torch.float32
    assert pred.dim() == 3 and gt.dim() == 3 and pred.shape[0] == gt.shape[0]
    pred, gt = pred.contiguous(), gt.contiguous()
    if mask is not None:
        assert mask.is_cuda and tuple(mask.shape) == tuple(gt.shape) and mask.dtype in (torch.uint8, torch.bool)
        mask = mask.contiguous().view(torch.uint8)
    out = torch.empty(pred.shape[0], 16, dtype=torch.float64, device=pred.device)
    scratch = torch.empty(gt.numel() * 2, dtype=torch.float32, device=pred.device)
    check(lib.fs_depth_eval_masked(pred.data_ptr(), gt.data_ptr(), _p(mask), pred.shape[0], pred.shape[1],
                                   pred.shape[2], gt.shape[1], gt.shape[2], float(lo), float(hi), int(bool(crop)),
                                   scratch.data_ptr(), out.data_ptr(), stream_ptr()), "depth_eval_masked")
    return out


def _depth_operand(t, name):
    """-> (contiguous tensor, is_u16).  float32, or 16-bit storage read as unsigned: torch.uint16, or torch.int16
    holding the same bits (numpy `a.view(np.int16)` of a uint16 plane; torch builds without uint16 kernels can still
    allocate, copy and slice int16)."""
    assert t.is_cuda and t.dim() == 3, "%s: device tensor [N, H, W]" % name
    if t.dtype == torch.float32:
        return t.contiguous(), 0
    if t.dtype in (torch.uint16, torch.int16):
        return t.contiguous(), 1
    raise TypeError("%s: float32, uint16 or int16 (read as uint16) expected, got %s" % (name, t.dtype))


def depth_errors9(pred, gt, scale=256.0):
    """The nine KITTI depth-benchmark metrics of N image pairs (fs_depth_errors9; kitti_supervised_eval.py:7-81).
    pred, gt: device tensors [N, H, W] of equal shape, each float32 (metres) or uint16 (the raw PNG plane, value / scale
    metres); int16 storage is accepted and read as uint16, bit for bit.  Returns f64 [N, 10] on the device: mae, rmse,
    inverse mae, inverse rmse, log mae, log rmse, scale invariant log, abs relative, squared relative, n_valid."""
    pred, pu = _depth_operand(pred, "pred")
    gt, gu = _depth_operand(gt, "gt")
    assert tuple(pred.shape) == tuple(gt.shape) and pred.device == gt.device
    N, H, W = pred.shape
    ws = int(lib.fs_depth_errors9_workspace_bytes(N, H, W))
    if ws < 0:
        raise ValueError("depth_errors9: bad shape N=%d H=%d W=%d" % (N, H, W))
    workspace = torch.empty(ws // 8, dtype=torch.float64, device=pred.device)
    out = torch.empty(N, 10, dtype=torch.float64, device=pred.device)
    check(lib.fs_depth_errors9(pred.data_ptr(), gt.data_ptr(), pu, gu, float(scale), N, H, W, workspace.data_ptr(), ws,
                               out.data_ptr(), stream_ptr()), "depth_errors9")
    return out


def depth_quantize_u16(depth, scale=256.0):
    """depth: device fp32 [H, W] -> torch.uint16 [H, W] = trunc(depth * scale) saturated to [0, 65535], NaN -> 0
    (fs_depth_quantize_u16: the KITTI devkit's uint16(depth * 256)).  `.cpu().numpy()` of the result is a uint16 array."""
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2
    depth = depth.contiguous()
    out = torch.empty(depth.shape, dtype=torch.int16, device=depth.device)
    check(lib.fs_depth_quantize_u16(depth.data_ptr(), out.data_ptr(), float(scale), depth.shape[0], depth.shape[1],
                                    stream_ptr()), "depth_quantize_u16")
    return out.view(torch.uint16)


class _LidarDepth:
    """What the LiDAR ground-truth ops share: the workspace, the scans of G frames as one `points` [N, 4] with
    `offsets` [G + 1] into it, and the `depth` maps.  Buffers are kept between calls of the same (G, H, W) so that a
    call can be captured into a graph and replayed: stage() copies the inputs into them, run() issues the kernels only."""

    def __init__(self, name, workspace_bytes, shape, dtype, device):
        """workspace_bytes: what the entry point's *_workspace_bytes gives for this shape; shape, dtype: of `depth`,
        (G, ..., H, W)"""
        self.G, self.H, self.W, self.device = shape[0], shape[-2], shape[-1], torch.device(device)
        ws = int(workspace_bytes)
        if ws < 0:
            raise ValueError("%s: bad shape G=%d H=%d W=%d" % (name, self.G, self.H, self.W))
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.offsets = torch.zeros(self.G + 1, dtype=torch.int64, device=self.device)
        self.depth = torch.empty(*shape, dtype=dtype, device=self.device)
        self.points = torch.empty(0, 4, dtype=torch.float32, device=self.device)

    def _stage_scans(self, scans):
        """scans: G float32 [Ni, 4] arrays / tensors"""
        import numpy as np
        assert len(scans) == self.G
        counts = [int(s.shape[0]) for s in scans]
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        pts = torch.cat([torch.as_tensor(np.asarray(s, dtype=np.float32).reshape(-1, 4)) for s in scans])
        if self.points.shape[0] != pts.shape[0]:
            self.points = torch.empty(pts.shape[0], 4, dtype=torch.float32, device=self.device)
        self.points.copy_(pts)
        self.offsets.copy_(torch.from_numpy(offs))

    def _stage_f64(self, dst, src):
        import numpy as np
        dst.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(src, dtype=np.float64).reshape(dst.shape))))

    def _points_ptr(self):
        """NULL for an empty cloud"""
        return _p(self.points) if self.points.numel() else None


class LidarMeiDepth(_LidarDepth):
    """LiDAR ground truth through the Mei fisheye model, G frames per call (fs_lidar_mei_depth;
    kitti360_fisheye_eval.py:97-145)."""

    def __init__(self, G, H, W, device):
        super().__init__("lidar_mei_depth", lib.fs_lidar_mei_depth_workspace_bytes(G, H, W), (G, H, W), torch.float32,
                         device)
        self.T = torch.zeros(G, 16, dtype=torch.float64, device=self.device)
        self.mei = torch.zeros(G, 7, dtype=torch.float64, device=self.device)
        self.close_mask = torch.empty(G, H, W, dtype=torch.uint8, device=self.device)

    def stage(self, scans, T, mei):
        """scans: G float32 [Ni, 4] arrays / tensors; T: f64 [G, 4, 4]; mei: f64 [G, 7] = gamma1 gamma2 u0 v0 k1 k2 xi"""
        self._stage_scans(scans)
        self._stage_f64(self.T, T)
        self._stage_f64(self.mei, mei)

    def run(self):
        check(lib.fs_lidar_mei_depth(self._points_ptr(), self.offsets.data_ptr(),
                                     int(self.points.shape[0]), self.T.data_ptr(), self.mei.data_ptr(), self.G, self.H,
                                     self.W, self.depth.data_ptr(), self.close_mask.data_ptr(),
                                     self.workspace.data_ptr(), self.workspace.numel(), stream_ptr()), "lidar_mei_depth")
        return self.depth, self.close_mask


def lidar_mei_depth(scans, T, mei, H, W, device):
    """one call: G = len(scans) frames -> (depth fp32 [G, H, W], close_mask uint8 [G, H, W]) on `device`"""
    op = LidarMeiDepth(len(scans), H, W, device)
    op.stage(scans, T, mei)
    return op.run()


class LidarPinholeDepth(_LidarDepth):
    """LiDAR ground truth through a pinhole camera with the KITTI export's duplicate pass, G frames per call
    (fs_lidar_pinhole_depth; monodepth_utils.py:422-458)."""

    def __init__(self, G, H, W, device):
        super().__init__("lidar_pinhole_depth", lib.fs_lidar_pinhole_depth_workspace_bytes(G, H, W), (G, H, W),
                         torch.float32, device)
        self.P = torch.zeros(G, 12, dtype=torch.float64, device=self.device)

    def stage(self, scans, P):
        """scans: G float32 [Ni, 4] arrays / tensors; P: f64 [G, 3, 4] velodyne -> image"""
        self._stage_scans(scans)
        self._stage_f64(self.P, P)

    def run(self):
        check(lib.fs_lidar_pinhole_depth(self._points_ptr(), self.offsets.data_ptr(),
                                         int(self.points.shape[0]), self.P.data_ptr(), self.G, self.H, self.W,
                                         self.depth.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
                                         stream_ptr()), "lidar_pinhole_depth")
        return self.depth


def lidar_pinhole_depth(scans, P, H, W, device):
    """one call: G = len(scans) frames -> depth fp32 [G, H, W] on `device`"""
    op = LidarPinholeDepth(len(scans), H, W, device)
    op.stage(scans, P)
    return op.run()


class LidarNuscDepth(_LidarDepth):
    """The nuScenes ground-truth export, G samples x C cameras per call (fs_lidar_nusc_depth_u16;
    nuscenes_unsupervised_eval.py:85-126 and the uint16 cast of :198).  `depth` is the PNG plane: torch.uint16
    [G, C, H, W] (int16 storage holding the same bits)."""

    def __init__(self, G, C, H, W, device):
        self.C = int(C)
        super().__init__("lidar_nusc_depth", lib.fs_lidar_nusc_depth_workspace_bytes(G, self.C, H, W),
                         (G, self.C, H, W), torch.int16, device)
        self.M = torch.zeros(G, self.C, 12, dtype=torch.float64, device=self.device)

    def stage(self, scans, M):
        """scans: G float32 [Ni, 4] arrays / tensors (ego-frame x, y, z, one unused lane); M: f64 [G, C, 3, 4], rows
        0..2 of homo_intrinsics @ inv(extrinsics)"""
        self._stage_scans(scans)
        self._stage_f64(self.M, M)

    def run(self):
        check(lib.fs_lidar_nusc_depth_u16(self._points_ptr(), self.offsets.data_ptr(), int(self.points.shape[0]),
                                          self.M.data_ptr(), self.G, self.C, self.H, self.W, self.depth.data_ptr(),
                                          self.workspace.data_ptr(), self.workspace.numel(), stream_ptr()),
              "lidar_nusc_depth_u16")
        return self.depth.view(torch.uint16)


def lidar_nusc_depth_u16(scans, M, H, W, device):
    """one call: G = len(scans) samples, C = M.shape[1] cameras -> torch.uint16 [G, C, H, W] on `device`"""
    import numpy as np
    M = np.asarray(M, dtype=np.float64)
    op = LidarNuscDepth(len(scans), M.shape[1], H, W, device)
    op.stage(scans, M)
    return op.run()


_CENTRE_TABLES = {}


def postopt_centres(h_seg, w_seg, device):
    """the SLIC start table [K, 2] fp32 on `device` (postopt_utils.py:108-112): numpy's meshgrid of
    arange(-1, 1, 2/h_seg) x arange(-1, 1, 2/w_seg), K from numpy's arange.  Cached, so a captured call copies
    nothing from the host."""
    import numpy as np
    key = (float(h_seg), float(w_seg), str(device))
    t = _CENTRE_TABLES.get(key)
    if t is None:
        c = np.stack(np.meshgrid(np.arange(-1, 1.0, 2.0 / h_seg), np.arange(-1, 1.0, 2.0 / w_seg), indexing='ij'),
                     axis=-1).reshape(-1, 2)
        t = torch.from_numpy(np.ascontiguousarray(c.astype(np.float32))).to(device)
        _CENTRE_TABLES[key] = t
    return t


def post_optimize(image, depth, vo, *, h_seg, w_seg, iter_num, lab_dist_weight, depth_dist_weight, image_dist_weight,
                  lambda0, lambda1, lambda2, max_points=800, rgb_mean, rgb_std, return_labels=False):
    """Sparse-VO depth post-optimisation of B images in one fs_postopt call (postopt_utils.py:170-226).
    image [B,3,H,W] normalised, depth [B,H,W] (> 0), vo [B,H,W] (metres): device fp32.  Returns the refined depth
    [B,H,W]; with return_labels also the int32 segment labels [B,H,W] (compacted to the non-empty segments, index
    order) and the int32 count of non-empty segments [B]."""
    assert image.is_cuda and image.dim() == 4 and image.shape[1] == 3
    B, _, H, W = image.shape
    assert depth.shape == (B, H, W) and vo.shape == (B, H, W)
    image = image.float().contiguous()
    depth = depth.float().contiguous()
    vo = vo.float().contiguous()
    ctab = postopt_centres(h_seg, w_seg, image.device)
    K = ctab.shape[0]
    nbytes = int(lib.fs_postopt_workspace_bytes(B, H, W, K))
    if nbytes < 0:
        raise ValueError("post_optimize: %d segment slots / %dx%d images are outside the kernel's limits" % (K, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
    out = torch.empty_like(depth)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=image.device) if return_labels else None
    nseg = torch.empty(B, dtype=torch.int32, device=image.device) if return_labels else None
    a = FsPostOptArgs()
    a.image, a.depth, a.vo, a.centres, a.out = image.data_ptr(), depth.data_ptr(), vo.data_ptr(), ctab.data_ptr(), \
        out.data_ptr()
    a.labels, a.nseg = _p(labels), _p(nseg)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    for i in range(3):
        a.rgb_mean[i], a.rgb_std[i] = float(rgb_mean[i]), float(rgb_std[i])
    a.lab_dist_weight, a.depth_dist_weight, a.image_dist_weight = lab_dist_weight, depth_dist_weight, image_dist_weight
    a.lambda0, a.lambda1, a.lambda2 = lambda0, lambda1, lambda2
    a.B, a.H, a.W, a.K, a.iter_num, a.max_points = B, H, W, K, int(iter_num), int(max_points)
    check(lib.fs_postopt(C.byref(a), stream_ptr()), "postopt")
    if return_labels:
        return out, labels, nseg
    return out


# ---------------------------------------------------------------------------------------------
# motion masks: dense Farneback flow and the epipolar mask (base_precompute_hooks.py:27-148), and ground-truth masks
# through the augmentation plan
# ---------------------------------------------------------------------------------------------
OPTFLOW_FARNEBACK_GAUSSIAN = 256


def _flow_args(B, H, W, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    """FsFlowArgs of the parameters, each checked here so that a bad one names itself (the C ABI says FS_EINVAL)"""
    if not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError("optical_flow_farneback: pyr_scale must lie in (0, 1), got %r" % (pyr_scale,))
    if not 0 <= int(levels) <= 15:
        raise ValueError("optical_flow_farneback: levels must lie in 0..15, got %r" % (levels,))
    if not 1 <= int(winsize) <= 129:
        raise ValueError("optical_flow_farneback: winsize must lie in 1..129, got %r" % (winsize,))
    if int(iterations) < 1:
        raise ValueError("optical_flow_farneback: iterations must be >= 1, got %r" % (iterations,))
    if int(poly_n) not in (5, 7):
        raise ValueError("optical_flow_farneback: poly_n must be 5 or 7, got %r" % (poly_n,))
    if not float(poly_sigma) >= 0.0:
        raise ValueError("optical_flow_farneback: poly_sigma must be >= 0, got %r" % (poly_sigma,))
    if int(flags) not in (0, OPTFLOW_FARNEBACK_GAUSSIAN):
        raise ValueError("optical_flow_farneback: flags must be 0 or OPTFLOW_FARNEBACK_GAUSSIAN (256), got %r"
                         % (flags,))
    a = FsFlowArgs()
    a.pyr_scale, a.poly_sigma = float(pyr_scale), float(poly_sigma)
    a.B, a.H, a.W, a.levels, a.winsize = B, H, W, int(levels), int(winsize)
    a.iterations, a.poly_n, a.flags = int(iterations), int(poly_n), int(flags)
    return a


def optical_flow_farneback(img0, img1, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2,
                           flags=0, workspace=None, out=None):
    """cv2.calcOpticalFlowFarneback(gray(img0), gray(img1), None, ...) of B frame pairs in one fs_optflow_farneback
    call.  img0 / img1: device uint8 [B,H,W,3] (gray as cv2 COLOR_BGR2GRAY, channel 0 weighted as blue).  Returns
    flow [B,H,W,2] fp32 (x, y).  workspace / out: optional preallocated uint8 / fp32 tensors (a captured graph keeps
    its own)."""
    assert img0.is_cuda and img0.dtype == torch.uint8 and img0.dim() == 4 and img0.shape[-1] == 3
    assert img1.shape == img0.shape and img1.dtype == torch.uint8
    B, H, W, _ = img0.shape
    img0, img1 = img0.contiguous(), img1.contiguous()
    a = _flow_args(B, H, W, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    nbytes = int(lib.fs_optflow_workspace_bytes(C.byref(a)))
    if nbytes < 0:
        raise ValueError("optical_flow_farneback: %dx%d frames are outside the kernel's limits" % (H, W))
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=img0.device)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes
    flow = out if out is not None else torch.empty(B, H, W, 2, dtype=torch.float32, device=img0.device)
    assert flow.shape == (B, H, W, 2) and flow.dtype == torch.float32 and flow.is_contiguous()
    a.img0, a.img1, a.flow, a.workspace, a.workspace_bytes = img0.data_ptr(), img1.data_ptr(), flow.data_ptr(), \
        ws.data_ptr(), nbytes
    check(lib.fs_optflow_farneback(C.byref(a), stream_ptr()), "optflow_farneback")
    return flow


def optflow_level_image(img0, img1, level, h, w, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5,
                        poly_sigma=1.2, flags=0):
    """pyramid level `level` (h x w) of the gray pair as optical_flow_farneback builds it -> fp32 [B,2,h,w]"""
    B, H, W, _ = img0.shape
    img0, img1 = img0.contiguous(), img1.contiguous()
    a = _flow_args(B, H, W, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    nbytes = int(lib.fs_optflow_workspace_bytes(C.byref(a)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img0.device)
    out = torch.empty(B, 2, h, w, dtype=torch.float32, device=img0.device)
    a.img0, a.img1, a.workspace, a.workspace_bytes = img0.data_ptr(), img1.data_ptr(), ws.data_ptr(), nbytes
    check(lib.fs_optflow_level_image(C.byref(a), int(level), out.data_ptr(), stream_ptr()), "optflow_level_image")
    return out


def optflow_workspace_bytes(B, H, W, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2,
                            flags=0):
    return int(lib.fs_optflow_workspace_bytes(C.byref(
        _flow_args(B, H, W, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags))))


def motion_mask(flow, P2, rel_pose, threshold=5.0, mode=0):
    """epipolar motion mask of B flows (base_precompute_hooks.py:58-89 for mode 0, :109-148 for mode 1).
    flow: device fp32 [B,H,W,2]; P2 [B,3,4] and rel_pose [B,4,4] (any float dtype, any device; used in f64).
    Returns uint8 [B,H,W] of 0 / 1."""
    if int(mode) not in (0, 1):
        raise ValueError("motion_mask: mode must be 0 (|d| > thr) or 1 (|d| / |flow| > thr), got %r" % (mode,))
    assert flow.is_cuda and flow.dim() == 4 and flow.shape[-1] == 2
    B, H, W, _ = flow.shape
    flow = flow.float().contiguous()
    P2 = torch.as_tensor(P2).to(flow.device, torch.float64).reshape(B, 3, 4).contiguous()
    pose = torch.as_tensor(rel_pose).to(flow.device, torch.float64).reshape(B, 4, 4).contiguous()
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=flow.device)
    a = FsMotionMaskArgs()
    a.flow, a.P2, a.pose, a.mask = flow.data_ptr(), P2.data_ptr(), pose.data_ptr(), mask.data_ptr()
    a.threshold, a.mode, a.B, a.H, a.W = float(threshold), int(mode), B, H, W
    check(lib.fs_motion_mask(C.byref(a), stream_ptr()), "motion_mask")
    return mask


def augment_masks(src, H, W, minv=None, dims=None, iplan=None):
    """uint8 ground-truth masks [B,Hs,Ws] (device) through the augmentation plan of fs_augment_frames (minv [B,6] f64 +
    iplan [B,8] int32) or fs_resize_frames (dims [B,4] int32, iplan optional) -> fp32 [B,H,W]"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3
    if (minv is None) == (dims is None):
        raise ValueError("augment_masks: exactly one of minv (warp) and dims (resize) is needed")
    B, Hs, Ws = src.shape
    src = src.contiguous()
    out = torch.empty(B, H, W, dtype=torch.float32, device=src.device)
    check(lib.fs_augment_masks(src.data_ptr(), _p(minv), _p(dims), _p(iplan), out.data_ptr(), B, Hs, Ws, H, W,
                               stream_ptr()), "augment_masks")
    return out


def augment_masks_ext(src, H, W, dims, win, minv=None):
    """the same masks through the windowed plan of fs_augment_frames_ext (minv [B,6] f64) or fs_resize_frames_ext
    (minv None): dims [B,4] int32, win [B,8] int32 -> fp32 [B,H,W]"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3
    B, Hs, Ws = src.shape
    src = src.contiguous()
    out = torch.empty(B, H, W, dtype=torch.float32, device=src.device)
    check(lib.fs_augment_masks_ext(src.data_ptr(), _p(minv), _p(dims), _p(win), out.data_ptr(), B, Hs, Ws, H, W,
                                   stream_ptr()), "augment_masks_ext")
    return out


# ---------------------------------------------------------------------------------------------
# self-distillation
# ---------------------------------------------------------------------------------------------
def sigmoid_head_fwd(logits):
    """logits: fp32 NHWC [N,H,W,Cp] whose channel 0 is the head output -> u [N,1,H,W] fp32"""
    N, H, W, Cp = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    u = torch.empty(N, 1, H, W, dtype=torch.float32, device=logits.device)
    check(lib.fs_sigmoid_head_fwd(logits.data_ptr(), u.data_ptr(), N * H * W, Cp, stream_ptr()), "sigmoid_head_fwd")
    return u


def sigmoid_head_bwd(u, du, Cp, dtype):
    """-> gradient w.r.t. the head's conv output, NHWC [N,H,W,Cp] in `dtype` (channels 1.. are zero)"""
    N, _, H, W = u.shape
    du = du.contiguous().float()
    dl = torch.empty(N, H, W, Cp, dtype=dtype, device=u.device)
    check(lib.fs_sigmoid_head_bwd(u.data_ptr(), du.data_ptr(), dl.data_ptr(), N * H * W, Cp, dtype_code(dtype),
                                  stream_ptr()), "sigmoid_head_bwd")
    return dl


def distill_fwd(pred, teacher, uncertain=None):
    """mean over all elements of |teacher - pred| (/ uncertain + log(uncertain + 1e-5)) as an f64 device scalar"""
    assert pred.shape == teacher.shape and pred.dtype == teacher.dtype == torch.float32
    pred, teacher = pred.contiguous(), teacher.contiguous()
    if uncertain is not None:
        assert uncertain.shape == pred.shape and uncertain.dtype == torch.float32
        uncertain = uncertain.contiguous()
    acc = torch.zeros((), dtype=torch.float64, device=pred.device)
    check(lib.fs_distill_fwd(pred.data_ptr(), teacher.data_ptr(), _p(uncertain), pred.numel(), acc.data_ptr(),
                             stream_ptr()), "distill_fwd")
    return acc / pred.numel()


def distill_bwd(pred, teacher, uncertain, gout):
    d_pred = torch.empty_like(pred)
    d_unc = torch.empty_like(uncertain) if uncertain is not None else None
    check(lib.fs_distill_bwd(pred.data_ptr(), teacher.data_ptr(), _p(uncertain), pred.numel(), _p(gout), d_pred.data_ptr(),
                             _p(d_unc), stream_ptr()), "distill_bwd")
    return d_pred, d_unc


def distill_unscaled_chunk():
    """elements of a plane that one block of the scale-aligned distillation kernels covers"""
    return int(lib.fs_distill_unscaled_chunk())


def distill_unscaled_fwd(preds, teachers, uncertains=None):
    """is_unscaled_distill: per (sample, channel) plane ratio = mean(pred / (teacher + 1e-5)), then the mean over all
    elements of |ratio * teacher - pred| (/ uncertain + log(uncertain + 1e-5)), for 1..4 scales in one call.
    preds, teachers (and uncertains): lists of fp32 [B,C,h_s,w_s] with one B*C.
    -> (f64 [S] losses on the device, context for distill_unscaled_bwd).  No host sync."""
    S = len(preds)
    assert 1 <= S <= 4 and len(teachers) == S and (uncertains is None or len(uncertains) == S)
    planes = preds[0].shape[0] * preds[0].shape[1]
    a = FsDistillUnscaledArgs()
    keep = []
    for s in range(S):
        p, t = preds[s], teachers[s]
        assert p.dim() == 4 and p.shape == t.shape and p.dtype == t.dtype == torch.float32
        assert p.shape[0] * p.shape[1] == planes, "every scale has the same number of planes"
        p, t = p.contiguous(), t.contiguous()
        a.pred[s], a.teacher[s], a.n[s] = p.data_ptr(), t.data_ptr(), p.shape[2] * p.shape[3]
        keep += [p, t]
        if uncertains is not None:
            u = uncertains[s]
            assert u.shape == p.shape and u.dtype == torch.float32
            u = u.contiguous()
            a.uncertain[s] = u.data_ptr()
            keep.append(u)
    a.planes, a.S = planes, S
    nbytes = int(lib.fs_distill_unscaled_workspace_bytes(planes, C.addressof(a.n), S))
    if nbytes < 0:
        check(1, "distill_unscaled_workspace_bytes")
    dev = preds[0].device
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    losses = torch.empty(S, dtype=torch.float64, device=dev)
    a.workspace, a.loss_out = ws.data_ptr(), losses.data_ptr()
    check(lib.fs_distill_unscaled_fwd(C.byref(a), stream_ptr()), "distill_unscaled_fwd")
    return losses, (a, keep, ws, [preds[s].shape for s in range(S)], uncertains is not None, dev)


def distill_unscaled_bwd(ctx, gouts=None):
    """gouts: f64 [S] on the device (None: ones) -> (d_pred[s], d_uncertain[s] or None), fresh tensors"""
    a, keep, ws, shapes, unc, dev = ctx
    d_pred = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
    d_unc = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes] if unc else None
    if gouts is not None:
        assert gouts.dtype == torch.float64 and gouts.numel() == a.S and gouts.is_contiguous()
    for s in range(a.S):
        a.d_pred[s] = d_pred[s].data_ptr()
        a.d_uncertain[s] = d_unc[s].data_ptr() if unc else None
    a.gout = _p(gouts)
    check(lib.fs_distill_unscaled_bwd(C.byref(a), stream_ptr()), "distill_unscaled_bwd")
    return d_pred, d_unc


COST_VOLUME_MAX_BINS = 128


def cost_volume(cur, look, K, inv_K, poses, bins, cat, want_volume=False):
    """Plane-sweep matching cost volume of a whole batch in one launch (fs_cost_volume; resnet_matching.py:83-173, 227-237).
    cur [B,h,w,C] and look [B*F,h,w,C]: NHWC features in the compute dtype; K, inv_K [B,4,4], poses [B,F,4,4], bins [D]:
    fp32 on the device; cat [B,h,w,Ci_p] in the compute dtype: channels [C, C+D) receive cost * confidence, the padding
    channels behind them zero, channels [0, C) stay as they are.
    -> (confidence [B,h,w], lowest_cost [B,h,w]) fp32, and with want_volume the filled, unmasked fp32 cost volume and the
    missing mask, both [B,D,h,w].  No host sync."""
    if cur.dim() != 4 or look.dim() != 4 or cat.dim() != 4 or poses.dim() != 4 or bins.dim() != 1:
        raise ValueError("cost_volume: cur / look / cat are NHWC, poses [B,F,4,4], bins [D]")
    B, h, w, Cc = cur.shape
    F, D = poses.shape[1], bins.shape[0]
    if Cc < 16 or Cc % 16:
        raise ValueError("cost_volume: the feature width must be a positive multiple of 16, got %d" % Cc)
    if not 1 <= D <= COST_VOLUME_MAX_BINS:
        raise ValueError("cost_volume: 1 <= depth bins <= %d, got %d" % (COST_VOLUME_MAX_BINS, D))
    if F < 1 or h < 5 or w < 5:
        raise ValueError("cost_volume: needs F >= 1 and h, w >= 5, got F=%d h=%d w=%d" % (F, h, w))
    if cur.dtype not in (torch.float32, torch.bfloat16) or look.dtype != cur.dtype or cat.dtype != cur.dtype:
        raise ValueError("cost_volume: cur, look and cat share one compute dtype (fp32 or bf16)")
    if tuple(look.shape) != (B * F, h, w, Cc) or tuple(poses.shape) != (B, F, 4, 4) or tuple(K.shape) != (B, 4, 4) \
            or tuple(inv_K.shape) != (B, 4, 4) or tuple(cat.shape[:3]) != (B, h, w) or cat.shape[3] < Cc + D:
        raise ValueError("cost_volume: shapes disagree (cur %s look %s poses %s K %s inv_K %s cat %s)" % (
            tuple(cur.shape), tuple(look.shape), tuple(poses.shape), tuple(K.shape), tuple(inv_K.shape), tuple(cat.shape)))
    for name, t in (("K", K), ("inv_K", inv_K), ("poses", poses), ("bins", bins)):
        if t.dtype != torch.float32 or t.device != cur.device or not t.is_contiguous():
            raise ValueError("cost_volume: %s must be a contiguous fp32 tensor on the features' device" % name)
    if not (cur.is_contiguous() and look.is_contiguous() and cat.is_contiguous()):
        raise ValueError("cost_volume: cur, look and cat must be dense NHWC")
    if B * h * w >= 1 << 31 or h * w * Cc >= 1 << 31:
        raise ValueError("cost_volume: B*h*w and h*w*C must stay below 2^31")
    dev = cur.device
    conf = torch.empty(B, h, w, dtype=torch.float32, device=dev)
    lowest = torch.empty(B, h, w, dtype=torch.float32, device=dev)
    vol = torch.empty(B, D, h, w, dtype=torch.float32, device=dev) if want_volume else None
    miss = torch.empty(B, D, h, w, dtype=torch.float32, device=dev) if want_volume else None
    check(lib.fs_cost_volume(cur.data_ptr(), look.data_ptr(), K.data_ptr(), inv_K.data_ptr(), poses.data_ptr(),
                             bins.data_ptr(), cat.data_ptr(), conf.data_ptr(), lowest.data_ptr(), _p(vol), _p(miss),
                             B, F, h, w, Cc, D, cat.shape[3], dtype_code(cur.dtype), stream_ptr()), "cost_volume")
    if want_volume:
        return conf, lowest, vol, miss
    return conf, lowest


# ---------------------------------------------------------------------------------- deformable convolution (dcn.hip)
def dcn_tile(which):
    """(pixels, channels) one block owns: which = 0 forward, 1 data backward, 2 weight gradient (fs_dcn_tile)"""
    px, ch = C.c_int32(), C.c_int32()
    check(lib.fs_dcn_tile(which, C.byref(px), C.byref(ch)), "dcn_tile")
    return px.value, ch.value


DCN_MAX_PAD = DCN_MAX_DIL = 64          # what check_geometry of dcn.hip takes


class DcnGeometry:
    """Shapes and options of one deformable convolution (deform_conv.py:54-223).  What the kernels do not take raises
    NotImplementedError naming the option — on any device, before anything is launched."""

    def __init__(self, in_shape, w_shape, stride, padding, dilation, groups, deformable_groups, dtype):
        self.N, self.Ci, self.H, self.W = (int(v) for v in in_shape)
        self.Co, ci_w, self.R, self.S = (int(v) for v in w_shape)
        self.stride, self.padding, self.dilation = (tuple(int(v) for v in _pair(o)) for o in (stride, padding, dilation))
        self.groups, self.dg = int(groups), int(deformable_groups)
        self.dtype, self.code = dtype, dtype_code(dtype)
        self.EG = 8 if dtype == torch.bfloat16 else 4
        if self.groups != 1:
            raise NotImplementedError("deformable convolution: groups=%d is not supported (groups must be 1)" % self.groups)
        if self.R > 3 or self.S > 3:
            raise NotImplementedError("deformable convolution: kernel_size=%dx%d is not supported (at most 3x3)" % (self.R, self.S))
        if any(s not in (1, 2) for s in self.stride):
            raise NotImplementedError("deformable convolution: stride=%s is not supported (1 or 2)" % (self.stride,))
        if any(not 0 <= v <= DCN_MAX_PAD for v in self.padding):
            raise NotImplementedError("deformable convolution: padding=%s is not supported (0 .. %d)" % (self.padding, DCN_MAX_PAD))
        if any(not 1 <= v <= DCN_MAX_DIL for v in self.dilation):
            raise NotImplementedError("deformable convolution: dilation=%s is not supported (1 .. %d)" % (self.dilation, DCN_MAX_DIL))
        if ci_w != self.Ci:
            raise ValueError("deformable convolution: weight expects %d input channels, input has %d" % (ci_w, self.Ci))
        if self.dg < 1 or self.Ci % self.dg:
            raise ValueError("deformable convolution: deformable_groups=%d does not divide %d channels" % (self.dg, self.Ci))
        if self.dg > 1 and (self.Ci // self.dg) % self.EG:
            raise NotImplementedError("deformable convolution: deformable_groups=%d leaves %d channels per group, not a "
                                      "multiple of %d (whole 16-byte units)" % (self.dg, self.Ci // self.dg, self.EG))
        self.Ci_p, self.Co_p = roundup(self.Ci, self.EG), roundup(self.Co, 16)
        ext = [(i + 2 * p - (d * (k - 1) + 1)) // s + 1 for i, p, d, k, s in
               zip((self.H, self.W), self.padding, self.dilation, (self.R, self.S), self.stride)]
        if min(ext) < 1:
            raise ValueError("convolution input is too small (output would be %dx%d)" % tuple(ext))
        self.Ho, self.Wo = ext
        self.RS = self.R * self.S

    def args(self):
        a = FsDcnArgs()
        a.N, a.H, a.W, a.Ho, a.Wo = self.N, self.H, self.W, self.Ho, self.Wo
        a.Ci, a.Ci_p, a.Co, a.Co_p, a.R, a.S = self.Ci, self.Ci_p, self.Co, self.Co_p, self.R, self.S
        a.stride_h, a.stride_w = self.stride
        a.pad_h, a.pad_w = self.padding
        a.dil_h, a.dil_w = self.dilation
        a.groups, a.deformable_groups = self.groups, self.dg
        return a

    def forward_channels(self):
        """output channels one forward block owns for this geometry (fs_dcn_fwd_channels)"""
        a = self.args()
        return int(lib.fs_dcn_fwd_channels(C.byref(a), self.code))

    def check_offset(self, offset, mask):
        want = (self.N, self.dg * 2 * self.RS, self.Ho, self.Wo)
        if tuple(offset.shape) != want:
            raise ValueError("deformable convolution: offset is %s, expected %s" % (tuple(offset.shape), want))
        if mask is not None and tuple(mask.shape) != (self.N, self.dg * self.RS, self.Ho, self.Wo):
            raise ValueError("deformable convolution: mask is %s, expected %s" % (
                tuple(mask.shape), (self.N, self.dg * self.RS, self.Ho, self.Wo)))


def _dcn_common(g, x, offset, mask):
    assert x.shape == (g.N, g.H, g.W, g.Ci_p) and x.dtype == g.dtype and x.is_contiguous()
    assert offset.dtype == torch.float32 and offset.is_contiguous()
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous())
    a = g.args()
    a.x, a.offset, a.mask = x.data_ptr(), offset.data_ptr(), _p(mask)
    return a


def dcn_pack(g, weight, transpose):
    """fp32 OIHW master -> the forward operand [Co_p][R*S*Ci_p] (transpose = 0) or the data-gradient operand
    [roundup(Ci_p, 16)][R*S*Co_p] (transpose = 1) in the compute dtype (fs_pack_weights)"""
    w = weight.detach().float().contiguous()
    rows, cs = (roundup(g.Ci_p, 16), g.Co_p) if transpose else (g.Co_p, g.Ci_p)
    dst = torch.empty(rows, g.RS * cs, dtype=g.dtype, device=w.device)
    check(lib.fs_pack_weights(w.data_ptr(), dst.data_ptr(), g.Co, g.Ci, g.R, g.S, rows, cs, g.RS * cs, int(transpose),
                              g.code, stream_ptr()), "pack_weights")
    return dst


def dcn_forward(g, x, offset, mask, w_f, bias=None, out=None):
    """x NHWC [N,H,W,Ci_p] -> out NHWC [N,Ho,Wo,Co_p], both in the compute dtype; offset / mask fp32 planar; bias fp32 [Co]"""
    a = _dcn_common(g, x, offset, mask)
    if out is None:
        out = torch.empty(g.N, g.Ho, g.Wo, g.Co_p, dtype=g.dtype, device=x.device)
    a.w_f, a.w_f_row, a.bias, a.out = w_f.data_ptr(), w_f.shape[1], _p(bias), out.data_ptr()
    check(lib.fs_dcn_fwd(C.byref(a), g.code, stream_ptr()), "dcn_fwd")
    return out


def dcn_backward_data(g, x, offset, mask, w_d, dy, dx=None, d_offset=None, d_mask=None):
    """-> (dx fp32 NHWC [N,H,W,Ci_p], d_offset, d_mask | None); every cell of the three is written"""
    a = _dcn_common(g, x, offset, mask)
    assert dy.shape == (g.N, g.Ho, g.Wo, g.Co_p) and dy.dtype == g.dtype and dy.is_contiguous()
    dev = x.device
    dx = torch.empty(g.N, g.H, g.W, g.Ci_p, dtype=torch.float32, device=dev) if dx is None else dx
    d_offset = torch.empty_like(offset) if d_offset is None else d_offset
    if mask is not None and d_mask is None:
        d_mask = torch.empty_like(mask)
    a.w_d, a.w_d_row, a.dy = w_d.data_ptr(), w_d.shape[1], dy.data_ptr()
    a.dx, a.d_offset, a.d_mask = dx.data_ptr(), d_offset.data_ptr(), _p(d_mask)
    check(lib.fs_dcn_bwd_data(C.byref(a), g.code, stream_ptr()), "dcn_bwd_data")
    return dx, d_offset, d_mask


def dcn_backward_weight(g, x, offset, mask, dy, want_bias=False, dw=None, d_bias=None):
    """-> (dw fp32 OIHW, d_bias fp32 [Co] | None), both in a fixed summation order"""
    a = _dcn_common(g, x, offset, mask)
    assert dy.shape == (g.N, g.Ho, g.Wo, g.Co_p) and dy.dtype == g.dtype and dy.is_contiguous()
    dev = x.device
    dw = torch.empty(g.Co, g.Ci, g.R, g.S, dtype=torch.float32, device=dev) if dw is None else dw
    if want_bias and d_bias is None:
        d_bias = torch.empty(g.Co, dtype=torch.float32, device=dev)
    nbytes = int(lib.fs_dcn_workspace_bytes(C.byref(a), g.code))
    if nbytes < 0:
        raise ValueError("deformable convolution: the library refuses this geometry")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    a.dy, a.dw, a.d_bias = dy.data_ptr(), dw.data_ptr(), _p(d_bias)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.fs_dcn_bwd_weight(C.byref(a), g.code, stream_ptr()), "dcn_bwd_weight")
    return dw, d_bias


# ---------------------------------------------------------------------------------- DLA backbone (dla.hip)
def _pixel_stride(t):
    """elements between neighbouring pixels of an NHWC view whose pixels are evenly spaced: a dense tensor, or a channel
    slice of one (the strides torch reports for dimensions of size 1 mean nothing and are not looked at)"""
    N, H, W, Cc = t.shape
    if t.is_contiguous():
        return Cc
    pix = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else t.stride(0))
    assert t.stride(3) == 1 and pix >= Cc
    assert (H == 1 or t.stride(1) == W * pix) and (N == 1 or t.stride(0) == H * W * pix)
    return pix


def pool2_fwd(x, out=None):
    """nn.MaxPool2d(2, stride=2) of dense NHWC x -> (y, idx).  out: a [N,H/2,W/2,C] view with contiguous channels whose
    pixels are evenly spaced (a channel slice of a wider dense buffer) that receives y instead of a fresh tensor."""
    N, H, W, Cc = x.shape
    assert x.is_contiguous()
    Ho, Wo = H // 2, W // 2
    if out is None:
        out = torch.empty(N, Ho, Wo, Cc, dtype=x.dtype, device=x.device)
    assert out.shape == (N, Ho, Wo, Cc) and out.dtype == x.dtype
    pix = _pixel_stride(out)
    idx = torch.empty(N, Ho, Wo, Cc, dtype=torch.uint8, device=x.device)
    _timed("pool2_fwd", x.numel() * x.element_size() * 1.25 + idx.numel(),
           lambda: check(lib.fs_pool2_fwd(x.data_ptr(), out.data_ptr(), idx.data_ptr(), N, H, W, Cc, pix, 0,
                                          dtype_code(x.dtype), stream_ptr()), "pool2_fwd"), tag=str(tuple(x.shape)))
    return out, idx


def pool2_bwd(dy, idx, H, W, addend=None):
    """gradient of pool2_fwd's input (+ addend, dense like it); dy may be a channel slice of a wider dense buffer"""
    N, Ho, Wo, Cc = dy.shape
    pix = _pixel_stride(dy)
    assert idx.is_contiguous() and idx.shape == dy.shape and H == 2 * Ho and W == 2 * Wo
    assert addend is None or (addend.is_contiguous() and addend.shape == (N, H, W, Cc) and addend.dtype == dy.dtype)
    dx = torch.empty(N, H, W, Cc, dtype=dy.dtype, device=dy.device)
    _timed("pool2_bwd", dx.numel() * dx.element_size() * (1.25 + (addend is not None)) + idx.numel(),
           lambda: check(lib.fs_pool2_bwd(dy.data_ptr(), idx.data_ptr(), _p(addend), dx.data_ptr(), N, H, W, Cc, pix, 0,
                                          dtype_code(dy.dtype), stream_ptr()), "pool2_bwd"), tag=str(tuple(dx.shape)))
    return dx


def _cat_args(wide, parts, offs, widths, accumulate):
    a = FsCatArgs()
    assert wide.is_contiguous() and len(parts) == len(offs) == len(widths)
    a.wide, a.Ctot, a.M, a.n = wide.data_ptr(), wide.shape[-1], wide.numel() // wide.shape[-1], len(parts)
    for i, (t, o, c) in enumerate(zip(parts, offs, widths)):
        if i >= FS_CAT_MAX:
            break                    # (the library refuses n > FS_CAT_MAX)
        assert t is None or (t.is_contiguous() and t.shape[-1] == c and t.numel() == a.M * c and t.dtype == wide.dtype)
        a.part[i], a.off[i], a.C[i] = _p(t), o, c
        a.accumulate[i] = int(bool(accumulate[i])) if accumulate is not None else 0
    return a


def cat_fwd(wide, parts, offs, widths):
    """channel slices [offs[i], offs[i] + widths[i]) of dense NHWC `wide` <- dense parts[i] (None: already there), ONE
    launch for up to FS_CAT_MAX parts"""
    a = _cat_args(wide, parts, offs, widths, None)
    nb = 2 * sum(t.numel() for t in parts if t is not None) * wide.element_size()
    _timed("cat_fwd", nb, lambda: check(lib.fs_cat_fwd(C.byref(a), dtype_code(wide.dtype), stream_ptr()), "cat_fwd"),
           tag=str(tuple(wide.shape)))
    return wide


def cat_bwd(wide, parts, offs, widths, accumulate=None):
    """dense parts[i] = (accumulate[i]: +=) channel slice i of `wide` (None: skipped), ONE launch"""
    a = _cat_args(wide, parts, offs, widths, accumulate)
    nb = sum(t.numel() * (2 + bool(accumulate and accumulate[i])) for i, t in enumerate(parts) if t is not None) * wide.element_size()
    _timed("cat_bwd", nb, lambda: check(lib.fs_cat_bwd(C.byref(a), dtype_code(wide.dtype), stream_ptr()), "cat_bwd"),
           tag=str(tuple(wide.shape)))
    return parts


# ---------------------------------------------------------------------------------- ConvNeXt backbone (convnext.hip)
def _rows(t):
    """dense [..., Cp] -> (rows, Cp)"""
    assert t.is_contiguous()
    return t.numel() // t.shape[-1], t.shape[-1]


def _is_f32(t, code):
    return int(t.dtype == torch.float32 and code != dtype_code(torch.float32))


def _check_kind(t, dtype):
    assert t.dtype in (dtype, torch.float32), (t.dtype, dtype)


def dwconv7_tile(dtype):
    """(rows, columns, channels) of the outputs one fs_dwconv7_fwd block owns"""
    r, c, ch = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.fs_dwconv7_tile(dtype_code(dtype), C.byref(r), C.byref(c), C.byref(ch)), "dwconv7_tile")
    return r.value, c.value, ch.value


def dwconv7_table(weight, bias, Cp):
    """[C,1,7,7] (+ [C]) fp32 -> the tap-major table [49][Cp] and the padded bias [Cp] the kernels read"""
    Cc = weight.shape[0]
    tab = torch.zeros(49, Cp, dtype=torch.float32, device=weight.device)
    tab[:, :Cc] = weight.detach().reshape(Cc, 49).t()
    b = None
    if bias is not None:
        b = torch.zeros(Cp, dtype=torch.float32, device=weight.device)
        b[:Cc] = bias.detach()
    return tab, b


def dwconv7_fwd(x, tab, bias, Cc, dtype, out_dtype=None, flip=False, addend=None, out=None):
    """depthwise 7x7 / pad 3 of dense NHWC x [N,H,W,Cp] (compute dtype or fp32) -> out in out_dtype (compute dtype or fp32);
    flip + addend: the data gradient (x = dy, addend = the residual path's gradient, in the compute dtype or fp32)"""
    N, H, W, Cp = x.shape
    code = dtype_code(dtype)
    _check_kind(x, dtype)
    out_dtype = out_dtype or dtype
    if out is None:
        out = torch.empty(N, H, W, Cp, dtype=out_dtype, device=x.device)
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and tab.shape == (49, Cp)
    assert addend is None or (addend.is_contiguous() and addend.shape == out.shape and addend.dtype in (dtype, torch.float32))
    a = FsDwconv7Args()
    a.x, a.wtab, a.bias, a.addend, a.out = x.data_ptr(), tab.data_ptr(), _p(bias), _p(addend), out.data_ptr()
    a.N, a.H, a.W, a.C, a.Cp = N, H, W, Cc, Cp
    a.x_f32, a.out_f32, a.flip = _is_f32(x, code), _is_f32(out, code), int(bool(flip))
    a.addend_f32 = _is_f32(addend, code) if addend is not None else 0
    _timed("dwconv7_bwd_data" if flip else "dwconv7_fwd", 2.0 * 49 * N * H * W * Cc,
           lambda: check(lib.fs_dwconv7_fwd(C.byref(a), code, stream_ptr()), "dwconv7_fwd"), tag=str(tuple(x.shape)))
    return out


def dwconv7_bwd_weight(dy, x, Cc, dw=None, dbias=None, accumulate=False, want_weight=True, want_bias=True):
    """-> (dw fp32 [C,1,7,7], dbias fp32 [C]) in a fixed summation order; dy in the compute dtype, x in it or fp32.
    dw / dbias given: written (accumulate: added to) in place; a None with want_* False is skipped"""
    N, H, W, Cp = x.shape
    dtype = dy.dtype
    code = dtype_code(dtype)
    _check_kind(x, dtype)
    assert x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape
    dev = x.device
    if dw is None and want_weight:
        assert not accumulate
        dw = torch.empty(Cc, 1, 7, 7, dtype=torch.float32, device=dev)
    if dbias is None and want_bias:
        assert not accumulate
        dbias = torch.empty(Cc, dtype=torch.float32, device=dev)
    nbytes = int(lib.fs_dwconv7_workspace_bytes(N, H, W, Cp))
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    a = FsDwconv7Args()
    a.x, a.dy, a.dw, a.dbias = x.data_ptr(), dy.data_ptr(), _p(dw), _p(dbias)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.N, a.H, a.W, a.C, a.Cp = N, H, W, Cc, Cp
    a.x_f32, a.accumulate = _is_f32(x, code), int(bool(accumulate))
    _timed("dwconv7_bwd_weight", 2.0 * 49 * N * H * W * Cc,
           lambda: check(lib.fs_dwconv7_bwd_weight(C.byref(a), code, stream_ptr()), "dwconv7_bwd_weight"), tag=str(tuple(x.shape)))
    return dw, dbias


def layernorm_fwd(x, gamma, beta, eps, dtype, out_dtype=None):
    """LayerNorm over the C = gamma.numel() real channels of dense [..., Cp] x -> (y, mean, rstd)"""
    M, Cp = _rows(x)
    code = dtype_code(dtype)
    _check_kind(x, dtype)
    y = torch.empty(x.shape, dtype=out_dtype or dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    a = FsLayerNormArgs()
    a.x, a.gamma, a.beta, a.y, a.mean, a.rstd = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    a.M, a.C, a.Cp, a.eps = M, gamma.numel(), Cp, float(eps)
    a.x_f32, a.y_f32 = _is_f32(x, code), _is_f32(y, code)
    _timed("layernorm_fwd", x.numel() * (x.element_size() + y.element_size()),
           lambda: check(lib.fs_layernorm_fwd(C.byref(a), code, stream_ptr()), "layernorm_fwd"), tag=str(tuple(x.shape)))
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dtype, addend=None, dgamma=None, dbeta=None, accumulate=False, want_dx=True):
    """-> dx (typed like x; + addend) or None; dgamma / dbeta (fp32 [C], given): written (accumulate: added to) in slab order"""
    M, Cp = _rows(x)
    code = dtype_code(dtype)
    _check_kind(x, dtype)
    _check_kind(dy, dtype)
    assert dy.is_contiguous() and dy.shape == x.shape
    assert addend is None or (addend.is_contiguous() and addend.shape == x.shape)
    dx = torch.empty_like(x) if want_dx else None
    a = FsLayerNormArgs()
    a.x, a.gamma, a.dy, a.addend, a.dx = x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), _p(addend), _p(dx)
    a.mean, a.rstd, a.dgamma, a.dbeta = mean.data_ptr(), rstd.data_ptr(), _p(dgamma), _p(dbeta)
    ws = None
    if dgamma is not None or dbeta is not None:
        nbytes = int(lib.fs_layernorm_workspace_bytes(M, Cp))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.M, a.C, a.Cp = M, gamma.numel(), Cp
    a.x_f32, a.y_f32, a.accumulate = _is_f32(x, code), _is_f32(dy, code), int(bool(accumulate))
    a.addend_f32 = _is_f32(addend, code) if addend is not None else 0
    _timed("layernorm_bwd", x.numel() * (2 * x.element_size() + 2 * dy.element_size()),
           lambda: check(lib.fs_layernorm_bwd(C.byref(a), code, stream_ptr()), "layernorm_bwd"), tag=str(tuple(x.shape)))
    return dx


def gelu_fwd(x):
    """exact (erf) GELU of a dense tensor in the compute dtype"""
    assert x.is_contiguous()
    y = torch.empty_like(x)
    _timed("gelu_fwd", 2 * x.numel() * x.element_size(),
           lambda: check(lib.fs_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), dtype_code(x.dtype), stream_ptr()), "gelu_fwd"),
           tag=str(tuple(x.shape)))
    return y


def gelu_bwd(x, dy):
    """dy * gelu'(x), x the pre-activation"""
    assert x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape and dy.dtype == x.dtype
    dx = torch.empty_like(x)
    _timed("gelu_bwd", 3 * x.numel() * x.element_size(),
           lambda: check(lib.fs_gelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), dtype_code(x.dtype), stream_ptr()),
                         "gelu_bwd"), tag=str(tuple(x.shape)))
    return dx


def _scale_residual_args(ref, Cc, code):
    N, Cp = ref.shape[0], ref.shape[-1]
    a = FsScaleResidualArgs()
    a.N, a.HW, a.C, a.Cp = N, ref.numel() // (N * Cp), Cc, Cp
    a.stream_f32 = _is_f32(ref, code)
    return a


def scale_residual_fwd(inp, z, gamma, keep, Cc, want_copy=False):
    """out = inp + keep[n] * gamma[c] * z -> (out typed like inp, its copy in z's dtype or None); gamma / keep None: ones"""
    code = dtype_code(z.dtype)
    _check_kind(inp, z.dtype)
    assert inp.is_contiguous() and z.is_contiguous() and inp.shape == z.shape
    out = torch.empty_like(inp)
    copy = torch.empty_like(z) if want_copy else None
    a = _scale_residual_args(inp, Cc, code)
    a.inp, a.z, a.gamma, a.keep, a.out, a.out_c = inp.data_ptr(), z.data_ptr(), _p(gamma), _p(keep), out.data_ptr(), _p(copy)
    _timed("scale_residual_fwd", inp.numel() * (2 * inp.element_size() + z.element_size()),
           lambda: check(lib.fs_scale_residual_fwd(C.byref(a), code, stream_ptr()), "scale_residual_fwd"), tag=str(tuple(z.shape)))
    return out, copy


def scale_residual_bwd(dout, z, gamma, keep, Cc, dtype, dgamma=None, dbias=None, accumulate=False):
    """-> dz = keep[n] * gamma[c] * dout in the compute dtype; dgamma (fp32 [C], given): sum keep[n] * dout * z; dbias (fp32
    [C], given): gamma[c] * sum keep[n] * dout, the gradient of the bias behind z; both in slab order"""
    code = dtype_code(dtype)
    _check_kind(dout, dtype)
    assert dout.is_contiguous() and (z is None or (z.is_contiguous() and z.shape == dout.shape and z.dtype == dtype))
    dz = torch.empty(dout.shape, dtype=dtype, device=dout.device)
    a = _scale_residual_args(dout, Cc, code)
    a.dout, a.z, a.gamma, a.keep, a.dz, a.dgamma = dout.data_ptr(), _p(z), _p(gamma), _p(keep), dz.data_ptr(), _p(dgamma)
    a.dbias = _p(dbias)
    ws = None
    if dgamma is not None or dbias is not None:
        nbytes = int(lib.fs_scale_residual_workspace_bytes(a.N * a.HW, a.Cp))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dout.device)
        a.workspace, a.workspace_bytes, a.accumulate = ws.data_ptr(), nbytes, int(bool(accumulate))
    _timed("scale_residual_bwd", dout.numel() * (dout.element_size() + 2 * dz.element_size()),
           lambda: check(lib.fs_scale_residual_bwd(C.byref(a), code, stream_ptr()), "scale_residual_bwd"), tag=str(tuple(dout.shape)))
    return dz


def bias_grad(x, dbias, accumulate=True):
    """dbias[c] (+)= column sums of dense x [..., Cp], c < dbias.numel(), in a fixed order"""
    M, Cp = _rows(x)
    nbytes = int(lib.fs_scale_residual_workspace_bytes(M, Cp))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    code = dtype_code(x.dtype)
    _timed("bias_grad", x.numel() * x.element_size(),
           lambda: check(lib.fs_bias_grad(x.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, M, dbias.numel(), Cp, 0,
                                          int(bool(accumulate)), code, stream_ptr()), "bias_grad"), tag=str(tuple(x.shape)))
    return dbias


def patch_gather(x, k):
    """dense NHWC [N,H,W,Cp] -> [N,H//k,W//k,k*k*Cp] in (r, s, c) order: the operand of a kernel-k / stride-k convolution as a
    1x1 one"""
    N, H, W, Cp = x.shape
    assert x.is_contiguous()
    out = torch.empty(N, H // k, W // k, k * k * Cp, dtype=x.dtype, device=x.device)
    _timed("patch_gather", 2 * out.numel() * x.element_size(),
           lambda: check(lib.fs_patch_gather(x.data_ptr(), out.data_ptr(), N, H, W, Cp, k, dtype_code(x.dtype), stream_ptr()),
                         "patch_gather"), tag=str(tuple(x.shape)))
    return out


def patch_scatter(dg, H, W, k):
    """the inverse: [N,H//k,W//k,k*k*Cp] -> [N,H,W,Cp], zero in the rows and columns the floor drops"""
    N, Ho, Wo, K = dg.shape
    Cp = K // (k * k)
    assert dg.is_contiguous() and Ho == H // k and Wo == W // k and Cp * k * k == K
    dx = torch.empty(N, H, W, Cp, dtype=dg.dtype, device=dg.device)
    _timed("patch_scatter", 2 * dx.numel() * dg.element_size(),
           lambda: check(lib.fs_patch_scatter(dg.data_ptr(), dx.data_ptr(), N, H, W, Cp, k, dtype_code(dg.dtype), stream_ptr()),
                         "patch_scatter"), tag=str(tuple(dx.shape)))
    return dx
