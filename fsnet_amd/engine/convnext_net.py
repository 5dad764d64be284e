"""Manual forward / backward runner of the ConvNeXt backbone on the HIP library, in the manner of dla_net.DLARunner.  The
nn.Modules are parameter containers.

Reference structure followed (vision_base/networks/models/backbone/convnext.py):
  Block            :25-49     dwconv 7x7 -> LayerNorm -> Linear -> GELU -> Linear -> gamma * . -> input + drop_path(.)
  ConvNeXt.forward :116-124   downsample layer i, stage i, for i up to the last requested feature

Launches: the depthwise convolution, LayerNorm, GELU and the scaled residual are convnext.hip; the two Linear layers are 1x1
convolutions (ConvOp forward with bias, dgrad, weight gradient through HO.submit, as the pose decoder's; their bias
gradient is fs_bias_grad on the chain: fs_channel_sum joins its blocks with float atomics and is not reproducible).  The
patch convolutions (kernel == stride: 4 / 4 in the stem, 2 / 2 in front of stages 1-3) all take one route: fs_patch_gather
(space to depth, (r, s, c) order) and a 1x1 ConvOp over k * k * Cg channels, with fs_patch_scatter behind the data gradient.
Their [Co, Ci, k, k] parameter is held a second time as an fp32 master [Co, k * k * Cg] in the gathered order (zero in the
channel padding), refreshed when the parameter changes; the weight gradient is taken in that order on the chain and added
to the parameter's gradient through the inverse permutation.

Precision: the residual stream — the output of every downsample layer and of every block — is fp32 in both compute modes
(gamma starts at 1e-6: a bf16 stream would round every branch away).  GEMM and depthwise operands, LayerNorm outputs that
feed a GEMM, the hidden activations and the returned features are in the compute dtype; LayerNorm statistics, GELU and
every sum are fp32.  Channel padding: every tensor here has roundup(C, 16) channels; a ConvOp that wants fewer input
channels reads a channel slice.
"""
import torch

from ..hip import ops
from ..hip.conv import roundup
from .handover import HO
from .nets import ConvLayer
from .runtime import RT, grad_of, require_gpu


class _As1x1:
    """what ConvLayer's constructor, the pack registry and HO.submit read of a convolution module, for a layer that runs as a
    1x1 / stride-1 convolution: the geometry, and the live weight and bias through two getters"""
    kernel_size, stride, padding = (1, 1), (1, 1), (0, 0)

    def __init__(self, weight_of, bias_of):
        self._weight_of, self._bias_of = weight_of, bias_of

    weight = property(lambda self: self._weight_of())
    bias = property(lambda self: self._bias_of())


class _WeightOnly:
    """a layer as HO.submit sees it, without its bias (that gradient is taken elsewhere)"""

    def __init__(self, weight_of):
        self.m = _As1x1(weight_of, lambda: None)


class _LinearLayer(ConvLayer):
    """nn.Linear over NHWC rows as a 1x1 convolution: the [out, in] parameter is the OIHW master seen through a view"""

    def __init__(self, lin, need_dgrad=True):
        super().__init__(_As1x1(lambda: lin.weight, lambda: lin.bias), need_dgrad=need_dgrad)
        self._weight_only = _WeightOnly(lambda: lin.weight)

    def accumulate_param_grads(self, op, dc, x, pro=None, bias=True):
        """the weight gradient off the chain (HO.submit); the bias gradient on it, in a fixed order (fs_bias_grad) —
        bias=False: the caller has it from elsewhere"""
        HO.submit([(self._weight_only, op, dc, x, pro)])
        gb = grad_of(self.m.bias) if bias else None
        if gb is not None:
            ops.bias_grad(dc, gb)


class _PatchLayer(ConvLayer):
    """Conv2d(kernel k, stride k) as a 1x1 convolution over gathered patches: `m.weight` is `master`, the fp32 copy
    [Co, k*k*Cg] of the parameter in (r, s, c) order, rewritten from the parameter when that has changed"""

    def __init__(self, conv, stem):
        k = conv.kernel_size[0]
        if conv.kernel_size != (k, k) or conv.stride != (k, k) or conv.padding != (0, 0) or conv.groups != 1 \
                or conv.dilation != (1, 1) or conv.bias is None:
            raise NotImplementedError("ConvNeXt on the HIP engine: a patch convolution has kernel == stride, no padding, a bias")
        self.master = None
        super().__init__(_As1x1(lambda: self.master, lambda: conv.bias), need_dgrad=not stem)
        self.conv, self.k, self.stem = conv, k, stem
        self._src = None

    def group_channels(self, dtype):
        """channels per tap of the gathered operand: the image's padded channels (stem), else the stream's"""
        Ci = self.conv.weight.shape[1]
        return roundup(Ci, 8 if dtype == torch.bfloat16 else 4) if self.stem else roundup(Ci, 16)

    def ready(self, dtype, device):
        w = self.conv.weight
        Co, Ci, k = w.shape[0], w.shape[1], self.k
        Cg = self.group_channels(dtype)
        held = self.master
        if held is None or held.device != device or held.shape[1] != k * k * Cg:
            held = self.master = torch.zeros(Co, k * k * Cg, dtype=torch.float32, device=device)
            self._src = None
        src = (w._version, RT.weights_epoch, w.data_ptr())
        if src != self._src:
            held.view(Co, k, k, Cg)[..., :Ci].copy_(w.detach().permute(0, 2, 3, 1))
            self._src = src
        return super().ready(dtype, device)

    def param_grads(self, op, dc, xg):
        """weight and bias gradient on the chain (the permutation back follows the launch)"""
        w, Cg, k = self.conv.weight, self.master.shape[1] // (self.k * self.k), self.k
        gw = grad_of(w)
        if gw is not None:
            g = torch.zeros_like(self.master)
            op.wgrad(dc, xg, g)
            gw.add_(g.view(w.shape[0], k, k, Cg)[..., :w.shape[1]].permute(0, 3, 1, 2))
        gb = grad_of(self.conv.bias)
        if gb is not None:
            ops.bias_grad(dc, gb)


class _Block:
    def __init__(self, blk):
        self.m = blk
        dw = blk.dwconv
        self.C = dw.weight.shape[0]
        self.Cp = roundup(self.C, 16)
        self.pw1, self.pw2 = _LinearLayer(blk.pwconv1), _LinearLayer(blk.pwconv2)
        self.rate = float(getattr(blk.drop_path, "drop_prob", 0.))
        self._tab = self._tab_key = None

    def table(self, device):
        dw = self.m.dwconv
        key = (dw.weight._version, dw.bias._version, RT.weights_epoch, dw.weight.data_ptr(), device)
        if key != self._tab_key:
            self._tab, self._tab_key = ops.dwconv7_table(dw.weight, dw.bias, self.Cp), key
        return self._tab


def _slice(t, C):
    """the first C channels of a dense NHWC tensor (itself where it has no more)"""
    return t if t.shape[3] == C else t[..., :C]


def _dgrad_full(op, dy, H, W, Cfull):
    """data gradient into a dense tensor of Cfull >= Ci_p channels, the rest zero"""
    if op.Ci_p == Cfull:
        return op.dgrad(dy, H, W)
    buf = torch.zeros(dy.shape[0], H, W, Cfull, dtype=dy.dtype, device=dy.device)
    op.dgrad(dy, H, W, out=buf[..., :op.Ci_p])
    return buf


class ConvNeXtRunner:
    def __init__(self, module):
        self.m = module
        self.down = []
        for i, seq in enumerate(module.downsample_layers):
            conv, ln = (seq[0], seq[1]) if i == 0 else (seq[1], seq[0])
            self.down.append((_PatchLayer(conv, stem=(i == 0)), ln))
        self.stages = [[_Block(b) for b in stage] for stage in module.stages]
        if any(not s for s in self.stages):
            raise NotImplementedError("ConvNeXt on the HIP engine: every stage has at least one block")

    def stem_channels(self, dtype):
        return self.down[0][0].group_channels(dtype)

    # ------------------------------------------------------------------ forward
    def _block_fwd(self, b, X, train, want_copy):
        dt, dev = self.dtype, X.device
        m = b.m
        N, H, W, _ = X.shape
        tab, bias = b.table(dev)
        y1 = ops.dwconv7_fwd(X, tab, bias, b.C, dt)
        y2, mean, rstd = ops.layernorm_fwd(y1, m.norm.weight.data, m.norm.bias.data, m.norm.eps, dt)
        op1, op2 = b.pw1.ready(dt, dev), b.pw2.ready(dt, dev)
        h = op1.forward(_slice(y2, op1.Ci_p), bias=b.pw1.bias)
        act = ops.gelu_fwd(h)
        z = op2.forward(_slice(act, op2.Ci_p), bias=b.pw2.bias)
        keep = None
        if train and b.rate > 0.:
            dp = m.drop_path
            keep = (dp.keep_mask(N, torch.float32, dev, 4) / dp.keep_prob).view(N)
        gamma = m.gamma.data if m.gamma is not None else None
        out, copy = ops.scale_residual_fwd(X, z, gamma, keep, b.C, want_copy=want_copy)
        return dict(b=b, X=X, y1=y1, y2=y2, mean=mean, rstd=rstd, h=h, act=act, z=z, keep=keep), out, copy

    def forward(self, x, train):
        """x: NHWC image batch in the compute dtype -> ([one NHWC feature per out_index, compute dtype], ctx)"""
        dt = self.dtype = x.dtype
        dev = x.device
        outs = tuple(self.m.out_indices)
        ctx = dict(x=x, down=[], blocks=[], train=bool(train), dtype=dt)
        feats, S = [], None
        for i in range(max(outs) + 1):
            cl, ln = self.down[i]
            op = cl.ready(dt, dev)
            if i == 0:
                xg = ops.patch_gather(x, cl.k)
                c = op.forward(xg, bias=cl.bias)
                S, mean, rstd = ops.layernorm_fwd(c, ln.weight.data, ln.bias.data, ln.eps, dt, out_dtype=torch.float32)
                ctx["down"].append(dict(xg=xg, c=c, mean=mean, rstd=rstd))
            else:
                y, mean, rstd = ops.layernorm_fwd(S, ln.weight.data, ln.bias.data, ln.eps, dt)
                xg = ops.patch_gather(y, cl.k)
                ctx["down"].append(dict(xg=xg, S=S, mean=mean, rstd=rstd))
                S = op.forward(xg, bias=cl.bias, out_f32=True)
            recs = []
            blocks = self.stages[i]
            copy = None
            for j, b in enumerate(blocks):
                want = i in outs and j == len(blocks) - 1 and dt != torch.float32
                rec, S, copy = self._block_fwd(b, S, train, want)
                recs.append(rec)
            ctx["blocks"].append(recs)
            if i in outs:
                feats.append(S if dt == torch.float32 else copy)
        return feats, ctx

    # ------------------------------------------------------------------ backward
    def _block_bwd(self, r, dout):
        """dout: gradient w.r.t. the block's output (fp32, or the compute dtype) -> fp32 gradient w.r.t. its input"""
        b, dt = r["b"], self.dtype
        m = b.m
        N, H, W, _ = dout.shape
        dev = dout.device
        g_gamma = grad_of(m.gamma) if m.gamma is not None else None
        dz = ops.scale_residual_bwd(dout, r["z"], (m.gamma.data if m.gamma is not None else None), r["keep"], b.C, dt,
                                    dgamma=g_gamma, dbias=grad_of(m.pwconv2.bias), accumulate=True)
        op1, op2 = b.pw1.ready(dt, dev), b.pw2.ready(dt, dev)
        # (pwconv2's bias gradient came with dz, summed from the unrounded gradient)
        b.pw2.accumulate_param_grads(op2, dz, _slice(r["act"], op2.Ci_p), bias=False)
        da = _dgrad_full(op2, dz, H, W, r["h"].shape[3])
        dh = ops.gelu_bwd(r["h"], da)
        b.pw1.accumulate_param_grads(op1, dh, _slice(r["y2"], op1.Ci_p))
        dy2 = _dgrad_full(op1, dh, H, W, b.Cp)
        dy1 = ops.layernorm_bwd(dy2, r["y1"], m.norm.weight.data, r["mean"], r["rstd"], dt,
                                dgamma=grad_of(m.norm.weight), dbeta=grad_of(m.norm.bias), accumulate=True)
        gw, gb = grad_of(m.dwconv.weight), grad_of(m.dwconv.bias)
        if gw is not None or gb is not None:
            ops.dwconv7_bwd_weight(dy1, r["X"], b.C, dw=gw, dbias=gb, accumulate=True, want_weight=False, want_bias=False)
        tab, _ = b.table(dev)
        return ops.dwconv7_fwd(dy1, tab, None, b.C, dt, out_dtype=torch.float32, flip=True, addend=dout)

    def backward(self, ctx, gfeats):
        """gfeats: one dense NHWC gradient (compute dtype) or None per returned feature.  Accumulates parameter gradients;
        stages above the last feature that received a gradient are skipped (their parameters keep the gradient they had)."""
        dt = self.dtype = ctx["dtype"]
        dev = ctx["x"].device
        outs = tuple(self.m.out_indices)
        gstage = {i: g for i, g in zip(sorted(outs), gfeats) if g is not None}
        if not gstage:
            return
        last = max(gstage)
        d = gstage[last]
        for i in range(last, -1, -1):
            HO.issue_advanced(dev)
            for r in reversed(ctx["blocks"][i]):
                d = self._block_bwd(r, d)
            cl, ln = self.down[i]
            op = cl.ready(dt, dev)
            rec = ctx["down"][i]
            g_w, g_b = grad_of(ln.weight), grad_of(ln.bias)
            if i == 0:
                need_dc = any(p.requires_grad for p in (cl.conv.weight, cl.conv.bias))
                if not (need_dc or g_w is not None or g_b is not None):
                    break
                dc = ops.layernorm_bwd(d, rec["c"], ln.weight.data, rec["mean"], rec["rstd"], dt, dgamma=g_w, dbeta=g_b,
                                       accumulate=True, want_dx=need_dc)
                if need_dc:
                    cl.param_grads(op, dc, rec["xg"])
                break
            S = rec["S"]
            # the stream's gradient in the compute dtype: what the GEMM launches read
            dc = d if d.dtype == dt else ops.scale_residual_bwd(d, None, None, None, d.shape[3], dt)
            cl.param_grads(op, dc, rec["xg"])
            N, H, W, Cp = S.shape
            dg = op.dgrad(dc, H // cl.k, W // cl.k)
            dy = ops.patch_scatter(dg, H, W, cl.k)
            d = ops.layernorm_bwd(dy, S, ln.weight.data, rec["mean"], rec["rstd"], dt, addend=gstage.get(i - 1),
                                  dgamma=g_w, dbeta=g_b, accumulate=True)
        HO.flush_deferred(RT.current_stream())
        HO.chain_ends(dev)


def _as_nchw(mod, feats):
    """the real channels of each NHWC feature as a logical-NCHW view"""
    dims = [mod._runner.stages[i][0].C for i in sorted(mod.out_indices)]
    return [f[..., :c].permute(0, 3, 1, 2) for f, c in zip(feats, dims)]


def _padded(g):
    """dense NHWC gradient of a feature -> the stream's channel padding (zeros)"""
    C = g.shape[3]
    Cp = roundup(C, 16)
    if Cp == C:
        return g
    out = torch.zeros(g.shape[:3] + (Cp,), dtype=g.dtype, device=g.device)
    out[..., :C] = g
    return out


class _ConvNeXtFn(torch.autograd.Function):
    """one autograd node per call: the requested features out (logical NCHW views of the NHWC tensors)"""

    @staticmethod
    def forward(ctx, mod, x, *params):
        ctx.set_materialize_grads(False)
        feats, c = mod._runner.forward(x, train=True)
        ctx.mod, ctx.c, ctx.dtype = mod, c, x.dtype
        mod._pending += 1
        if RT.dp is not None:
            RT.dp.note_forward(mod)
        return tuple(_as_nchw(mod, feats))

    @staticmethod
    def backward(ctx, *g):
        from ..vision_base.networks.models.backbone.resnet import nhwc_dense
        mod = ctx.mod
        mod._runner.backward(ctx.c, [None if gi is None else _padded(nhwc_dense(gi, ctx.dtype)) for gi in g])
        ctx.c = None
        mod._pending -= 1
        if mod._pending == 0 and RT.dp is not None:
            RT.dp.grads_ready(mod)
        return (None, None) + (None,) * len(mod._plist)


def run_convnext(mod, img):
    """ConvNeXt.forward of a CUDA batch -> the features of out_indices as logical-NCHW views in the compute dtype"""
    require_gpu(img, "ConvNeXt.forward")
    if RT.dp is not None and RT.dp.world > 1:
        raise NotImplementedError("ConvNeXt on the HIP engine: data parallelism is not implemented; run it with world size 1")
    if torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("ConvNeXt on the HIP engine: a step that contains it is not captured into a hipGraph "
                                  "(BaseTrainingHook(use_graph=False))")
    if mod._runner is None or mod._runner.m is not mod:
        mod._runner = ConvNeXtRunner(mod)
    dt = RT.compute_dtype
    x = ops.nchw_to_nhwc(img.float(), None, mod._runner.stem_channels(dt), dt)
    if torch.is_grad_enabled() and mod.training and any(p.requires_grad for p in mod.parameters()):
        if mod._plist is None:
            mod._plist = list(mod.parameters())
        return list(_ConvNeXtFn.apply(mod, x, *mod._plist))
    with torch.no_grad():
        nhwc, _ = mod._runner.forward(x, train=mod.training)
    return _as_nchw(mod, nhwc)
