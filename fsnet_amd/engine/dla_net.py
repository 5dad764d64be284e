"""Manual forward / backward runner of the DLA backbone on the HIP library, in the manner of nets.ResNetRunner: every
convolution a ConvOp with its BatchNorm statistics in the epilogue, BatchNorm (+ residual, + ReLU) one fs_bn_apply, the
2x2 max pool and the roots' channel concatenation the launches of dla.hip.  The nn.Modules are parameter containers.

Reference structure followed (vision_base/networks/models/backbone/dla.py):
  blocks        :39-108      conv-bn-relu chains with a residual added before the last ReLU
  Root          :155-173     1x1 convolution over cat([x2, x1, *children]) (+ x2 with residual_root)
  Tree          :176-229     the recursion, its shared `children` list and the projection nobody reads (levels > 1)
  DLA.forward   :316-325     base layer, then all six levels

Where a root's sources live (the concatenation buffer `wide` of a root is allocated when the tree that owns its `children`
list is entered):
  x2            written into its slice by the BatchNorm pass that produces it — unless residual_root, where the root's
                BatchNorm pass reads it as a dense residual
  pooled input  (level_root) written into its slice by fs_pool2_fwd; the projection reads it there.  Dense instead
                where it is a block's residual (a level-root tree of one level without projection)
  x1, the x1 of every enclosing tree   each is the dense residual of the block that follows it: copied by fs_cat_fwd,
                all of a root's in one launch
Backwards the root's data gradient is one tensor over `wide`.  x2's BatchNorm backward and the pooling gradient read
their slices in place; a projection's data gradient takes the pooled input's slice as its addend.  Every x1 has three
gradient terms — its slice, the following block's first data gradient and that block's residual — of which a data
gradient launch sums two: fs_cat_bwd adds the slice when the other two exist, one launch per x1 (and one for x2 under
residual_root, whose second term is the root's masked gradient).
"""
import torch

from ..hip import ops
from ..hip.conv import LaunchProfile
from .handover import HO
from .nets import ConvLayer, StatsPool, _bn_bwd, bn_tensors, bwd_pool_reset
from .runtime import RT, grad_of, require_gpu


class _Unit:
    """one convolution and the BatchNorm behind it"""
    __slots__ = ("cl", "bn")

    def __init__(self, conv, bn, need_dgrad=True):
        if conv.groups != 1:
            raise NotImplementedError("DLA on the HIP engine: grouped convolution (groups=%d, the BottleneckX variants) "
                                      "has no kernel; those models construct and load, and run on the CPU" % conv.groups)
        if tuple(conv.dilation) != (1, 1) or conv.stride[0] != conv.stride[1] or conv.bias is not None:
            raise NotImplementedError("DLA on the HIP engine: dilation 1, square strides and no convolution bias")
        self.cl, self.bn = ConvLayer(conv, need_dgrad=need_dgrad), bn


class _Block:
    def __init__(self, blk):
        n = 3 if hasattr(blk, "conv3") else 2
        self.units = [_Unit(getattr(blk, "conv%d" % j), getattr(blk, "bn%d" % j)) for j in range(1, n + 1)]


class _Tree:
    def __init__(self, t):
        self.levels, self.level_root = t.levels, t.level_root
        self.pool = t.downsample is not None
        if self.pool and (t.downsample.kernel_size, t.downsample.stride) != (2, 2):
            raise NotImplementedError("DLA on the HIP engine: Tree.downsample is MaxPool2d(2, stride=2)")
        if self.level_root and not self.pool:
            raise NotImplementedError("DLA on the HIP engine: a level-root tree without downsample")
        self.project = _Unit(t.project[0], t.project[1]) if t.project is not None else None
        if t.levels == 1:
            self.tree1, self.tree2 = _Block(t.tree1), _Block(t.tree2)
            self.root = _Unit(t.root.conv, t.root.bn)
            if t.root.conv.kernel_size != (1, 1):
                raise NotImplementedError("DLA on the HIP engine: root_kernel_size 1")
            self.root_residual = bool(t.root.residual)
            self.root_dim = t.root.conv.in_channels
            self.out_channels = t.root.conv.out_channels
        else:
            self.tree1, self.tree2 = _Tree(t.tree1), _Tree(t.tree2)

    def final(self):
        """the one-level tree whose root reads the `children` list this tree starts"""
        t = self
        while t.levels > 1:
            t = t.tree2
        return t


class _Cat:
    """one root's concatenation buffer: x2 at channel 0, x1 behind it, then the children in the order they were appended"""

    def __init__(self, N, H, W, C, root_dim, dtype, device):
        self.wide = torch.empty(N, H, W, root_dim, dtype=dtype, device=device)
        self.next = 2 * C
        self.parts, self.offs, self.widths = [], [], []      # what fs_cat_fwd copies
        self.dwide = None

    def slot(self, C):
        off = self.next
        self.next += C
        assert self.next <= self.wide.shape[3]
        return off

    def view(self, off, C, grad=False):
        return (self.dwide if grad else self.wide)[..., off:off + C]

    def copy_in(self, t, off):
        self.parts.append(t); self.offs.append(off); self.widths.append(t.shape[3])

    def add_slice(self, off, into):
        """into += its slice of the root's data gradient (fs_cat_bwd)"""
        ops.cat_bwd(self.dwide, [into], [off], [into.shape[3]], accumulate=[True])
        return into


class DLARunner:
    def __init__(self, module):
        self.m = module
        # [feature index of the unit's output or None, _Unit, name]: base layer -> -1, the last unit of level0 / level1 -> 0 / 1
        self.chain = []
        for k, name in enumerate(("base_layer", "level0", "level1")):
            mods = list(getattr(module, name))
            for j in range(0, len(mods), 3):
                self.chain.append([None, _Unit(mods[j], mods[j + 1], need_dgrad=bool(self.chain)), name])
            self.chain[-1][0] = k - 1
        self.trees = [_Tree(getattr(module, "level%d" % i)) for i in range(2, 6)]
        self.pool = None
        self.marks = []           # (launch-profile record count, "fwd" | "bwd", level name) while LaunchProfile is active

    def _mark(self, phase, name):
        if LaunchProfile.active:
            self.marks.append((len(LaunchProfile.records), phase, name))

    # ------------------------------------------------------------------ forward
    def _unit_fwd(self, u, x, relu=True, res=None, out=None):
        """conv -> BatchNorm (+ res) (-> ReLU); out: the strided view that receives the activation.  -> record"""
        train = self.train
        op = u.cl.ready(x.dtype, x.device)
        bt = train and u.bn.training
        stats = self.pool.take(op.Co_p) if bt else None
        c = op.forward(x, stats=stats)
        N, Ho, Wo, _ = c.shape
        y = out if out is not None else torch.empty_like(c)
        st = ops.BnState(op.Co_p, x.device)
        count = N * Ho * Wo if (bt or not train) else float("inf")
        ops.bn_apply(c, stats, bn_tensors(u.bn), st, y, Ho, Wo, count, relu=relu, res=res, track=bt)
        return dict(u=u, x=x, c=c, y=y, st=st, relu=relu)

    def _block_fwd(self, b, x, residual, out=None):
        recs, cur = [], x
        for j, u in enumerate(b.units):
            last = j == len(b.units) - 1
            r = self._unit_fwd(u, cur, res=(residual if last else None), out=(out if last else None))
            recs.append(r)
            cur = r["y"]
        return dict(units=recs, res_is_x=residual is x), cur

    def _tree_fwd(self, t, x, cat=None):
        """-> (record, output).  cat: the enclosing tree's _Cat (this tree is its tree2), None: this tree starts one"""
        N, H, W, Cin = x.shape
        Ho, Wo = (H // 2, W // 2) if t.pool else (H, W)
        rec = dict(t=t, x=x, own=cat is None)
        if cat is None:
            f = t.final()
            cat = _Cat(N, Ho, Wo, f.out_channels, f.root_dim, x.dtype, x.device)
        rec["cat"] = cat
        bottom, rec["idx"] = x, None
        # the pooled input: a root source (level_root), a residual or the projection's input (one level), or — deeper trees —
        # nothing but the input of the projection whose result is dropped (its running statistics still move in training)
        dead = t.levels > 1 and t.project is not None
        if t.pool and (t.level_root or t.levels == 1 or (dead and self.train)):
            dense = not t.level_root or (t.levels == 1 and t.project is None)
            off = cat.slot(Cin) if t.level_root else None
            bottom, rec["idx"] = ops.pool2_fwd(x, out=(None if dense else cat.view(off, Cin)))
            if t.level_root and dense:
                cat.copy_in(bottom, off)
            rec["bottom_off"] = off
        rec["bottom"] = bottom
        residual, rec["proj"] = bottom, None
        if t.project is not None and (t.levels == 1 or self.train):
            rec["proj"] = self._unit_fwd(t.project, bottom, relu=False)
            residual = rec["proj"]["y"]
        if t.levels == 1:
            C = t.out_channels
            rec["b1"], x1 = self._block_fwd(t.tree1, x, residual)
            cat.copy_in(x1, C)
            rec["b2"], x2 = self._block_fwd(t.tree2, x1, x1, out=(None if t.root_residual else cat.view(0, C)))
            if t.root_residual:
                cat.copy_in(x2, 0)
            ops.cat_fwd(cat.wide, cat.parts, cat.offs, cat.widths)
            rec["root"] = self._unit_fwd(t.root, cat.wide, res=(x2 if t.root_residual else None))
            return rec, rec["root"]["y"]
        rec["t1"], x1 = self._tree_fwd(t.tree1, x)
        rec["x1_off"] = cat.slot(x1.shape[3])
        cat.copy_in(x1, rec["x1_off"])
        rec["t2"], y = self._tree_fwd(t.tree2, x1, cat)
        return rec, y

    def forward(self, x, train):
        """x: NHWC [N,H,W,Ci_p] in the compute dtype -> ([base, level0 .. level5] NHWC dense, ctx)"""
        dev = x.device
        if self.pool is None or self.pool.buf.device != dev:
            self.pool = StatsPool(dev)
        self.pool.reset()
        self.train = bool(train)
        ctx = dict(x=x, chain=[], trees=[], train=self.train)
        feats, cur = [], x
        for fi, u, name in self.chain:
            self._mark("fwd", name)
            r = self._unit_fwd(u, cur)
            ctx["chain"].append(r)
            cur = r["y"]
            if fi is not None:
                feats.append(cur)
        for i, t in enumerate(self.trees):
            self._mark("fwd", "level%d" % (i + 2))
            rec, cur = self._tree_fwd(t, cur)
            ctx["trees"].append(rec)
            feats.append(cur)
        self._mark("fwd", "end")
        return feats, ctx

    # ------------------------------------------------------------------ backward
    @staticmethod
    def _wgrad(u, dc, x):
        if grad_of(u.cl.m.weight) is not None:
            u.cl.accumulate_param_grads(u.cl.ready(dc.dtype, dc.device), dc, x)

    def _unit_bwd(self, r, dout, want_dx=True, addend=None, g_out=None):
        """dout: gradient w.r.t. the unit's output (any pixel strides).  -> gradient w.r.t. its input (+ addend)"""
        u, c = r["u"], r["c"]
        dc = _bn_bwd(dout, (r["y"] if r["relu"] else None), c, u.bn, r["st"], c.shape[1], c.shape[2], relu=r["relu"], g_out=g_out)
        self._wgrad(u, dc, r["x"])
        if not want_dx:
            return None
        x = r["x"]
        return u.cl.ready(dc.dtype, dc.device).dgrad(dc, x.shape[1], x.shape[2], addend=addend)

    def _block_bwd(self, brec, dout, extra=None):
        """-> (gradient w.r.t. the block's input, gradient w.r.t. its residual or None where the residual is the input).
        extra: one more dense term of the input's gradient"""
        recs = brec["units"]
        g = torch.empty_like(recs[-1]["c"])          # the ReLU-masked gradient: what the residual receives
        d = self._unit_bwd(recs[-1], dout, g_out=g)
        for r in recs[-2:0:-1]:
            d = self._unit_bwd(r, d)
        if brec["res_is_x"]:
            if extra is not None:
                raise NotImplementedError("DLA on the HIP engine: a feature gradient into a block whose residual is its input")
            return self._unit_bwd(recs[0], d, addend=g), None
        return self._unit_bwd(recs[0], d, addend=extra), g

    def _tree_bwd(self, rec, dout, extra=None):
        """dout: gradient w.r.t. the tree's output; extra: a dense term to add to the returned gradient w.r.t. its input
        (the feature gradient of the level below).  Gradients of what the tree appended to an enclosing `children` list
        stay in cat.dwide for the enclosing tree."""
        t, cat = rec["t"], rec["cat"]
        if t.levels == 1:
            C = t.out_channels
            root = rec["root"]
            g_root = torch.empty_like(root["c"]) if t.root_residual else None
            cat.dwide = self._unit_bwd(root, dout, g_out=g_root)
            d_x2 = cat.add_slice(0, g_root) if t.root_residual else cat.view(0, C, grad=True)
            d_x1, _ = self._block_bwd(rec["b2"], d_x2)
            cat.add_slice(C, d_x1)
            dx, g_res = self._block_bwd(rec["b1"], d_x1, extra=extra)
            if rec["b1"]["res_is_x"]:
                return dx
        else:
            d_x1 = self._tree_bwd(rec["t2"], dout)
            cat.add_slice(rec["x1_off"], d_x1)
            dx = self._tree_bwd(rec["t1"], d_x1, extra=extra)
            g_res = None
        # the pooled input's gradient: the residual path (through the projection) and, for a level root, its slice
        slice_ = cat.view(rec["bottom_off"], rec["x"].shape[3], grad=True) if t.level_root else None
        if g_res is not None and rec["proj"] is not None:
            if not t.pool:
                return self._unit_bwd(rec["proj"], g_res, addend=dx)
            d_bottom = self._unit_bwd(rec["proj"], g_res, addend=slice_)
        elif g_res is not None:
            d_bottom = cat.add_slice(rec["bottom_off"], g_res) if t.level_root else g_res
        else:
            d_bottom = slice_
        if d_bottom is None:
            return dx
        x = rec["x"]
        return ops.pool2_bwd(d_bottom, rec["idx"], x.shape[1], x.shape[2], addend=dx)

    def backward(self, ctx, gfeats):
        """gfeats: 7 dense NHWC gradients (or None) for [base, level0 .. level5].  Accumulates parameter gradients; levels
        above the last one that received a gradient are skipped (their parameters keep the gradient they had)."""
        dev = ctx["x"].device
        bwd_pool_reset(dev)
        self.train = ctx["train"]
        last = max((i for i, g in enumerate(gfeats) if g is not None), default=None)
        if last is None:
            return
        dout = gfeats[last]
        for i in range(last, 2, -1):            # feature i is level i - 1: trees are levels 2..5 = features 3..6
            self._mark("bwd", "level%d" % (i - 1))
            HO.issue_advanced(dev)
            dout = self._tree_bwd(ctx["trees"][i - 3], dout, extra=gfeats[i - 1])
        # the convolution chain: unit k's output is feature fi (or none); its input's gradient takes the feature gradient
        # of the unit below as the data gradient's addend
        nchain = len(self.chain)
        start = nchain - 1 if last >= 2 else max(k for k, e in enumerate(self.chain) if e[0] == last - 1)
        for k in range(start, -1, -1):
            self._mark("bwd", self.chain[k][2])
            below = self.chain[k - 1][0] if k > 0 else None
            dout = self._unit_bwd(ctx["chain"][k], dout, want_dx=k > 0,
                                  addend=(gfeats[below + 1] if below is not None else None))
        self._mark("bwd", "end")
        HO.flush_deferred(RT.current_stream())
        HO.chain_ends(dev)


class _DLAFn(torch.autograd.Function):
    """one autograd node per call: all seven features out (logical NCHW views of the NHWC tensors)"""

    @staticmethod
    def forward(ctx, mod, x, *params):
        ctx.set_materialize_grads(False)
        feats, c = mod._runner.forward(x, train=True)
        ctx.mod, ctx.c, ctx.dtype = mod, c, x.dtype
        mod._pending += 1
        if RT.dp is not None:
            RT.dp.note_forward(mod)
        return tuple(f.permute(0, 3, 1, 2) for f in feats)

    @staticmethod
    def backward(ctx, *g):
        from ..vision_base.networks.models.backbone.resnet import nhwc_dense
        mod = ctx.mod
        mod._runner.backward(ctx.c, [None if gi is None else nhwc_dense(gi, ctx.dtype) for gi in g])
        ctx.c = None
        mod._pending -= 1
        if mod._pending == 0 and RT.dp is not None:
            RT.dp.grads_ready(mod)
        return (None, None) + (None,) * len(mod._plist)


def run_dla(mod, img):
    """DLA.forward of a CUDA batch -> (base feature, [level0 .. level5]) as logical-NCHW views in the compute dtype"""
    require_gpu(img, "DLA.forward")
    if RT.dp is not None and RT.dp.world > 1:
        raise NotImplementedError("DLA on the HIP engine: data parallelism (the SyncBN exchange of its BatchNorms) is not "
                                  "implemented; run it with world size 1")
    if torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("DLA on the HIP engine: a step that contains it is not captured into a hipGraph "
                                  "(BaseTrainingHook(use_graph=False))")
    if mod._runner is None or mod._runner.m is not mod:
        mod._runner = DLARunner(mod)
    op = mod._runner.chain[0][1].cl.ready(RT.compute_dtype, img.device)
    x = ops.nchw_to_nhwc(img.float(), None, op.Ci_p, RT.compute_dtype)
    if torch.is_grad_enabled() and mod.training and any(p.requires_grad for p in mod.parameters()):
        if mod._plist is None:
            mod._plist = list(mod.parameters())
        feats = list(_DLAFn.apply(mod, x, *mod._plist))
    else:
        with torch.no_grad():
            nhwc, _ = mod._runner.forward(x, train=mod.training)
        feats = [f.permute(0, 3, 1, 2) for f in nhwc]
    return feats[0], feats[1:]
