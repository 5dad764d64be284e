"""ManyDepth-style multi-frame depth encoder with the reference's constructor, attributes and state_dict
(reference monodepth/networks/models/backbone/resnet_matching.py:8-268), executed by the HIP engine.

forward = stem + layer1 on the current image (one EncoderPass that stops after stage 0), the same on the B*F lookup
images as one batch without gradient, the plane-sweep cost volume in one launch (ops.cost_volume: the warped features
never reach memory and nothing waits for the host), reduce_conv over [current features | cost volume], then layer2-4
as a pass that is entered after the stem.  Autograd sees one custom Function per call.

match_features on CPU tensors runs `match_features_host`, the same arithmetic in plain torch ops vectorised over
the batch and the lookup frames (also the baseline of tools/bench_cost_volume.py)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from fsnet_amd.engine.nets import ConvLayer, ResNetRunner
from fsnet_amd.engine.runtime import RT, require_gpu
from fsnet_amd.hip import ops
from fsnet_amd.vision_base.networks.models.backbone.resnet import nhwc_dense, resnet


def intrinsics_4x4(P2):
    """K [B,4,4] f64 with K[:, :3, :3] = P2[:, :3, :3] as given (not rescaled to the matching resolution) and its
    np.linalg.pinv, both on the host (resnet_matching.py:98-101)."""
    P2 = P2.detach().cpu().numpy() if isinstance(P2, torch.Tensor) else np.asarray(P2)
    K = np.zeros([P2.shape[0], 4, 4])
    K[:, 0:3, 0:3] = P2[:, 0:3, 0:3]
    K[:, 3, 3] = 1
    return K, np.linalg.pinv(K)


def match_features_host(current_feats, lookup_feats, relative_poses, K, inv_K, depth_bins, dtype=torch.float32):
    """The reference's match_features (resnet_matching.py:83-173) as plain torch ops on the tensors' device, vectorised
    over the batch and the lookup frames: no Python loop over the batch, no test on the host.
    current_feats [B,C,h,w], lookup_feats [B,F,C,h,w], relative_poses [B,F,4,4], K / inv_K [B,4,4], depth_bins [D]
    -> (cost volume with the missing bins filled [B,D,h,w], missing mask [B,D,h,w]) in `dtype` (fp32; the golden tool
    also evaluates it in f64 from f64 intrinsics)."""
    B, C, h, w = current_feats.shape
    Fn, D = lookup_feats.shape[1], depth_bins.numel()
    dev = current_feats.device
    cur = current_feats.to(dtype)
    K, inv_K = K.to(dtype), inv_K.to(dtype)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=dev),
                            torch.arange(w, dtype=dtype, device=dev), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, dtype=dtype, device=dev)], 0)
    cam = torch.matmul(inv_K[:, :3, :3], pix)                                   # [B,3,hw]
    pts = depth_bins.to(dtype).view(1, D, 1, 1) * cam[:, None]                    # [B,D,3,hw]
    pts = torch.cat([pts, torch.ones(B, D, 1, h * w, dtype=dtype, device=dev)], 2)
    P = torch.matmul(K[:, None], relative_poses.to(dtype))[:, :, :3, :]           # [B,F,3,4]
    cp = torch.matmul(P[:, :, None], pts[:, None])                              # [B,F,D,3,hw]
    pc = cp[:, :, :, :2] / (cp[:, :, :, 2:3] + 1e-7)
    gx = (pc[:, :, :, 0] / (w - 1) - 0.5) * 2
    gy = (pc[:, :, :, 1] / (h - 1) - 0.5) * 2
    grid = torch.stack([gx, gy], -1).view(B * Fn, D * h, w, 2)                  # the D bins stacked along the height
    warped = F.grid_sample(lookup_feats.reshape(B * Fn, C, h, w).to(dtype), grid, padding_mode="zeros", mode="bilinear",
                           align_corners=True).view(B, Fn, C, D, h, w)
    x_vals = ((gx / 2 + 0.5) * (w - 1)).view(B, Fn, D, h, w)
    y_vals = ((gy / 2 + 0.5) * (h - 1)).view(B, Fn, D, h, w)
    edge = ((x_vals >= 2.0) & (x_vals <= w - 2) & (y_vals >= 2.0) & (y_vals <= h - 2)).to(dtype)
    current_mask = torch.zeros(h, w, dtype=dtype, device=dev)
    current_mask[2:-2, 2:-2] = 1.0
    present = (relative_poses.to(dtype).reshape(B, Fn, 16).sum(-1) != 0).to(dtype).view(B, Fn, 1, 1, 1)
    diffs = torch.abs(warped - cur[:, None, :, None]).mean(2) * (edge * current_mask) * present
    cost = torch.zeros(B, D, h, w, dtype=dtype, device=dev)
    counts = torch.zeros_like(cost)
    for f in range(Fn):                      # (frame order kept: the sums are the reference's)
        cost = cost + diffs[:, f]
        counts = counts + (diffs[:, f] > 0).to(dtype)
    cost = cost / (counts + 1e-7)
    missing = (cost == 0).to(dtype)
    cost = cost * (1 - missing) + cost.max(1)[0].unsqueeze(1) * missing
    return cost, missing


class _MatchingFn(torch.autograd.Function):
    """features[0..4], lowest_cost, confidence of one call; backward: layer4-2, reduce_conv, layer1 + stem."""

    @staticmethod
    def forward(ctx, mod, x, xl, K, inv_K, poses, *params):
        ctx.set_materialize_grads(False)
        feats, lowest, conf, c = mod._execute(x, xl, K, inv_K, poses, train=True)
        ctx.mod, ctx.c, ctx.dtype = mod, c, x.dtype
        ctx.mark_non_differentiable(lowest, conf)
        return tuple(f.permute(0, 3, 1, 2) for f in feats) + (lowest, conf)

    @staticmethod
    def backward(ctx, *g):
        mod = ctx.mod
        gf = [None if gi is None else nhwc_dense(gi, ctx.dtype) for gi in g[:5]]
        mod._backward(ctx.c, gf)
        ctx.c = None
        return (None,) * (6 + len(mod._plist))


class ResnetEncoderMatching(nn.Module):
    """ResNet encoder with a plane-sweep matching cost volume between layer1 and layer2 (constructor signature,
    attributes and state_dict of the reference class).  adaptive_bins=True: forward() recomputes the depth bins from its
    min_depth_bin / max_depth_bin arguments on every call, for training whose scale is not known in advance."""

    BINNINGS = ("linear", "inverse")

    def __init__(self, depth, pretrained, input_height, input_width,
                 min_depth_bin=0.1, max_depth_bin=20.0, num_depth_bins=96,
                 adaptive_bins=False, depth_binning='linear', **kwargs):
        super().__init__()
        self.adaptive_bins, self.depth_binning = adaptive_bins, depth_binning
        self.set_missing_to_max = True           # (the reference's switch; the kernel implements the True branch)
        self.num_depth_bins = num_depth_bins
        self.matching_height, self.matching_width = input_height // 4, input_width // 4     # layer1's resolution
        self.is_cuda = False
        self.depth_bins = self.warp_depths = None
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        if depth > 34:                           # Bottleneck stages are four times as wide
            self.num_ch_enc[1:] *= 4

        # The ResNet itself stays an unregistered attribute, as in the reference: its layers are registered here under
        # the names layer0 (conv, BatchNorm, ReLU), layer1 (max-pool, stage 1), layer2-4, which fixes the state_dict
        # keys and keeps the ResNet's own train() override out of reach of this module's train().
        encoder = resnet(depth, pretrained=pretrained, **kwargs)
        if encoder.num_stages != 4:
            raise NotImplementedError("ResnetEncoderMatching runs a four-stage ResNet")
        self.__dict__["_encoder"] = encoder
        self.layer0 = nn.Sequential(encoder.conv1, encoder.bn1, encoder.relu)
        self.layer1 = nn.Sequential(encoder.maxpool, encoder.layer1)
        self.layer2, self.layer3, self.layer4 = encoder.layer2, encoder.layer3, encoder.layer4
        self.compute_depth_bins(min_depth_bin, max_depth_bin)
        width = int(self.num_ch_enc[1])
        # registration order = state_dict order: prematching_conv (never called) before reduce_conv
        self.prematching_conv = nn.Sequential(nn.Conv2d(64, 16, kernel_size=1), nn.ReLU(inplace=True))
        self.reduce_conv = nn.Sequential(nn.Conv2d(width + num_depth_bins, width, kernel_size=3, padding=1),
                                         nn.ReLU(inplace=True))

        self._head = ResNetRunner(encoder, 0, 1)        # stem + layer1
        self._tail = ResNetRunner(encoder, 1, 4)        # layer2-4, entered with reduce_conv's output
        self._reduce = ConvLayer(self.reduce_conv[0])
        self._plist = None

    # ---------------------------------------------------------------- bins
    def compute_depth_bins(self, min_depth_bin, max_depth_bin):
        """num_depth_bins hypothesised depths in increasing order, evenly spaced in depth ('linear') or in inverse depth
        ('inverse'), computed in f64 and stored as fp32.  An existing tensor of the same length is overwritten in place
        (it may live on the device, and a captured graph keeps reading it)."""
        if self.depth_binning not in self.BINNINGS:
            raise NotImplementedError
        lo, hi, n = float(min_depth_bin), float(max_depth_bin), self.num_depth_bins
        if self.depth_binning == "linear":
            bins = np.linspace(lo, hi, n)
        else:
            bins = (1 / np.linspace(1 / hi, 1 / lo, n)[::-1])
        bins = torch.from_numpy(np.ascontiguousarray(bins)).float()
        if self.depth_bins is not None and self.depth_bins.shape == bins.shape:
            self.depth_bins.copy_(bins)
        else:
            self.depth_bins = bins
        self._expand_warp_depths()

    def _expand_warp_depths(self):
        # [D,1,h,w] like the reference's attribute, as a view: nothing of that size is stored
        self.warp_depths = self.depth_bins.view(-1, 1, 1, 1).expand(-1, 1, self.matching_height, self.matching_width)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.depth_bins is not None:
            self.depth_bins = fn(self.depth_bins)
            self._expand_warp_depths()
            self.is_cuda = self.depth_bins.is_cuda
        return self

    # ---------------------------------------------------------------- matching
    def match_features(self, current_feats, lookup_feats, relative_poses, P2):
        """L1 matching cost between the current features and the lookup features warped to every depth bin.

        current_feats [B,C,h,w], lookup_feats [B,F,C,h,w], relative_poses [B,F,4,4], P2 [B,3,4] (its [:3,:3] is used
        as given).  A lookup frame whose pose sums to 0 is skipped.  Returns (cost volume with the missing bins set to
        the pixel's maximum, missing mask), both [B,D,h,w] fp32.  Tensors on the GPU run the HIP kernel, CPU tensors the
        host form."""
        K, inv_K = intrinsics_4x4(P2)
        dev = current_feats.device
        K = torch.from_numpy(K).float().to(dev)
        inv_K = torch.from_numpy(inv_K).float().to(dev)
        bins = self.depth_bins.to(dev)
        if dev.type != "cuda":
            return match_features_host(current_feats, lookup_feats, relative_poses.to(dev), K, inv_K, bins)
        B, C, h, w = current_feats.shape
        Fn = lookup_feats.shape[1]
        dt = current_feats.dtype if current_feats.dtype in (torch.float32, torch.bfloat16) else torch.float32
        cur = nhwc_dense(current_feats.detach(), dt)
        look = nhwc_dense(lookup_feats.detach().reshape(B * Fn, C, h, w), dt)
        D = self.num_depth_bins
        eg = 16 // cur.element_size()
        cat = torch.empty(B, h, w, (C + D + eg - 1) // eg * eg, dtype=dt, device=dev)
        _, _, vol, missing = ops.cost_volume(cur, look, K, inv_K, relative_poses.detach().float().contiguous(), bins,
                                             cat, want_volume=True)
        return vol, missing

    def feature_extraction(self, image, return_all_feats=False):
        """normalised image -> layer1's features (return_all_feats: [stem activation, layer1's features]).  Called on its
        own it carries no gradient: forward() is the differentiable path."""
        require_gpu(image, "ResnetEncoderMatching.feature_extraction")
        x = self._to_nhwc(image)
        with torch.no_grad():
            feats, _ = self._head.forward(x, train=self.layer0[1].training)
        feats = [f.permute(0, 3, 1, 2) for f in feats]
        return feats if return_all_feats else feats[-1]

    def indices_to_disparity(self, indices):
        """bin indices [B,h,w] -> 1 / depth of the bin"""
        return 1 / self.depth_bins[indices.to(self.depth_bins.device)]

    def compute_confidence_mask(self, cost_volume, num_bins_threshold=None):
        """1.0 where the number of bins with a positive cost equals num_bins_threshold (default: all of them)"""
        need = self.num_depth_bins if num_bins_threshold is None else num_bins_threshold
        return ((cost_volume > 0).sum(1) == need).float()

    # ---------------------------------------------------------------- execution
    def _to_nhwc(self, image):
        image = (image.float() - 0.45) / 0.225
        op = self._head.stem.ready(RT.compute_dtype, image.device)
        return ops.nchw_to_nhwc(image, None, op.Ci_p, RT.compute_dtype)

    def _execute(self, x, xl, K, inv_K, poses, train):
        """x [B,H,W,Cp], xl [B*F,H,W,Cp] NHWC in the compute dtype -> (5 NHWC features, lowest_cost, confidence, ctx)"""
        feats_h, ctx_h = self._head.forward(x, train=train)
        f1 = feats_h[1]
        # lookup images: no gradient; one BatchNorm statistics group of B*F images, after the current pass
        look, _ = self._head.forward(xl, train=train)
        B, h, w, C = f1.shape
        op = self._reduce.ready(f1.dtype, f1.device)
        cat = torch.empty(B, h, w, op.Ci_p, dtype=f1.dtype, device=f1.device)
        cat[..., :C].copy_(f1)
        conf, lowest = ops.cost_volume(f1, look[1], K, inv_K, poses, self.depth_bins, cat)
        y = op.forward(cat, bias=self._reduce.bias, relu=True)
        feats_t, ctx_t = self._tail.forward(y, train=train)
        return list(feats_h) + list(feats_t), lowest, conf, dict(head=ctx_h, tail=ctx_t, cat=cat, y=y, f1=f1)

    def _backward(self, c, gf):
        y, cat, f1 = c["y"], c["cat"], c["f1"]
        # layer4-2; the returned gradient is masked by reduce_conv's ReLU
        dy = self._tail.backward(c["tail"], gf[2:5], in_mask=y)
        op = self._reduce.ready(y.dtype, y.device)
        self._reduce.accumulate_param_grads(op, dy, cat)
        # only the first C channels of reduce_conv's data gradient exist: the cost volume carries no gradient.  The
        # decoder's skip gradient on features[1] is the addend.
        g1 = op.dgrad(dy, f1.shape[1], f1.shape[2], out=torch.empty_like(f1), addend=gf[1])
        self._head.backward(c["head"], [gf[0], g1])

    def forward(self, current_image, lookup_images, poses, P2,
                min_depth_bin=None, max_depth_bin=None
                ):
        require_gpu(current_image, "ResnetEncoderMatching.forward")
        dev = current_image.device
        if self.depth_bins.device != dev:
            raise RuntimeError("ResnetEncoderMatching: move the module to %s first" % dev)
        if self.adaptive_bins:
            self.compute_depth_bins(min_depth_bin, max_depth_bin)
        batch_size, num_frames, chns, height, width = lookup_images.shape
        K, inv_K = intrinsics_4x4(P2)
        K = torch.from_numpy(K).float().to(dev)
        inv_K = torch.from_numpy(inv_K).float().to(dev)
        poses = poses.detach().to(dev, torch.float32).contiguous()
        x = self._to_nhwc(current_image)
        xl = self._to_nhwc(lookup_images.reshape(batch_size * num_frames, chns, height, width))
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters()):
            if self._plist is None:
                self._plist = list(self.parameters())
            outs = _MatchingFn.apply(self, x, xl, K, inv_K, poses, *self._plist)
            self.features = list(outs[:5])
            return self.features, outs[5], outs[6]
        with torch.no_grad():
            feats, lowest, conf, _ = self._execute(x, xl, K, inv_K, poses, train=self.layer0[1].training)
        self.features = [f.permute(0, 3, 1, 2) for f in feats]
        return self.features, lowest, conf
