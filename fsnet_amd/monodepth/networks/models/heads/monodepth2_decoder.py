"""MonoDepth2Decoder with the reference's constructor and method names
(monodepth/networks/models/heads/monodepth2_decoder.py:19-347).  loss() runs the fused HIP
photometric chain (backproject -> project -> grid_sample -> SSIM+L1 -> per-pixel min -> masked mean,
plus edge-aware smoothness), forward and backward, for the option set the shipped configs use;
every other option raises instead of silently taking a different path."""
import torch
import torch.nn as nn

from fsnet_amd.engine.runtime import RT, require_gpu
from fsnet_amd.hip import ops
from fsnet_amd.vision_base.utils.builder import build

_UNSUPPORTED_FLAGS = ("is_residual_flow", "is_light_compensate", "learnable_photometric_uncertain", "is_ssim_weight")


class _PhotoLossFn(torch.autograd.Function):
    """(pl, S, N, img0, P2, patched_mask, motion_mask, src_1..N, T_1..N, depths, disps); the gradient of the transforms
    comes back per frame"""

    @staticmethod
    def forward(ctx, pl, S, N, img0, P2, patched_mask, motion_mask, *rest):
        ctx.set_materialize_grads(False)
        srcs = [t.contiguous().float() for t in rest[:N]]
        Ts = [t.contiguous().float() for t in rest[N:2 * N]]
        dd = rest[2 * N:]
        depths = [d.contiguous().float() for d in dd[:S]]
        disps = [d.contiguous().float() for d in dd[S:]]
        seed = None if RT.tie_noise else -1     # None: device-resident seed, bumped in-stream every step
        RT.mark("photo.fwd.start")
        out = pl.forward(img0.contiguous().float(), srcs, P2.contiguous().float(), Ts, patched_mask, depths, disps,
                         noise_seed=seed, motion_mask=None if motion_mask is None else motion_mask.contiguous().float())
        ctx.pl, ctx.S, ctx.N = pl, S, N
        ctx.mark_non_differentiable(out)    # fresh tensors of this call (ops.PhotometricLoss.forward): no copies
        return pl.total, out

    @staticmethod
    def backward(ctx, g_total, _g_vec):
        pl, N = ctx.pl, ctx.N
        gout = None
        if g_total is not None:
            gout = g_total.detach().double().contiguous()
        RT.mark("photo.bwd.start")
        d_depth, d_disp, dT = pl.backward(gout)
        RT.mark("photo.bwd.end")
        return (None,) * 7 + (None,) * N + tuple(dT) + tuple(d_depth) + tuple(d_disp)


class _DistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, teacher, unc):
        pred, teacher = pred.contiguous().float(), teacher.contiguous().float()
        unc = None if unc is None else unc.contiguous().float()
        ctx.save_for_backward(pred, teacher, unc)
        return ops.distill_fwd(pred, teacher, unc)

    @staticmethod
    def backward(ctx, g):
        pred, teacher, unc = ctx.saved_tensors
        d_pred, d_unc = ops.distill_bwd(pred, teacher, unc, g.detach().double().contiguous())
        return d_pred, None, d_unc


class _DistillUnscaledFn(torch.autograd.Function):
    """(S, with_unc, pred_1..S, teacher_1..S[, uncertain_1..S]) -> S scalar losses of is_unscaled_distill, every scale in
    one set of launches; the gradient flows through each plane's ratio as well"""

    @staticmethod
    def forward(ctx, S, with_unc, *rest):
        preds = [t.contiguous().float() for t in rest[:S]]
        teachers = [t.contiguous().float() for t in rest[S:2 * S]]
        uncs = [t.contiguous().float() for t in rest[2 * S:3 * S]] if with_unc else None
        losses, ctx.du = ops.distill_unscaled_fwd(preds, teachers, uncs)
        ctx.S, ctx.with_unc = S, with_unc
        return tuple(losses.unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        gouts = torch.stack([g.detach().double() for g in gs])
        d_pred, d_unc = ops.distill_unscaled_bwd(ctx.du, gouts)
        return (None, None) + tuple(d_pred) + (None,) * ctx.S + (tuple(d_unc) if ctx.with_unc else ())


class MonoDepth2Decoder(nn.Module):
    def __init__(self, scales, height, width, frame_ids, depth_decoder_cfg, pose_decoder_cfg=None,
                 multiscale_head_cfg=None, **kwargs):
        super().__init__()
        self.scales = list(scales)
        self.num_scales = len(self.scales)
        self.height, self.width = height, width
        self.frame_ids = list(frame_ids)
        self.depth_decoder = build(**depth_decoder_cfg)
        if pose_decoder_cfg is not None:
            self.pose_decoder = build(**pose_decoder_cfg)
        if multiscale_head_cfg is not None:
            raise NotImplementedError("multiscale_head_cfg (residual flow head) is outside the monodepth hot path")
        for key in kwargs:           # min_depth, max_depth, overlapped_mask, is_log_image, ... (reference :48-49)
            setattr(self, key, kwargs[key])
        self._pl = None

    # ---- network heads -------------------------------------------------------------------
    def forward_pose(self, *args, **kwargs):
        return self.pose_decoder(*args, **kwargs)

    def forward_pose_transform(self, features, invert):
        """fused (axisangle, translation, cam_T_cam): pose_decoder.py:26-45 + monodepth2_model.py:42-43."""
        return self.pose_decoder.forward_with_transform(features, invert)

    def forward_pose_pairs(self, features, inverts):
        """all image pairs of the step in one pass over the stacked pose-encoder feature"""
        return self.pose_decoder.forward_pairs_with_transform(features, inverts)

    def forward_depth(self, features, *args, **kwargs):
        return self.depth_decoder(features, *args, **kwargs)

    def get_prediction(self, input_dict, output_dict):
        return dict(depth=output_dict[("depth", 0, 0)])

    # ---- loss ---------------------------------------------------------------------------------
    def _check_options(self, input_dict):
        for flag in _UNSUPPORTED_FLAGS:
            if getattr(self, flag, False):
                raise NotImplementedError("MonoDepth2Decoder option %s is not implemented in the HIP loss chain" % flag)
        if getattr(self, "residualflow_weight", 0) > 0:
            raise NotImplementedError("MonoDepth2Decoder term residualflow_weight > 0 is not implemented in the HIP loss chain")
        self._check_frame_ids()

    MAX_SOURCES = 4

    def _check_frame_ids(self):
        """frame_ids = [0, a, ...]: the target and one to four distinct temporal source frames"""
        ids = self.frame_ids
        if "s" in ids:
            raise NotImplementedError("frame_ids %r: the stereo frame 's' is not implemented in the HIP loss chain "
                                      "(temporal source frames only)" % (ids,))
        if len(ids) < 2 or ids[0] != 0 or not all(isinstance(f, int) and not isinstance(f, bool) for f in ids):
            raise NotImplementedError("frame_ids %r: expected [0, a, ...] with integer frame offsets, the target 0 "
                                      "first and at least one source frame" % (ids,))
        if 0 in ids[1:]:
            raise NotImplementedError("frame_ids %r: a source frame must differ from the target (no 0 after the "
                                      "first entry)" % (ids,))
        if len(set(ids)) != len(ids):
            raise NotImplementedError("frame_ids %r: every source frame may appear once (duplicates)" % (ids,))
        if len(ids) - 1 > self.MAX_SOURCES:
            raise NotImplementedError("frame_ids %r: the HIP loss chain takes at most %d source frames, got %d"
                                      % (ids, self.MAX_SOURCES, len(ids) - 1))

    def _loss_engine(self, img0):
        B, _, H, W = img0.shape
        return self._loss_engine_for(B, H, W, img0.device)

    def _loss_engine_for(self, B, H, W, device):
        key = (B, H, W, tuple(self.scales), device)
        if self._pl is None or self._pl_key != key:
            # the warped images only reach HBM when somebody looks at them (logging; output_dict entries below)
            kw = dict(want_pred=bool(getattr(self, "is_log_image", True) or getattr(self, "keep_warped_images", False)),
                      overlapped_mask=bool(getattr(self, "overlapped_mask", False)))
            # (frame_ids = [0, a, b] runs the two-source kernels, every other count the N-frame ones)
            self._pl = ops.PhotometricLoss(B, H, W, self.scales, device, self.min_depth, self.max_depth,
                                           nsrc=len(self.frame_ids) - 1, **kw)
            self._pl_key = key
        return self._pl

    def _stage_geometry(self, input_dict):
        """camera-model inputs of the loss engine beyond P2 (none for the pinhole model)"""
        self._pl.fisheye = False

    def stage_step_inputs(self, input_dict):
        """host-side per-step staging the training hook runs before replaying a captured step (non-tensor inputs)"""
        return

    @staticmethod
    def _mask64(input_dict):
        pm = input_dict.get("patched_mask", None)
        if pm is not None and pm.dtype != torch.float64:
            pm = pm.double()
        return pm.contiguous() if pm is not None else None

    def prefetch_loss_inputs(self, input_dict):
        """launch the input-only part of the loss chain (identity reprojection, colour pyramid) on the current
        stream — the meta-arch calls this on the pose stream, off the depth chain's critical path"""
        try:
            self._check_frame_ids()
        except NotImplementedError:
            return                    # loss() raises it
        img0 = input_dict[("original_image", 0)]
        if not (img0.is_cuda and img0.dtype == torch.float32 and img0.is_contiguous()):
            return
        srcs = [input_dict[("original_image", f)] for f in self.frame_ids[1:]]
        if not all(s.dtype == torch.float32 and s.is_contiguous() for s in srcs):
            return
        pm = input_dict.get("patched_mask", None)
        if pm is not None and not (pm.dtype == torch.float64 and pm.is_contiguous()):
            return                    # a converted copy would not be the tensor loss() sees
        self._loss_engine(img0).prefetch(img0, srcs, pm)

    def compute_total_reprojection_loss(self, output_dict, input_dict):
        self._check_options(input_dict)
        img0 = input_dict[("original_image", 0)]
        require_gpu(img0, "MonoDepth2Decoder.loss")
        B, _, H, W = img0.shape
        S = self.num_scales
        for s in self.scales:
            d = output_dict[("depth", s, s)]
            if d.shape[2] != (H >> s) or d.shape[3] != (W >> s):
                raise NotImplementedError("depth at scale %d must be %dx%d" % (s, H >> s, W >> s))
        self._loss_engine(img0)
        self._stage_geometry(input_dict)
        sources = self.frame_ids[1:]
        N = len(sources)
        pm = self._mask64(input_dict)
        depths = [output_dict[("depth", s, s)] for s in self.scales]
        disps = [output_dict[("disp", s)] for s in self.scales]
        Ts = [output_dict[("cam_T_cam", f)] for f in sources]
        # (what the loss differentiates: the training hook's per-chain capture cuts the backward here)
        self._loss_inputs = (Ts, depths + disps)
        total, vec = _PhotoLossFn.apply(self._pl, S, N, img0, input_dict["P2"], pm, input_dict.get("motion_mask", None),
                                        *[input_dict[("original_image", f)] for f in sources], *Ts, *depths, *disps)
        losses = {}
        for k, s in enumerate(self.scales):
            losses["loss/%d" % s] = vec[k]
            losses["smooth_loss/%d" % s] = vec[S + k]
        # warped images / masks the reference leaves in output_dict (_generate_images_pred :98-116).  The fused loss
        # kernels keep them in registers: they are written out when is_log_image (the reference default) or
        # keep_warped_images=True asks for them
        if self._pl.pred is not None:
            for k, s in enumerate(self.scales):
                for j, f in enumerate(sources):
                    output_dict[("original_image", f, s)] = self._pl.pred[k, j]
                    if self._pl.overlapped_mask:      # (the reference only produces it when the option is on)
                        output_dict[("overlapped_mask", f, s)] = self._pl.ov[k, j].view(torch.bool)   # 0/1 bytes
        hm = {}
        if getattr(self, "is_log_image", True) and self._pl.pred is not None:
            hm["original_image"] = img0[0:1]
            for j, f in enumerate(sources):
                hm["predicted_image_%s" % f] = self._pl.pred[0, j, 0:1]
            # the reference's literal `idxs >= 2` on its concatenated index (identity 0..N-1, reprojection N..2N-1),
            # whatever N is: with N = 1 it is never true for a reprojection winner, with N >= 3 it is true for identity
            # index 2 — the reference's quirk, mirrored.  Its index has no entry for "selected reprojection term whose
            # sample missed" (2N here): there the constant 100 stands in that term's own slot, >= N
            hm["loss_mask_%d" % self.scales[0]] = dict(data=self._loss_mask(self._pl.sel[0, 0:1], N).unsqueeze(1))
        return losses, hm, total

    @staticmethod
    def _loss_mask(sel, N):
        # sel == 2N stands for a reprojection index in N..2N-1: >= 2 exactly when N >= 2 (N = 1: indices 0 and 1 only)
        return (sel >= 2) if N >= 2 else torch.zeros_like(sel, dtype=torch.bool)

    def compute_pose_loss(self, output_dict, input_dict):
        """sum over the source frames of mean |relative_pose - cam_T_cam| (reference :176-183): the mean-absolute-difference
        kernel of the distillation term on the 4x4 matrices; its gradient reaches the pose networks through cam_T_cam"""
        pose_loss = 0
        for f in self.frame_ids[1:]:
            target = input_dict[('relative_pose', f)].detach()
            pose_loss = pose_loss + _DistillFn.apply(output_dict[("cam_T_cam", f)], target, None)
        return pose_loss

    def compute_distill_loss(self, output_dict, input_dict, scale):
        """monodepth2_decoder.py:185-203: mean |teacher - pred| (/ uncertain_z + log(uncertain_z + 1e-5)); with
        is_unscaled_distill the teacher is first scaled by each sample's mean of pred / (teacher + 1e-5)"""
        if getattr(self, 'is_unscaled_distill', False):
            return self._distill_unscaled(output_dict, [scale])[0]
        pred = output_dict[('depth', scale, scale)]
        teacher = output_dict[('teacher_depth', scale, scale)].detach()
        unc = output_dict[('uncertain_z', scale)] if getattr(self, 'is_uncertain_distill', False) else None
        return _DistillFn.apply(pred, teacher, unc)

    def _distill_unscaled(self, output_dict, scales):
        """the is_unscaled_distill term of every scale in `scales` from one set of launches"""
        with_unc = bool(getattr(self, 'is_uncertain_distill', False))
        preds = [output_dict[('depth', s, s)] for s in scales]
        teachers = [output_dict[('teacher_depth', s, s)].detach() for s in scales]
        uncs = [output_dict[('uncertain_z', s)] for s in scales] if with_unc else []
        return _DistillUnscaledFn.apply(len(scales), with_unc, *preds, *teachers, *uncs)

    def loss(self, output_dict, input_dict):
        losses, hm, total = self.compute_total_reprojection_loss(output_dict, input_dict)
        pose_weight = getattr(self, 'pose_loss_weight', 0)
        if pose_weight > 0:                                           # reference :176-183, 322-326
            pose_loss = self.compute_pose_loss(output_dict, input_dict)
            losses['pose_loss'] = pose_loss.detach()
            total = total + pose_weight * pose_loss
        distillation_weight = getattr(self, 'distillation_loss_weight', 0)
        if distillation_weight > 0:                                   # reference :328-334
            if getattr(self, 'is_unscaled_distill', False):
                dls = self._distill_unscaled(output_dict, self.scales)
            else:
                dls = [self.compute_distill_loss(output_dict, input_dict, scale) for scale in self.scales]
            for scale, dl in zip(self.scales, dls):
                losses["distilation/{}".format(scale)] = dl.detach()
                total = total + dl * distillation_weight
        losses["total_loss"] = total.detach()
        if not getattr(self, "is_log_image", True):
            hm = {}
        return {"loss": total, "loss_dict": losses, "hm": hm}


class FishEyeDecoder(MonoDepth2Decoder):
    """MonoDepth2Decoder for the Mei unified fisheye model (monodepth2_decoder.py:350-420): the network output is the
    ray norm, the 3-D point is the per-calibration ray table x norm, the relative pose acts on it directly and
    cam2image (mirror + radial distortion) maps it into the source frame; the overlap mask samples
    patched_mask x table mask.  Same fused HIP loss chain, ray-table variant (FsPhotoArgs.lut_ptrs; one, three or four
    source frames: FsPhotoMeiMultiArgs)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        from fsnet_amd.monodepth.networks.utils.mei_fisheye_utils import MeiCameraProjection
        self.mei_projection = MeiCameraProjection()
        self._staged = None          # (P2 tensor, its version, calib list) of the last staging: strong references,
        self._hook_staged = False    # so an equal identity really is the same batch object

    # head option (not in the reference): frame_ids of another length than [0, a, b] run the ray-table N-frame kernels
    # (fs_photo_mei_multi_*).  Without it such a list is refused as it always was: that refusal is pinned behaviour
    # (tests/test_photo64n_cpu.py, tests/test_distill_unscaled_cpu.py).  configs.meta_arch_cfg(fisheye=True) sets it
    # whenever the list it is given needs it.
    n_frame_kernels = False

    def _check_frame_ids(self):
        super()._check_frame_ids()
        if len(self.frame_ids) != 3 and not getattr(self, "n_frame_kernels", False):
            raise NotImplementedError("FishEyeDecoder: frame_ids %r — the two-source ray-table (Mei) loss kernels run "
                                      "exactly two source frames, [0, a, b]; set the head option n_frame_kernels=True "
                                      "for the N-frame ones" % (self.frame_ids,))

    def stage_step_inputs(self, input_dict, from_hook=True):
        """ray tables of this batch's calibrations (built once each, cached by the reference's key) -> the loss
        engine's persistent pointer table.  Host side; the training hook runs it before every step (before the H2D
        move, so P2 is normally still a host tensor) and before every hipGraph replay."""
        P, calib = input_dict["P2"], input_dict["calib_meta"]
        img0 = input_dict[("original_image", 0)]
        B, _, H, W = img0.shape
        dev = img0.device if img0.is_cuda else next(self.parameters()).device
        pl = self._loss_engine_for(B, H, W, dev)
        self._hook_staged = from_hook
        st = self._staged
        if st is not None and st[0] is P and st[1] == P._version and st[2] is calib and st[3] is pl and pl.fisheye:
            return
        tabs, rows = self.mei_projection.tables(H, W, P, calib, dev)
        pl.stage_fisheye(tabs, rows)
        self._staged = (P, P._version, calib, pl)

    def _stage_geometry(self, input_dict):
        if "calib_meta" not in input_dict:
            raise KeyError("FishEyeDecoder.loss needs input_dict['calib_meta'] (list of Mei calibration dicts)")
        if torch.cuda.is_current_stream_capturing():
            if not self._pl.fisheye:
                raise RuntimeError("FishEyeDecoder: stage_step_inputs() must run before the step is captured")
        elif self._hook_staged and self._pl.fisheye:
            pass                      # the hook staged this step's calibrations already
        else:
            self.stage_step_inputs(input_dict, from_hook=False)
        self._hook_staged = False

    def prefetch_loss_inputs(self, input_dict):
        return        # MonoDepthWPose has no side stream; the identity terms run inside loss()

    def get_prediction(self, input_dict, output_dict):
        norm = output_dict[("depth", 0, 0)]
        points, _ = self.mei_projection.image2cam(norm, input_dict["P2"], input_dict["calib_meta"])
        return dict(depth=points[..., 2], norm=norm)
