"""Generate golden vectors by running the REAL reference (/root/reference) on CPU.

Dev-only: runs in the build container (the reference never travels to the GPU box).  Imports the
reference with the import shims of SURVEY Appendix A, feeds seeded synthetic inputs and writes
inputs + reference outputs to tests/golden/*.npz.  It also cross-checks oracle/fsnet_oracle.py
against the reference while doing so (prints max deviations).

    python tools/gen_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools", "ref_shims"), "/root/reference", ROOT]
tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = type("SummaryWriter", (), {})
sys.modules["torch.utils.tensorboard"] = tb
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
torch.cuda.synchronize = lambda *a, **k: None

from easydict import EasyDict  # noqa: E402
from vision_base.utils.builder import build  # noqa: E402
from monodepth.networks.utils import monodepth_utils as mu  # noqa: E402
from oracle import fsnet_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
os.makedirs(GOLD, exist_ok=True)
torch.set_num_threads(8)


def npy(t):
    return t.detach().cpu().numpy()


def ref_model(H, W, with_pose=True, depth=18, frozen_stages=-1, norm_eval=False):
    enc = [64, 64, 128, 256, 512]
    bb = dict(name='vision_base.networks.models.backbone.resnet.resnet', depth=depth, pretrained=False,
              frozen_stages=frozen_stages, num_stages=4, out_indices=(-1, 0, 1, 2, 3), norm_eval=norm_eval,
              dilations=(1, 1, 1, 1))
    head = dict(name='monodepth.networks.models.heads.monodepth2_decoder.MonoDepth2Decoder', scales=[0, 1, 2, 3],
                height=H, width=W, min_depth=0.5, max_depth=100.0, overlapped_mask=True, is_log_image=False,
                depth_decoder_cfg=dict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoder',
                                       num_ch_enc=np.array(enc), num_output_channels=16, use_skips=True,
                                       scales=[0, 1, 2, 3], min_depth=0.5, max_depth=100))
    kw = dict(depth_backbone_cfg=bb, head_cfg=head, train_cfg=EasyDict(frame_ids=[0, 1, -1]), test_cfg=EasyDict())
    if with_pose:
        head['pose_decoder_cfg'] = dict(name='monodepth.networks.models.heads.pose_decoder.PoseDecoder',
                                        num_ch_enc=np.array(enc), num_input_features=1,
                                        num_frames_to_predict_for=2, stride=1)
        kw['pose_backbone_cfg'] = dict(bb, num_input_images=2)
        name = 'monodepth.networks.models.meta_archs.monodepth2_model.MonoDepthMeta'
    else:
        name = 'monodepth.networks.models.meta_archs.monodepth2_model.MonoDepthWPose'
    return build(name=name, **kw)


def dev(a, b):
    return float((a.double() - b.double()).abs().max())


def gen_ops():
    """op-level vectors (tiny shapes) straight from the reference's functions."""
    g = torch.Generator().manual_seed(11)
    out = {}
    B, H, W = 2, 24, 40
    # --- geometry: BackprojectDepth + Project3D (monodepth_utils.py:101-165) ---
    depth = 0.5 + 30 * torch.rand(B, 1, H, W, generator=g)
    data = O.synthetic_batch(B, H, W, seed=5)
    K = np.zeros([B, 4, 4]); K[:, :3, :3] = data['P2'][:, :3, :3].numpy(); K[:, 3, 3] = 1
    invK = np.linalg.pinv(K)
    aa = 0.02 * torch.randn(B, 1, 3, generator=g)
    tr = 0.3 * torch.randn(B, 1, 3, generator=g)
    T = mu.transformation_from_parameters(aa, tr, invert=False)
    Ti = mu.transformation_from_parameters(aa, tr, invert=True)
    cam = mu.BackprojectDepth()(depth, torch.from_numpy(invK).float())
    pix = mu.Project3D()(cam, torch.from_numpy(K).float(), T, B, H, W)
    out.update(geo_depth=npy(depth), geo_P2=npy(data['P2']), geo_aa=npy(aa), geo_tr=npy(tr), geo_T=npy(T),
               geo_Tinv=npy(Ti), geo_pix=npy(pix))
    Ko, invKo = O.intrinsics(data['P2'])
    print("oracle pix dev", dev(O.project(O.backproject(depth, invKo), Ko, T, H, W), pix),
          "T dev", dev(O.transformation_from_parameters(aa, tr), T),
          dev(O.transformation_from_parameters(aa, tr, True), Ti))
    # --- SSIM / reprojection / smoothness (monodepth_utils.py:168-215; decoder.py:118-128) ---
    x = torch.rand(B, 3, H, W, generator=g); y = (x + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    s = mu.SSIM()(x, y)
    dec = ref_model(64, 128, True).head
    rl = dec.compute_reprojection_loss(x, y)
    disp = torch.rand(B, 1, H, W, generator=g)
    sm = mu.get_smooth_loss(disp, x)
    out.update(ssim_x=npy(x), ssim_y=npy(y), ssim_out=npy(s), reproj_out=npy(rl), smooth_disp=npy(disp),
               smooth_out=npy(sm))
    print("oracle ssim dev", dev(O.ssim(x, y), s), "reproj", dev(O.reprojection_loss(x, y), rl), "smooth",
          dev(O.smooth_loss(disp, x), sm))
    # --- depth head (depth_encoder.py:76-88,114-121) ---
    logits = 6 * torch.randn(B, 16, 6, 10, generator=g)
    dd = dec.depth_decoder
    d_ref = dd._gather_activation(logits)
    disp_ref = mu.depth_to_disp(d_ref, 0.5, 100.0)
    out.update(head_logits=npy(logits), head_bins=npy(dd.depth_bins), head_depth=npy(d_ref), head_disp=npy(disp_ref))
    print("oracle bins dev", dev(O.depth_bins(0.5, 100, 16), dd.depth_bins), "head",
          dev(O.gather_activation(logits, dd.depth_bins), d_ref))
    np.savez_compressed(os.path.join(GOLD, "ops.npz"), **out)


def gen_loss_chain():
    """MonoDepth2Decoder.loss on synthetic network outputs (no network): loss_dict, dL/d depth_s,
    dL/d cam_T_cam (monodepth2_decoder.py:61-116, 205-347)."""
    B, H, W = 2, 64, 96
    data = O.synthetic_batch(B, H, W, seed=21)
    data['patched_mask'][:, :6, :] = 0  # exercise the overlapped-mask / patched-mask path
    g = torch.Generator().manual_seed(3)
    dec = ref_model(H, W, True).head
    outputs = {}
    leaves = {}
    for s in range(4):
        h, w = H >> s, W >> s
        ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
        d = (4 + 25 * (1 - ys) + 3 * torch.rand(B, 1, h, w, generator=g)).requires_grad_(True)
        leaves[("depth", s)] = d
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        aa = (0.01 * torch.randn(B, 1, 3, generator=g)).requires_grad_(True)
        tr = torch.tensor([[[0.02, -0.01, -0.6 if f > 0 else 0.6]]]).repeat(B, 1, 1) + 0.02 * torch.randn(B, 1, 3, generator=g)
        tr.requires_grad_(True)
        leaves[("aa", f)], leaves[("tr", f)] = aa, tr
        outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
    torch.manual_seed(0)
    res = dec.loss(outputs, data)
    res['loss'].backward()
    out = {"H": H, "W": W, "seed": 21, "total_loss": npy(res['loss'])}
    for k, v in res['loss_dict'].items():
        out["ld_" + k.replace('/', '_')] = npy(v)
    for s in range(4):
        out["depth_%d" % s] = npy(leaves[("depth", s)])
        out["gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
        out["minidx_%d" % s] = 0
    for f in (1, -1):
        tag = "p" if f > 0 else "m"
        out["aa_" + tag], out["tr_" + tag] = npy(leaves[("aa", f)]), npy(leaves[("tr", f)])
        out["gaa_" + tag], out["gtr_" + tag] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
        out["warp0_" + tag] = npy(outputs[("original_image", f, 0)])[:, :, ::4, ::4]
        out["ovmask0_" + tag] = npy(outputs[("overlapped_mask", f, 0)])
    for f in (0, 1, -1):
        out["img_%s" % {0: "0", 1: "p", -1: "m"}[f]] = npy(data[("original_image", f)])
    out["P2"] = npy(data["P2"]); out["patched_mask"] = npy(data["patched_mask"])
    # cross-check the oracle
    o2 = {}
    lv = {}
    for s in range(4):
        d = leaves[("depth", s)].detach().clone().requires_grad_(True); lv[s] = d
        o2[("depth", s, s)] = d; o2[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        o2[("cam_T_cam", f)] = outputs[("cam_T_cam", f)].detach()
    tot, ld = O.photometric_loss(o2, data)
    tot.backward()
    print("oracle chain: loss dev", dev(tot, res['loss']), "gdepth0 dev rel",
          dev(lv[0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max()))
    np.savez_compressed(os.path.join(GOLD, "loss_chain.npz"), **out)


def gen_loss_chain_nsrc():
    """gen_loss_chain for frame_ids of other lengths: MonoDepth2Decoder.loss of the reference with 1, 3 and 4 temporal
    source frames at 24 x 56, B = 2 -> inputs, per-scale losses, total, min_idx and the gradients (loss_chain_nsrc.npz)."""
    B, H, W = 2, 24, 56
    out = {"H": H, "W": W}
    for fids in ([0, -1], [0, -2, -1, 1], [0, -2, -1, 1, 2]):
        N = len(fids) - 1
        tag = "n%d_" % N
        data = O.synthetic_batch(B, H, W, seed=30 + N, frame_ids=tuple(fids))
        data['patched_mask'][:, :3, :] = 0
        g = torch.Generator().manual_seed(5 + N)
        dec = ref_model(H, W, False).head
        dec.frame_ids = list(fids)
        outputs, leaves = {}, {}
        for s in range(4):
            h, w = H >> s, W >> s
            ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
            d = (4 + 25 * (1 - ys) + 3 * torch.rand(B, 1, h, w, generator=g)).requires_grad_(True)
            leaves[("depth", s)] = d
            outputs[("depth", s, s)] = d
            outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 100.0)
        for f in fids[1:]:
            aa = (0.01 * torch.randn(B, 1, 3, generator=g)).requires_grad_(True)
            tr = torch.tensor([[[0.02, -0.01, -0.3 * f]]]).repeat(B, 1, 1) + 0.02 * torch.randn(B, 1, 3, generator=g)
            tr.requires_grad_(True)
            leaves[("aa", f)], leaves[("tr", f)] = aa, tr
            outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
        torch.manual_seed(0)
        res = dec.loss(outputs, data)
        res['loss'].backward()
        out[tag + "frame_ids"] = np.asarray(fids, np.int64)
        out[tag + "total_loss"] = npy(res['loss'])
        for k, v in res['loss_dict'].items():
            out[tag + "ld_" + k.replace('/', '_')] = npy(v)
        # cross-check the oracle, under the same tie-break noise, and take min_idx from it (the reference keeps its index
        # in a local variable)
        o2, lv = {}, {}
        for s in range(4):
            d = leaves[("depth", s)].detach().clone().requires_grad_(True); lv[s] = d
            o2[("depth", s, s)] = d; o2[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
        for f in fids[1:]:
            o2[("cam_T_cam", f)] = outputs[("cam_T_cam", f)].detach()
        # the reference's tie-break noise (:258-259) is the first draw after torch.manual_seed(0), one per scale
        torch.manual_seed(0)
        noise = {s: torch.randn(B, N, H, W) * 0.00001 for s in range(4)}
        tot, ld = O.photometric_loss(o2, data, frame_ids=tuple(fids), noise=noise)
        tot.backward()
        print("oracle chain N=%d: loss dev" % N, dev(tot, res['loss']), "gdepth0 dev rel",
              dev(lv[0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max()))
        for s in range(4):
            out[tag + "depth_%d" % s] = npy(leaves[("depth", s)])
            out[tag + "gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
            out[tag + "minidx_%d" % s] = npy(o2[("min_idx", s)]).astype(np.uint8)
        for f in fids[1:]:
            out[tag + "aa_%d" % f], out[tag + "tr_%d" % f] = npy(leaves[("aa", f)]), npy(leaves[("tr", f)])
            out[tag + "gaa_%d" % f], out[tag + "gtr_%d" % f] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
        for f in fids:
            out[tag + "img_%d" % f] = npy(data[("original_image", f)])
        out[tag + "P2"] = npy(data["P2"]); out[tag + "patched_mask"] = npy(data["patched_mask"])
    np.savez_compressed(os.path.join(GOLD, "loss_chain_nsrc.npz"), **out)


def gen_model(with_pose, tag, steps=3):
    """Full model: forward outputs, loss_dict, per-parameter grad norms, and parameter checksums
    after Adam steps driven by the reference's own BaseTrainingHook (clip 35.0)."""
    from vision_base.pipeline_hooks.train_val_hooks.base_training_hooks import BaseTrainingHook
    B, H, W = 2, 64, 128
    sd0 = O.init_state(seed=1, with_pose=with_pose)
    m = ref_model(H, W, with_pose)
    missing = m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    m.train()
    names = [k for k, _ in m.named_parameters()]
    assert names == [k for k in sd0 if O.is_param(k)], "parameter order/name mismatch"
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    hook = BaseTrainingHook(clip_gradients=35.0)
    out = {"B": B, "H": H, "W": W, "init_seed": 1}
    tr = O.OracleTrainer(sd0, with_pose=with_pose)
    for it in range(steps):
        data = O.synthetic_batch(B, H, W, seed=100 + it)
        if it == 0:
            torch.manual_seed(0)
            res = m(dict(data), dict(is_training=True))
            # forward-only capture on a copy of BN state: redo state restore below
            m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
            feats = None
        # capture forward outputs of step `it` through a manual pass identical to the hook
        opt.zero_grad()
        torch.manual_seed(0)
        d2 = dict(data)
        res = m(d2, dict(is_training=True))
        res['loss'].mean().backward()
        gn = torch.stack([p.grad.norm() for p in m.parameters()])
        total_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), 35.0)
        opt.step()
        out["loss_%d" % it] = npy(res['loss'])
        for k, v in res['loss_dict'].items():
            out["ld%d_%s" % (it, k.replace('/', '_'))] = npy(v)
        out["gradnorm_%d" % it] = npy(gn)
        out["totalnorm_%d" % it] = npy(total_norm)
        out["psum_%d" % it] = npy(torch.stack([p.double().sum() for p in m.parameters()]))
        out["pabs_%d" % it] = npy(torch.stack([p.double().abs().sum() for p in m.parameters()]))
        # oracle in lock-step
        tot, ld, o_out, raw, norm = tr.step(data)
        gn_o = torch.stack([raw[k].norm() for k in tr.names])
        print("[%s] step %d: ref loss %.9f oracle %.9f | gradnorm rel dev %.2e | total norm %.6f vs %.6f" % (
            tag, it, float(res['loss']), float(tot), float(((gn - gn_o).abs() / (gn + 1e-12)).max()),
            float(total_norm), float(norm)))
        if it == 0:
            # re-run reference forward for tensors (BN state already advanced: use oracle's outputs vs hooks)
            pass
    # forward tensors at the initial state (fresh model, train mode)
    m2 = ref_model(H, W, with_pose)
    m2.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    m2.train()
    data = O.synthetic_batch(B, H, W, seed=100)
    feats = m2.depth_backbone(data[('image', 0)])
    outs = m2.head.forward_depth(feats)
    for s in range(4):
        out["disp_%d" % s] = npy(outs[('disp', s)])
        out["depth_%d" % s] = npy(outs[('depth', s, s)])
    out["feat4"] = npy(feats[4])
    out["feat0_sub"] = npy(feats[0])[:, ::8, ::4, ::4]
    if with_pose:
        pf = m2.pose_backbone(torch.cat([data[('image', 0)], data[('image', 1)]], 1))
        aa, trn = m2.head.forward_pose([pf])
        out["axisangle_p"], out["translation_p"] = npy(aa), npy(trn)
    sdo = {k: v.clone() for k, v in sd0.items()}
    fo = O.resnet_forward(sdo, "depth_backbone.", data[('image', 0)])
    oo = O.depth_decoder_forward(sdo, "head.depth_decoder.", fo, 0.5, 100.0)
    print("[%s] oracle fwd dev: feat4 %.2e disp0 %.2e" % (tag, dev(fo[4], feats[4]), dev(oo[('disp', 0)], outs[('disp', 0)])))
    sd_ref = m.state_dict()
    print("[%s] after %d steps: max param dev oracle vs ref %.3e; running_mean dev %.3e" % (
        tag, steps, max(dev(tr.sd[k], sd_ref[k]) for k in tr.names),
        max(dev(tr.sd[k], sd_ref[k]) for k in sd_ref if k.endswith('running_mean'))))
    out["bn_rm_final"] = npy(torch.cat([sd_ref[k].flatten() for k in sd_ref if k.endswith('running_mean')]))
    out["bn_rv_final"] = npy(torch.cat([sd_ref[k].flatten() for k in sd_ref if k.endswith('running_var')]))
    np.savez_compressed(os.path.join(GOLD, "model_%s.npz" % tag), **out)


def gen_eval():
    """depth-error metrics of the REAL reference (monodepth_utils.compute_errors) on seeded inputs"""
    from oracle import eval_oracle as EO
    rng = np.random.RandomState(7)
    out = {}
    for k, n in enumerate((1, 7, 4096)):
        gt = (rng.rand(n).astype(np.float32) * 79 + 0.5)
        pred = (gt * np.exp(rng.randn(n).astype(np.float32) * 0.2)).astype(np.float32).clip(1e-3, 80.0)
        ref = np.array(mu.compute_errors(gt, pred), dtype=np.float64)
        mine = np.array(EO.compute_errors(gt, pred), dtype=np.float64)
        print("compute_errors case %d: oracle - reference max abs %.3e" % (k, np.abs(ref - mine).max()))
        out["gt_%d" % k], out["pred_%d" % k], out["err_%d" % k] = gt, pred, ref
    np.savez_compressed(os.path.join(GOLD, "eval.npz"), **out)


def _real_distill_step(H, W, B, seed, teacher_seed, batch_seed, **head_flags):
    """one training step of the REAL DistillWPoseMeta with its gradients -> (model, output, batch)"""
    import tempfile
    from oracle import distill_oracle as D
    enc = dict(name='vision_base.networks.models.backbone.resnet.resnet', depth=18, pretrained=False, frozen_stages=-1,
               num_stages=4, out_indices=(-1, 0, 1, 2, 3), norm_eval=False, dilations=(1, 1, 1, 1))
    dec = dict(num_ch_enc=np.array([64, 64, 128, 256, 512]), num_output_channels=16, use_skips=True, scales=[0, 1, 2, 3],
               min_depth=0.5, max_depth=100)
    sd = D.init_states(seed=seed, teacher_seed=teacher_seed)
    with tempfile.TemporaryDirectory() as d:
        tpath = os.path.join(d, "teacher.pth")
        torch.save({k[len("teacher_net."):]: v.clone() for k, v in sd.items() if k.startswith("teacher_net.")}, tpath)
        m = build(name='monodepth.networks.models.meta_archs.monodepth2_model.DistillWPoseMeta',
                  teacher_net_cfg=EasyDict(name='monodepth.networks.models.meta_archs.teacher_model.MonoDepthInference',
                                           backbone_cfg=EasyDict(**enc),
                                           depth_head_cfg=EasyDict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoder', **dec)),
                  teacher_net_path=tpath,
                  depth_backbone_cfg=EasyDict(**enc),
                  head_cfg=EasyDict(name='monodepth.networks.models.heads.monodepth2_decoder.MonoDepth2Decoder',
                                    scales=[0, 1, 2, 3], height=H, width=W, min_depth=0.5, max_depth=100.0,
                                    overlapped_mask=True, is_log_image=False, distillation_loss_weight=0.3,
                                    depth_decoder_cfg=EasyDict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoderUncertain', **dec),
                                    **dict(dict(is_uncertain_distill=True), **head_flags)),
                  train_cfg=EasyDict(frame_ids=[0, 1, -1]), test_cfg=EasyDict())
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m.train()
    data = O.synthetic_batch(B, H, W, seed=batch_seed)
    torch.manual_seed(0)
    out = m(dict(data), dict(is_training=True, epoch_num=0, global_step=0))
    out["loss"].backward()
    return m, out, data


def gen_distill():
    """self-distillation stage through the REAL DistillWPoseMeta (monodepth2_model.py:150-206): loss terms and
    parameter-gradient norms on a seeded batch; cross-checks oracle/distill_oracle.py"""
    from oracle import distill_oracle as D
    H, W, B = 64, 128, 2
    m, out, data = _real_distill_step(H, W, B, 21, 22, 400)
    names = [k for k, _ in m.named_parameters() if not k.startswith("teacher_net.")]
    gn = np.array([float(p.grad.norm()) if p.grad is not None else 0.0 for k, p in m.named_parameters()
                   if not k.startswith("teacher_net.")])
    res = {"B": B, "H": H, "W": W, "seed": 21, "teacher_seed": 22, "batch_seed": 400,
           "loss": float(out["loss"].detach()), "gradnorm": gn,
           "unc_w_grad": npy(dict(m.named_parameters())["head.depth_decoder.decoder.14.weight"].grad),
           "teacher_depth_0_mean": float(m.teacher_net.compute_teacher_depth(data[("image", 0)])[("teacher_depth", 0, 0)].mean())}
    for k, v in out["loss_dict"].items():
        res["ld_" + k.replace("/", "_")] = float(v)
    # oracle against the reference
    sdo = D.init_states(seed=21, teacher_seed=22)
    for k in sdo:
        if D.is_student_param(k):
            sdo[k].requires_grad_(True)
    tot, losses, _ = D.forward_train(sdo, O.synthetic_batch(B, H, W, seed=400))
    tot.backward()
    gno = np.array([float(sdo[k].grad.norm()) for k in names])
    print("distill: loss ref %.8f oracle %.8f | gradnorm max rel dev %.3e" % (
        res["loss"], float(tot), np.abs(gno - gn).max() / gn.max()))
    for k in losses:
        if k.startswith("distilation"):
            print("   %s ref %.6f oracle %.6f" % (k, res["ld_" + k.replace("/", "_")], float(losses[k])))
    np.savez_compressed(os.path.join(GOLD, "distill.npz"), **res)


def gen_distill_unscaled():
    """is_unscaled_distill (monodepth2_decoder.py:185-203): the REAL compute_distill_loss on the small cases of
    tests/helpers_distill_unscaled.py with gradients, with and without is_uncertain_distill, and the REAL DistillWPoseMeta
    step of gen_distill with the flag set; cross-checks the helper's restatement and its oracle step.  Layout of the
    file: helpers_distill_unscaled.golden_rows() / digest()"""
    from tests import helpers_distill_unscaled as HU
    from oracle import distill_oracle as D
    head = ref_model(64, 128, with_pose=False).head
    head.is_unscaled_distill = True
    rows = HU.golden_rows()
    k_loss = np.zeros([len(rows), 2], np.float32)
    k_grad = np.zeros([len(rows), 2, 2, HU.SAMPLES + 2], np.float32)      # [row][with_unc][d_pred, d_uncertain][digest]
    worst = 0.0
    for r, (name, s) in enumerate(rows):
        c = HU.case(name)
        for unc in (0, 1):
            head.is_uncertain_distill = bool(unc)
            p = c["pred"][s].clone().requires_grad_(True)
            u = c["uncertain"][s].clone().requires_grad_(True)
            od = {("depth", 7, 7): p, ("teacher_depth", 7, 7): c["teacher"][s].clone(), ("uncertain_z", 7): u}
            loss = head.compute_distill_loss(od, {}, 7)
            loss.backward()
            k_loss[r, unc] = float(loss.detach())
            k_grad[r, unc, 0] = HU.digest(p.grad)
            if unc:
                k_grad[r, unc, 1] = HU.digest(u.grad)
            mine = HU.restate(c["pred"][s], c["teacher"][s], c["uncertain"][s] if unc else None)
            worst = max(worst, dev(mine[0], loss.detach()), dev(mine[1], p.grad) / float(p.grad.abs().max()))
    print("distill_unscaled: restatement vs the real method, worst deviation %.3e" % worst)
    M = HU.MODEL
    m_loss = np.zeros([2, 5], np.float32)                                   # [with_unc][total, distilation/0..3]
    m_gradnorm = []
    for unc in (0, 1):
        m, out, data = _real_distill_step(M["H"], M["W"], M["B"], M["seed"], M["teacher_seed"], M["batch_seed"],
                                          is_unscaled_distill=True, is_uncertain_distill=bool(unc))
        names = [k for k, _ in m.named_parameters() if not k.startswith("teacher_net.")]
        m_gradnorm.append([float(p.grad.norm()) if p.grad is not None else 0.0 for k, p in m.named_parameters()
                           if not k.startswith("teacher_net.")])
        m_loss[unc] = [float(out["loss"].detach())] + [float(out["loss_dict"]["distilation/%d" % s]) for s in range(4)]
        sdo = D.init_states(seed=M["seed"], teacher_seed=M["teacher_seed"])
        for k in sdo:
            if D.is_student_param(k):
                sdo[k].requires_grad_(True)
        tot, losses, _ = HU.forward_train_unscaled(sdo, O.synthetic_batch(M["B"], M["H"], M["W"], seed=M["batch_seed"]),
                                                   is_uncertain_distill=bool(unc))
        tot.backward()
        gno = np.array([float(sdo[k].grad.norm()) if sdo[k].grad is not None else 0.0 for k in names])
        gn = np.array(m_gradnorm[-1])
        print("distill_unscaled[unc=%d]: loss ref %.8f oracle %.8f | gradnorm max rel dev %.3e | distilation/0 ref %.6f "
              "oracle %.6f" % (unc, m_loss[unc, 0], float(tot.detach()), np.abs(gno - gn).max() / gn.max(), m_loss[unc, 1],
                               float(losses["distilation/0"])))
    np.savez_compressed(os.path.join(GOLD, "distill_unscaled.npz"), k_seed=np.array([HU.case(n)["seed"] for n in HU.SMALL], np.int32),
                        k_loss=k_loss, k_grad=k_grad, m_loss=m_loss, m_gradnorm=np.array(m_gradnorm, np.float32))


def gen_augment():
    """Training input pipeline (configs/kitti_wpose_example:129-155) through the REAL reference classes, built by
    the reference's own builder.  cv2 is absent here: tools/ref_shims/cv2 routes warpAffine / cvtColor to the oracle's
    restatement, so this pins draw order, P2 / pose bookkeeping, mirror, colour arithmetic and Normalize — not OpenCV."""
    from oracle import augment_oracle as A
    aug = 'vision_base.data.augmentations.augmentations'
    frame_idxs = [0, 1, -1]
    out_h, out_w, H, W = 24, 80, 300, 420
    resize_keys = [('image', i) for i in frame_idxs] + [('original_image', i) for i in frame_idxs]
    colour_keys = [('image', i) for i in frame_idxs]
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    seeds = dict(warp=101, bright=102, contrast=103, sat=104)
    E = EasyDict
    cfg = E(name='vision_base.utils.builder.Sequential', cfg_list=[
        E(name=aug + '.ConvertToFloat'),
        E(name=aug + '.RandomWarpAffine', output_w=out_w, output_h=out_h, random_seed=seeds['warp']),
        E(name=aug + '.RandomMirror', mirror_prob=0.5, pose_axis_pairs=[(("relative_pose", i), 0) for i in frame_idxs[1:]]),
        E(name='vision_base.utils.builder.Shuffle', cfg_list=[
            E(name=aug + '.RandomBrightness', distort_prob=1.0, random_seed=seeds['bright']),
            E(name=aug + '.RandomContrast', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seeds['contrast']),
            E(name='vision_base.utils.builder.Sequential', cfg_list=[
                E(name=aug + '.ConvertColor', transform='HSV'),
                E(name=aug + '.RandomSaturation', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seeds['sat']),
                E(name=aug + '.ConvertColor', current='HSV', transform='RGB')])],
          image_keys=colour_keys),
        E(name=aug + '.Normalize', mean=mean, stds=std, image_keys=colour_keys),
        E(name=aug + '.Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]),
          image_keys=[('original_image', i) for i in frame_idxs]),
        E(name=aug + '.ConvertToTensor')],
        image_keys=resize_keys, calib_keys=['P2'], gt_image_keys=['patched_mask'])
    transform = build(**cfg)
    # the oracle draws from generators seeded like the reference instances
    rngs = {k: np.random.default_rng(v) for k, v in seeds.items()}
    res = dict(H=H, W=W, out_h=out_h, out_w=out_w, mean=mean, std=std, n=4, frame_seed=900, global_seed=77,
               **{"seed_" + k: v for k, v in seeds.items()})
    np.random.seed(77)
    gstate = np.random.get_state()
    maxdev = 0.0
    for n in range(4):
        fr = np.random.RandomState(900 + n)
        frames = [fr.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in frame_idxs]
        P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.0027]], dtype=np.float64)
        poses = []
        for j in range(2):
            from scipy.spatial.transform import Rotation as R
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = R.from_euler('xyz', fr.uniform(-0.05, 0.05, 3)).as_matrix()
            T[:3, 3] = fr.uniform(-1, 1, 3)
            poses.append(T)
        data = {}
        for i, f in zip(frame_idxs, frames):
            data[('image', i)] = f.copy()
            data[('original_image', i)] = f.copy()
        data['patched_mask'] = np.ones([H, W])
        data['P2'] = P2.copy()
        for i, T in zip(frame_idxs[1:], poses):
            data[('relative_pose', i)] = T.copy()
        np.random.set_state(gstate)
        out = transform(data)
        # the same sample through the oracle, with the global stream rewound to the same point
        np.random.set_state(gstate)
        plan = A.draw_plan(rngs['warp'], rngs['bright'], rngs['contrast'], rngs['sat'], H, W, out_w, out_h)
        gstate = np.random.get_state()
        imgs, origs, mask = A.run_sample(frames, plan, out_w, out_h, mean, std)
        P = A.warp_P2(P2, plan["final_scale"], plan["shift_w"], plan["shift_h"])
        if plan["mirror"]:
            P = A.mirror_P2(P, out_w)
        for j, i in enumerate(frame_idxs):
            res["s%d_image_%d" % (n, j)] = npy(out[('image', i)])
            res["s%d_orig_%d" % (n, j)] = npy(out[('original_image', i)])
            maxdev = max(maxdev, float(np.abs(npy(out[('image', i)]) - imgs[j]).max()),
                         float(np.abs(npy(out[('original_image', i)]) - origs[j]).max()))
        res["s%d_mask" % n] = npy(out['patched_mask'])
        res["s%d_P2" % n] = np.asarray(out['P2'])
        res["s%d_mirror" % n] = plan["mirror"]
        res["s%d_order" % n] = plan["order"]
        for j, i in enumerate(frame_idxs[1:]):
            res["s%d_pose_%d" % (n, j)] = np.asarray(out[('relative_pose', i)])
            want = A.flip_relative_pose(poses[j].copy(), 0) if plan["mirror"] else poses[j]
            maxdev = max(maxdev, float(np.abs(want - res["s%d_pose_%d" % (n, j)]).max()))
            res["s%d_pose_in_%d" % (n, j)] = poses[j]
        maxdev = max(maxdev, float(np.abs(mask - res["s%d_mask" % n]).max()), float(np.abs(P - res["s%d_P2" % n]).max()))
        print("augment sample %d: mirror=%s order=%s" % (n, plan["mirror"], plan["order"]))
    print("augment: oracle vs reference classes, max abs deviation over images/masks/P2/poses: %.3e" % maxdev)
    # validation input: ConvertToFloat, Resize, Normalize, ConvertToTensor (configs/kitti_wpose_example:156-166)
    if not hasattr(np, "int"):
        np.int = int          # the reference's Resize uses the alias numpy removed in 1.24 (:134, :157)
    vdev = 0.0
    for tag, kw, shp in (("stretch", dict(preserve_aspect_ratio=False), (75, 250)),
                         ("pad1", dict(preserve_aspect_ratio=True, force_pad=True), (120, 250)),
                         ("pad0", dict(preserve_aspect_ratio=True, force_pad=True), (60, 400)),
                         ("crop1", dict(preserve_aspect_ratio=True, force_pad=False), (60, 400))):
        vt = build(**E(name='vision_base.utils.builder.Sequential', cfg_list=[
            E(name=aug + '.ConvertToFloat'), E(name=aug + '.Resize', size=(48, 160), **kw),
            E(name=aug + '.Normalize', mean=mean, stds=std), E(name=aug + '.ConvertToTensor')],
            image_keys=[('image', 0)], calib_keys=['P2']))
        fr = np.random.RandomState(950 + len(tag))
        frame = fr.randint(0, 256, size=shp + (3,)).astype(np.uint8)
        P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.0027]], dtype=np.float64)
        out = vt({('image', 0): frame.copy(), 'P2': P2.copy()})
        res["val_%s_image" % tag] = npy(out[('image', 0)])
        res["val_%s_P2" % tag] = np.asarray(out['P2'])
        res["val_%s_shape" % tag] = np.array(shp)
        res["val_%s_seed" % tag] = 950 + len(tag)
        res["val_%s_effective" % tag] = np.asarray(out[('image_resize', 'effective_size')])
        res["val_%s_original" % tag] = np.asarray(out[('image_resize', 'original_shape')])
        vdev = max(vdev, float(np.abs(A.run_val_sample(frame, (48, 160), mean, std, **kw) - res["val_%s_image" % tag]).max()))
    print("augment (validation Resize): oracle vs reference class, max abs deviation %.3e" % vdev)
    np.savez_compressed(os.path.join(GOLD, "augment.npz"), **res)


def gen_augment_resize():
    """Training input of the Resize-based shipped configs (configs/multi_dataset_example:178-205) through the REAL
    reference classes: Resize of six frames + nearest patched_mask, Shuffle of the colour ops, RandomMirror AFTER
    them, two Normalizes.  cv2.resize is the shim's restatement (unpinned, like warpAffine)."""
    from oracle import augment_oracle as A
    if not hasattr(np, "int"):
        np.int = int
    aug = 'vision_base.data.augmentations.augmentations'
    frame_idxs = [0, 1, -1]
    size = (48, 160)
    resize_keys = [('image', i) for i in frame_idxs] + [('original_image', i) for i in frame_idxs]
    colour_keys = [('image', i) for i in frame_idxs]
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    seeds = dict(bright=202, contrast=203, sat=204)
    E = EasyDict
    cfg = E(name='vision_base.utils.builder.Sequential', cfg_list=[
        E(name=aug + '.ConvertToFloat'),
        E(name=aug + '.Resize', size=size, preserve_aspect_ratio=True, force_pad=True),
        E(name='vision_base.utils.builder.Shuffle', cfg_list=[
            E(name=aug + '.RandomBrightness', distort_prob=1.0, random_seed=seeds['bright']),
            E(name=aug + '.RandomContrast', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seeds['contrast']),
            E(name='vision_base.utils.builder.Sequential', cfg_list=[
                E(name=aug + '.ConvertColor', transform='HSV'),
                E(name=aug + '.RandomSaturation', distort_prob=1.0, lower=0.6, upper=1.4, random_seed=seeds['sat']),
                E(name=aug + '.ConvertColor', current='HSV', transform='RGB')])],
          image_keys=colour_keys),
        E(name=aug + '.RandomMirror', mirror_prob=0.5, pose_axis_pairs=[(("relative_pose", i), 0) for i in frame_idxs[1:]]),
        E(name=aug + '.Normalize', mean=mean, stds=std, image_keys=colour_keys),
        E(name=aug + '.Normalize', mean=np.array([0, 0, 0]), stds=np.array([1, 1, 1]),
          image_keys=[('original_image', i) for i in frame_idxs]),
        E(name=aug + '.ConvertToTensor')],
        image_keys=resize_keys, calib_keys=['P2'], gt_image_keys=['patched_mask'])
    transform = build(**cfg)
    rngs = {k: np.random.default_rng(v) for k, v in seeds.items()}
    shapes = [(75, 250), (120, 250), (60, 400), (96, 320)]      # pad_1, pad_1, pad_0, exact fit
    res = dict(size=np.array(size), mean=mean, std=std, n=len(shapes), frame_seed=1200, global_seed=88,
               shapes=np.array(shapes), **{"seed_" + k: v for k, v in seeds.items()})
    np.random.seed(88)
    gstate = np.random.get_state()
    maxdev = 0.0
    for n, (H, W) in enumerate(shapes):
        fr = np.random.RandomState(1200 + n)
        frames = [fr.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in frame_idxs]
        P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.0027]], dtype=np.float64)
        from scipy.spatial.transform import Rotation as R
        poses = []
        for j in range(2):
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = R.from_euler('xyz', fr.uniform(-0.05, 0.05, 3)).as_matrix()
            T[:3, 3] = fr.uniform(-1, 1, 3)
            poses.append(T)
        data = {}
        for i, f in zip(frame_idxs, frames):
            data[('image', i)] = f.copy()
            data[('original_image', i)] = f.copy()
        data['patched_mask'] = np.ones([H, W])
        data['P2'] = P2.copy()
        for i, T in zip(frame_idxs[1:], poses):
            data[('relative_pose', i)] = T.copy()
        np.random.set_state(gstate)
        out = transform(data)
        np.random.set_state(gstate)
        plan = A.draw_resize_plan(rngs['bright'], rngs['contrast'], rngs['sat'])
        gstate = np.random.get_state()
        imgs, origs, mask, syx = A.run_resize_train_sample(frames, plan, size, mean, std)
        P = P2.copy()
        P[0, :] *= syx[1]; P[1, :] *= syx[0]
        if plan["mirror"]:
            P = A.mirror_P2(P, size[1])
        for j, i in enumerate(frame_idxs):
            res["s%d_image_%d" % (n, j)] = npy(out[('image', i)])
            res["s%d_orig_%d" % (n, j)] = npy(out[('original_image', i)])
            maxdev = max(maxdev, float(np.abs(npy(out[('image', i)]) - imgs[j]).max()),
                         float(np.abs(npy(out[('original_image', i)]) - origs[j]).max()))
        res["s%d_mask" % n] = npy(out['patched_mask'])
        res["s%d_P2" % n] = np.asarray(out['P2'])
        res["s%d_mirror" % n] = plan["mirror"]
        res["s%d_order" % n] = plan["order"]
        for j, i in enumerate(frame_idxs[1:]):
            res["s%d_pose_%d" % (n, j)] = np.asarray(out[('relative_pose', i)])
            res["s%d_pose_in_%d" % (n, j)] = poses[j]
        maxdev = max(maxdev, float(np.abs(mask - res["s%d_mask" % n]).max()), float(np.abs(P - res["s%d_P2" % n]).max()))
        print("augment-resize sample %d: shape %s mirror=%s order=%s" % (n, (H, W), plan["mirror"], plan["order"]))
    print("augment-resize: oracle vs reference classes, max abs deviation %.3e" % maxdev)
    np.savez_compressed(os.path.join(GOLD, "augment_resize.npz"), **res)


def gen_augment_mask():
    """A patched_mask that is not all ones (NusceneJsonDataset's CAM_BACK, nuscene_dataset.py:176-191) through the REAL
    reference Resize, RandomWarpAffine and RandomMirror, built by the reference's own builder over the cases of
    tests/helpers_patched_mask.py, each with the mirror drawn on and off.  cv2.resize / cv2.warpAffine are the shim's
    restatement (unpinned, as in gen_augment_resize); what this pins is the reference's own handling of the mask: the
    order nearest resample -> pad / crop -> mirror, the modes, the dtype."""
    from tests import helpers_patched_mask as HM
    if not hasattr(np, "int"):
        np.int = int
    res = dict(resize_size=np.array(HM.RESIZE_SIZE), warp_out=np.array([HM.WARP_OUT_H, HM.WARP_OUT_W]))
    maxdev = 0.0
    for mirror in (False, True):
        transform = build(**HM.geometry_cfg("resize", mirror))
        for n, (frames, mask) in enumerate(HM.resize_inputs()):
            out = transform(HM.sample_dict(frames, mask))
            got = np.asarray(out['patched_mask'])
            assert got.dtype == np.float64 and set(np.unique(got)) <= {0.0, 1.0}
            res["resize%d_m%d" % (n, mirror)] = got.astype(np.uint8)
            res["resize%d_effective" % n] = np.asarray(out[('image_resize', 'effective_size')])
            maxdev = max(maxdev, float(np.abs(HM.expect_resize(mask, mirror) - got).max()))
        transform = build(**HM.geometry_cfg("warp", mirror))          # a fresh instance: the same seeded draws
        inputs = HM.warp_inputs()
        Ms = HM.warp_matrices([m.shape for _, m in inputs])
        for n, (frames, mask) in enumerate(inputs):
            out = transform(HM.sample_dict(frames, mask))
            got = np.asarray(out['patched_mask'])
            assert got.dtype == np.float64 and set(np.unique(got)) <= {0.0, 1.0}
            res["warp%d_m%d" % (n, mirror)] = got.astype(np.uint8)
            res["warp%d_M" % n] = Ms[n]
            maxdev = max(maxdev, float(np.abs(HM.expect_warp(mask, Ms[n], mirror) - got).max()))
    res["dtype"] = np.array("float64")
    print("augment-mask: oracle composition vs reference classes, max abs deviation %.3e" % maxdev)
    np.savez_compressed(os.path.join(GOLD, "augment_mask.npz"), **res)


def gen_augment_ext():
    """The remaining augmentation classes (CropTop, Pad2Shape, RandomCropToWidth, RandomHue, RandomEigenvalueNoise,
    PhotometricDistort, Copy; augmentations.py:228-375, :500-524, :594-680) through the REAL reference classes, built by
    the reference's own builder over the six chains of tests/helpers_augment_ext.py.  cv2 is the shim's restatement
    (unpinned, as in gen_augment).  The global seed of a case is the first one under which every RandomMirror of the
    chain is drawn on and off among the four samples (and, case d, both contrast positions occur)."""
    from tests import helpers_augment_ext as HX
    if not hasattr(np, "int"):
        np.int = int
    ref_aug, ref_builder = 'vision_base.data.augmentations.augmentations', 'vision_base.utils.builder'
    res = dict(frame_idxs=np.array(HX.FRAME_IDXS), sizes=np.array(HX.SIZES), mean=HX.MEAN, std=HX.STD)
    maxdev = 0.0

    def run(tag, c, global_seed, frame_seed):
        np.random.seed(c["build_seed"])
        ref = build(**HX.cfg(c["steps"], c["common"], ref_aug, ref_builder))
        np.random.seed(c["build_seed"])
        mine = HX.NumpyChain(c["steps"], c["common"])
        np.random.seed(global_seed)
        state = np.random.get_state()
        outs, wants, logs = [], [], []
        for n in range(len(HX.SIZES)):
            np.random.set_state(state)
            outs.append(ref(HX.sample(tag, n, frame_seed)))
            after = np.random.get_state()
            np.random.set_state(state)
            wants.append(mine(HX.sample(tag, n, frame_seed)))
            logs.append(mine.log)
            mine_next = np.random.rand()
            np.random.set_state(after)
            assert mine_next == np.random.rand(), "the two chains consumed the global stream differently"
            state = after
        np.random.set_state(state)
        return outs, wants, logs, np.random.rand()

    for k, tag in enumerate(HX.CASES):
        c = HX.case(tag)
        frame_seed = 2000 + 10 * k
        for global_seed in range(500 + 100 * k, 600 + 100 * k):
            outs, wants, logs, nxt = run(tag, c, global_seed, frame_seed)
            mirrors = np.array([l["mirrors"] for l in logs])
            ok = bool(np.all(mirrors.any(0) & ~mirrors.all(0)))
            if tag == "d":
                ok = ok and len({l["contrast_first"] for l in logs}) == 2
            if ok:
                break
        assert ok, tag
        if tag == "e":
            assert set().union(*[l["wraps"] for l in logs]) == {"up", "down"}, "the hue must wrap both ways"
        res["%s_global_seed" % tag], res["%s_frame_seed" % tag], res["%s_next" % tag] = global_seed, frame_seed, nxt
        res["%s_mirrors" % tag] = mirrors
        for n, (out, want) in enumerate(zip(outs, wants)):
            pre = "%s%d_" % (tag, n)
            frames = range(1) if tag == "f" else range(len(HX.FRAME_IDXS))      # f pins the masks; c has its pixels
            for j in frames:
                i = HX.FRAME_IDXS[j]
                for fam, short in (("image", "image"), ("original_image", "orig")):
                    got = HX.chw(npy(out[(fam, i)]) if isinstance(out[(fam, i)], torch.Tensor) else out[(fam, i)])
                    assert got.dtype == np.float32 and got.shape == (3,) + c["out_hw"], (tag, fam, got.dtype, got.shape)
                    res[pre + "%s_%d" % (short, j)] = got
                    maxdev = max(maxdev, float(np.abs(got - HX.chw(want[(fam, i)])).max()))
            mask = npy(out['patched_mask'])
            assert mask.dtype == np.float64 and set(np.unique(mask)) <= {0.0, 1.0}
            res[pre + "mask"] = mask.astype(np.uint8)
            maxdev = max(maxdev, float(np.abs(mask - want['patched_mask']).max()))
            if tag == "f":
                res[pre + "motion_mask"] = npy(out['motion_mask'])
                maxdev = max(maxdev, float(np.abs(res[pre + "motion_mask"].astype(np.float64) - want['motion_mask']).max()))
            res[pre + "P2"] = npy(out['P2'])
            maxdev = max(maxdev, float(np.abs(res[pre + "P2"] - np.asarray(want['P2'], dtype=np.float32)).max()))
            for j, i in enumerate(HX.FRAME_IDXS[1:]):
                res[pre + "pose_%d" % j] = np.asarray(out[('relative_pose', i)])
                maxdev = max(maxdev, float(np.abs(res[pre + "pose_%d" % j] - want[('relative_pose', i)]).max()))
            for key in (('image_resize', 'original_shape'), ('image_resize', 'effective_size')):
                if key in out:
                    res[pre + key[1]] = np.asarray(out[key])
        print("augment-ext case %s: global seed %d, mirrors %s%s" % (
            tag, global_seed, mirrors.astype(int).tolist(),
            ", contrast first %s" % [l["contrast_first"] for l in logs] if tag == "d" else ""))
    print("augment-ext: numpy composition vs reference classes, max abs deviation %.3e" % maxdev)
    np.savez_compressed(os.path.join(GOLD, "augment_ext.npz"), **res)
    print("augment_ext.npz: %d bytes" % os.path.getsize(os.path.join(GOLD, "augment_ext.npz")))


def gen_fisheye():
    """Fisheye path (BASELINE configs[3]) through the REAL classes: MeiCameraProjection LUT + cam2image
    (mei_fisheye_utils.py:14-187) and FishEyeDecoder.loss with gradients (monodepth2_decoder.py:350-420)."""
    from monodepth.networks.utils.mei_fisheye_utils import MeiCameraProjection
    from oracle import fisheye_oracle as FO
    out = {}
    proj = MeiCameraProjection()
    # --- LUT at 48x48 for two calibrations ---
    H = W = 48
    for v in range(2):
        P, calib = FO.synthetic_calib(H, W, v)
        norm = torch.ones(1, 1, H, W)
        pts, mask = proj.image2cam(norm, P[None], [calib])
        lut = np.stack([npy(pts[0, 0, ..., 0]), npy(pts[0, 0, ..., 1]), npy(pts[0, 0, ..., 2]), npy(mask[0, 0])], 0)
        out["lut%d" % v] = lut
        out["lut%d_P" % v] = npy(P)
        out["lut%d_calib" % v] = np.array([calib["distortion_parameters"]["k1"], calib["distortion_parameters"]["k2"],
                                           calib["mirror_parameters"]["xi"]])
        mine = np.stack(FO.mei_lut(H, W, P[0, 0].item(), P[1, 1].item(), P[0, 2].item(), P[1, 2].item(),
                                   calib["distortion_parameters"]["k1"], calib["distortion_parameters"]["k2"],
                                   calib["mirror_parameters"]["xi"]), 0)
        print("fisheye LUT %d: valid %.1f %%, oracle max dev %.3e, mask mismatches %d" % (
            v, 100 * lut[3].mean(), np.abs(mine[:3] - lut[:3]).max(), int((mine[3] != lut[3]).sum())))
    # --- cam2image on random points in front of / beside the camera ---
    g = torch.Generator().manual_seed(5)
    pts = torch.randn(64, 3, generator=g) * torch.tensor([3.0, 3.0, 2.0]) + torch.tensor([0.0, 0.0, 2.5])
    P, calib = FO.synthetic_calib(H, W, 0)
    uvz = proj.cam2image(pts, P, calib)
    out["c2i_points"], out["c2i_uvz"] = npy(pts), npy(uvz)
    u, v_ = FO.cam2image(pts, P, calib)
    print("fisheye cam2image oracle dev", dev(torch.stack([u, v_], -1), uvz[..., :2]))
    # --- loss chain with gradients ---
    B, H, W = 2, 64, 64
    data = O.synthetic_batch(B, H, W, seed=31)
    data['patched_mask'][:, :5, :] = 0
    Ps, calibs = zip(*[FO.synthetic_calib(H, W, v) for v in range(B)])
    data["P2"] = torch.stack(Ps, 0)
    data["calib_meta"] = list(calibs)
    g = torch.Generator().manual_seed(4)
    dec = build(name='monodepth.networks.models.heads.monodepth2_decoder.FishEyeDecoder', scales=[0, 1, 2, 3],
                height=H, width=W, frame_ids=[0, 1, -1], min_depth=0.5, max_depth=150.0, overlapped_mask=True,
                is_log_image=False,
                depth_decoder_cfg=dict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoder',
                                       num_ch_enc=np.array([64, 64, 128, 256, 512]), num_output_channels=64,
                                       use_skips=True, scales=[0, 1, 2, 3], min_depth=0.5, max_depth=150))
    outputs, leaves = {}, {}
    for s in range(4):
        h, w = H >> s, W >> s
        ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
        d = (5 + 20 * (1 - ys) + 3 * torch.rand(B, 1, h, w, generator=g)).requires_grad_(True)
        leaves[("depth", s)] = d
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 150.0)
    for f in (1, -1):
        aa = (0.01 * torch.randn(B, 1, 3, generator=g)).requires_grad_(True)
        tr = torch.tensor([[[0.6 if f > 0 else -0.6, -0.01, 0.03]]]).repeat(B, 1, 1) + 0.02 * torch.randn(B, 1, 3, generator=g)
        tr.requires_grad_(True)
        leaves[("aa", f)], leaves[("tr", f)] = aa, tr
        outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
    torch.manual_seed(0)
    res = dec.loss(outputs, data)
    res['loss'].backward()
    out.update(H=H, W=W, seed=31, total_loss=npy(res['loss']))
    for k, v in res['loss_dict'].items():
        out["ld_" + k.replace('/', '_')] = npy(v)
    for s in range(4):
        out["depth_%d" % s] = npy(leaves[("depth", s)])
        out["gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
    for f in (1, -1):
        tag = "p" if f > 0 else "m"
        out["aa_" + tag], out["tr_" + tag] = npy(leaves[("aa", f)]), npy(leaves[("tr", f)])
        out["gaa_" + tag], out["gtr_" + tag] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
        out["warp0_" + tag] = npy(outputs[("original_image", f, 0)])[:, :, ::2, ::2]
        out["ovmask0_" + tag] = npy(outputs[("overlapped_mask", f, 0)])
    for f in (0, 1, -1):
        out["img_%s" % {0: "0", 1: "p", -1: "m"}[f]] = npy(data[("original_image", f)])
    out["P2"] = npy(data["P2"]); out["patched_mask"] = npy(data["patched_mask"])
    out["calib"] = np.array([[c["distortion_parameters"]["k1"], c["distortion_parameters"]["k2"],
                              c["mirror_parameters"]["xi"]] for c in calibs])
    pred = dec.get_prediction(data, {("depth", 0, 0): leaves[("depth", 0)].detach()})
    out["pred_depth"] = npy(pred["depth"])
    # cross-check the oracle
    o2, lv = {}, {}
    for s in range(4):
        d = leaves[("depth", s)].detach().clone().requires_grad_(True); lv[s] = d
        o2[("depth", s, s)] = d; o2[("disp", s)] = O.depth_to_disp(d, 0.5, 150.0)
    for f in (1, -1):
        o2[("cam_T_cam", f)] = outputs[("cam_T_cam", f)].detach()
    tot, ld = FO.photometric_loss(o2, data)
    tot.backward()
    print("fisheye chain: ref loss %.9f oracle %.9f | gdepth0 dev rel %.3e | warp dev %.3e | ov mismatches %d" % (
        float(res['loss']), float(tot),
        dev(lv[0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max()),
        dev(o2[("original_image", 1, 0)], outputs[("original_image", 1, 0)]),
        int((o2[("overlapped_mask", 1, 0)] != outputs[("overlapped_mask", 1, 0)]).sum())))
    np.savez_compressed(os.path.join(GOLD, "fisheye.npz"), **out)


def gen_fisheye_nsrc():
    """gen_fisheye's loss chain for frame_ids of other lengths: the REAL FishEyeDecoder.loss with 1, 3 and 4 temporal
    source frames at 64 x 64, B = 2, on the inputs of tests/helpers_fisheye_n.py (every candidate of the per-pixel minimum
    wins somewhere) -> inputs, per-scale losses, total, gradients, the scale-0 warp (thinned ::2) and overlap masks, and
    min_idx from the oracle under the same noise (fisheye_nsrc.npz)."""
    from oracle import fisheye_oracle as FO
    from tests import helpers_fisheye_n as Q
    out = {}
    for N in (1, 3, 4):
        case = Q.make_case("golden-n%d" % N)
        fids, H, W, data = list(case["fids"]), case["H"], case["W"], case["data"]
        tag = "n%d_" % N
        dec = build(name='monodepth.networks.models.heads.monodepth2_decoder.FishEyeDecoder', scales=[0, 1, 2, 3],
                    height=H, width=W, frame_ids=fids, min_depth=0.5, max_depth=150.0, overlapped_mask=True,
                    is_log_image=False,
                    depth_decoder_cfg=dict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoder',
                                           num_ch_enc=np.array([64, 64, 128, 256, 512]), num_output_channels=64,
                                           use_skips=True, scales=[0, 1, 2, 3], min_depth=0.5, max_depth=150))
        outputs, leaves = {}, {}
        for s in range(4):
            d = case["depths"][s].clone().requires_grad_(True)
            leaves[("depth", s)] = d
            outputs[("depth", s, s)] = d
            outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 150.0)
        for f in fids[1:]:
            aa, tr = case["aa"][f].clone().requires_grad_(True), case["tr"][f].clone().requires_grad_(True)
            leaves[("aa", f)], leaves[("tr", f)] = aa, tr
            outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
        torch.manual_seed(0)
        res = dec.loss(outputs, data)
        res['loss'].backward()
        out[tag + "frame_ids"] = np.asarray(fids, np.int64)
        out[tag + "seed"] = np.int64(case["seed"])
        out[tag + "total_loss"] = npy(res['loss'])
        for k, v in res['loss_dict'].items():
            out[tag + "ld_" + k.replace('/', '_')] = npy(v)
        for s in range(4):
            out[tag + "depth_%d" % s] = npy(leaves[("depth", s)])
            out[tag + "gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
        for f in fids[1:]:
            out[tag + "aa_%d" % f], out[tag + "tr_%d" % f] = npy(leaves[("aa", f)]), npy(leaves[("tr", f)])
            out[tag + "gaa_%d" % f], out[tag + "gtr_%d" % f] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
            out[tag + "warp0_%d" % f] = npy(outputs[("original_image", f, 0)])[:, :, ::2, ::2]
            out[tag + "ovmask0_%d" % f] = npy(outputs[("overlapped_mask", f, 0)])
        for f in fids:
            out[tag + "img8_%d" % f] = case["u8"][f]         # the frame is uint8 / 255 (helpers_fisheye_n.image_from_u8)
        out[tag + "P2"] = npy(data["P2"]); out[tag + "patched_mask"] = npy(data["patched_mask"]).astype(np.uint8)
        # cross-check the oracle under the same tie-break noise, and take min_idx from it (the reference keeps its index
        # in a local variable)
        o = Q.oracle_chain(case, noise=Q.reference_noise(case), grads=True)
        for s in range(4):
            out[tag + "minidx_%d" % s] = npy(o["outputs"][("min_idx", s)]).astype(np.uint8)
        f1 = fids[1]
        print("fisheye chain N=%d: ref loss %.9f oracle %.9f | gdepth0 dev rel %.3e | warp dev %.3e | ov mismatches %d" % (
            N, float(res['loss']), float(o["total"]),
            dev(o["depths"][0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max()),
            dev(o["outputs"][("original_image", f1, 0)], outputs[("original_image", f1, 0)]),
            int((o["outputs"][("overlapped_mask", f1, 0)] != outputs[("overlapped_mask", f1, 0)]).sum())))
    out["calib"] = np.array([[c["distortion_parameters"]["k1"], c["distortion_parameters"]["k2"],
                              c["mirror_parameters"]["xi"]] for c in data["calib_meta"]])
    out.update(H=H, W=W)
    np.savez_compressed(os.path.join(GOLD, "fisheye_nsrc.npz"), **out)


def gen_model_r50fx():
    """BASELINE configs[4] wiring at a small size: MonoDepthWPose, ResNet-50 (Bottleneck), 64 depth bins,
    base_fx = 492 (configs/multi_dataset_example:227-257) with per-sample focal lengths; forward tensors, loss_dict and
    per-parameter gradient norms of one step from the REAL reference."""
    B, H, W = 2, 64, 128
    enc = [64, 256, 512, 1024, 2048]
    bb = dict(name='vision_base.networks.models.backbone.resnet.resnet', depth=50, pretrained=False,
              frozen_stages=-1, num_stages=4, out_indices=(-1, 0, 1, 2, 3), norm_eval=False, dilations=(1, 1, 1, 1))
    head = dict(name='monodepth.networks.models.heads.monodepth2_decoder.MonoDepth2Decoder', scales=[0, 1, 2, 3],
                height=H, width=W, min_depth=0.5, max_depth=100.0, overlapped_mask=True, is_log_image=False,
                depth_decoder_cfg=dict(name='monodepth.networks.models.heads.depth_encoder.MultiChannelDepthDecoder',
                                       num_ch_enc=np.array(enc), num_output_channels=64, use_skips=True,
                                       scales=[0, 1, 2, 3], min_depth=0.5, max_depth=100, base_fx=492))
    m = build(name='monodepth.networks.models.meta_archs.monodepth2_model.MonoDepthWPose', depth_backbone_cfg=bb,
              head_cfg=head, train_cfg=EasyDict(frame_ids=[0, 1, -1]), test_cfg=EasyDict())
    sd0 = O.init_state(seed=7, depth=50, with_pose=False, num_out=64)
    m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    m.train()
    data = O.synthetic_batch(B, H, W, seed=300)
    data["P2"][0, 0, 0] *= 1.4          # two focal lengths in the batch: depth scales 0.211 and 0.151
    data["P2"][1, 0, 0] *= 1.0
    torch.manual_seed(0)
    res = m(dict(data), dict(is_training=True))
    res['loss'].mean().backward()
    out = {"B": B, "H": H, "W": W, "init_seed": 7, "batch_seed": 300, "base_fx": 492.0, "fx_mul": np.array([1.4, 1.0]),
           "loss": npy(res['loss'])}
    for k, v in res['loss_dict'].items():
        out["ld_" + k.replace('/', '_')] = npy(v)
    out["gradnorm"] = npy(torch.stack([p.grad.norm() for p in m.parameters()]))
    m2 = build(name='monodepth.networks.models.meta_archs.monodepth2_model.MonoDepthWPose', depth_backbone_cfg=bb,
               head_cfg=head, train_cfg=EasyDict(frame_ids=[0, 1, -1]), test_cfg=EasyDict())
    m2.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    m2.train()
    feats = m2.depth_backbone(data[('image', 0)])
    outs = m2.head.forward_depth(feats, data['P2'])
    for s in range(4):
        out["disp_%d" % s] = npy(outs[('disp', s)])
        out["depth_%d" % s] = npy(outs[('depth', s, s)])
    out["feat4"] = npy(feats[4])[:, ::16]
    tr = O.OracleTrainer(sd0, depth=50, with_pose=False, base_fx=492.0)
    tot, ld, o_out, raw, norm = tr.step(data)
    gn_o = torch.stack([raw[k].norm() for k in tr.names])
    gn = torch.from_numpy(out["gradnorm"])
    print("[r50fx] ref loss %.9f oracle %.9f | gradnorm rel dev %.2e | depth0 dev %.2e" % (
        float(res['loss']), float(tot), float(((gn - gn_o).abs() / (gn + 1e-12)).max()),
        dev(o_out[('depth', 0, 0)], outs[('depth', 0, 0)])))
    np.savez_compressed(os.path.join(GOLD, "model_r50fx.npz"), **out)


def gen_kitti_dataset():
    """the REAL KittiDepthMonoDataset (mono_dataset.py:108-250) over the seeded fake KITTI tree of
    tests/helpers_kitti.py: filtered index, relative poses, P2, image tensors"""
    import tempfile
    from tests import helpers_kitti as HK
    from monodepth.data.datasets.mono_dataset import KittiDepthMonoDataset
    out = {}
    with tempfile.TemporaryDirectory() as d:
        raw, split = HK.make_tree(d, seed=5)
        ds = KittiDepthMonoDataset(**HK.dataset_cfg(raw, split, prefix=''))
        out["n"] = len(ds)
        out["index"] = np.array([[o["index"], 0 if o["side"] == "l" else 1] for o in ds.imdb])
        for i in range(len(ds)):
            smp = ds[i]
            for f, tag in ((0, "0"), (1, "p"), (-1, "m")):
                out["s%d_image_%s" % (i, tag)] = npy(smp[("image", f)])
                out["s%d_orig_%s" % (i, tag)] = npy(smp[("original_image", f)])
            out["s%d_pose_p" % i], out["s%d_pose_m" % i] = np.asarray(smp[("relative_pose", 1)]), np.asarray(smp[("relative_pose", -1)])
            out["s%d_P2" % i], out["s%d_original_P2" % i] = np.asarray(smp["P2"]), np.asarray(smp["original_P2"])
            out["s%d_mask" % i] = npy(smp["patched_mask"])
    print("kitti dataset: %d of 5 split entries kept, sides %s" % (out["n"], out["index"][:, 1].tolist()))
    np.savez_compressed(os.path.join(GOLD, "kitti_dataset.npz"), **out)


def gen_kitti_eigen_test_dataset():
    """the REAL KittiDepthMonoEigenTestDataset (mono_dataset.py:253-345) over the seeded tree of
    tests/helpers_kitti_eigen.py, once with depth_path among the config keys and once without"""
    import tempfile
    from tests import helpers_kitti_eigen as HE
    from monodepth.data.datasets.mono_dataset import KittiDepthMonoEigenTestDataset
    out = {}
    with tempfile.TemporaryDirectory() as d:
        raw, split = HE.make_eigen_tree(d)
        for with_depth, tag in ((True, "d"), (False, "n")):
            ds = KittiDepthMonoEigenTestDataset(**HE.eigen_cfg(raw, split, prefix='', with_depth=with_depth))
            out["n"] = len(ds)
            out["index"] = np.array([[o["index"], 0 if o["side"] == "l" else 1] for o in ds.imdb])
            for i in range(len(ds)):
                smp = ds[i]
                out["%s%d_keys" % (tag, i)] = np.array(sorted(repr(k) for k in smp))
                if with_depth:
                    out["d%d_sparse_depth" % i] = np.asarray(smp[("sparse_depth", 0)])
                    continue
                out["s%d_image_0" % i], out["s%d_image_m" % i] = npy(smp[("image", 0)]), npy(smp[("image", -1)])
                out["s%d_orig_0" % i] = npy(smp[("original_image", 0)])
                out["s%d_pose_m" % i] = np.asarray(smp[("relative_pose", -1)])
                out["s%d_P2" % i], out["s%d_original_P2" % i] = np.asarray(smp["P2"]), np.asarray(smp["original_P2"])
    print("kitti eigen test dataset: %d samples, (index, side) %s" % (out["n"], out["index"].tolist()))
    np.savez_compressed(os.path.join(GOLD, "kitti_eigen_test_dataset.npz"), **out)


def gen_supervised_eval():
    """the REAL compute_errors (kitti_supervised_eval.py:7-81; numba's jit is the identity shim, so the double loop runs
    as plain Python) on the seeded uint16 pairs of tests/helpers_supervised_eval.py, divided by 256 as evaluate_depth
    divides what cv2.imread returns"""
    from tests import helpers_supervised_eval as HS
    from monodepth.evaluation.kitti_supervised_eval import compute_errors
    out = {}
    for k, (H, W) in enumerate(HS.GOLDEN_SHAPES):
        gt, pred = HS.u16_pair(H, W, seed=100 + k)
        out["gt_%dx%d" % (H, W)], out["pred_%dx%d" % (H, W)] = gt, pred
        out["errors_%dx%d" % (H, W)] = np.asarray(compute_errors(gt / 256.0, pred / 256.0), np.float64)
        print("supervised eval %dx%d: %d valid, errors %s" % (H, W, int((gt / 256.0 > 0.01).sum()),
                                                               np.array2string(out["errors_%dx%d" % (H, W)], precision=4)))
    np.savez_compressed(os.path.join(GOLD, "supervised_eval.npz"), **out)


def gen_kitti360_fisheye():
    """the REAL KITTI360FisheyeDataset (fisheye_dataset.py:107-262) and Kitti360FisheyeEvaluator
    (kitti360_fisheye_eval.py:15-145) over the seeded fake KITTI-360 tree of tests/helpers_kitti360.py: filtered index
    lists, frames, P2 / original_P2 / calib_meta / patched_mask, relative poses (static filter on and off, left only
    and seeded right images), the ground-truth maps of _precompute (stored as flat indices + values) and _single_loss on
    seeded predictions.

    Repair 1: MeiCameraProjection.cam2image (mei_fisheye_utils.py:135-137) torch.stack-s the numpy arrays _cam2image
    returns for a numpy input and raises TypeError; here it is np.stack([x, y, z], -1) of the same three arrays.
    The dataset reads its fisheye mask from a hard-coded path (fisheye_dataset.py:161-163): the cv2 shim's imread
    serves the fixture mask for that path.  Both fixture conditions are asserted: every point with z > 0 projects
    inside the image, and no two points share the reference's float sub2ind value (so its duplicate search is idle)."""
    import hashlib
    import json
    import tempfile
    import cv2
    from tests import helpers_kitti360 as HK
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    from monodepth.data.datasets.fisheye_dataset import KITTI360FisheyeDataset
    from monodepth.networks.utils import mei_fisheye_utils as MU
    from monodepth.evaluation.kitti360_fisheye_eval import Kitti360FisheyeEvaluator
    MU.MeiCameraProjection.cam2image = lambda self, points, P, calib: np.stack(list(MU._cam2image(points, P, calib)), -1)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        raw, train, val, mask_path = HK.make_tree(d)
        imread = cv2.imread
        cv2.imread = lambda path, flags=1: imread(mask_path if path.endswith("kitti360_trainsub/fisheye_mask.png")
                                                  else path, flags)
        cases = dict(static_left=dict(is_filter_static=True, use_right_image=False, seed=None),
                     all_left=dict(is_filter_static=False, use_right_image=False, seed=None),
                     static_right=dict(is_filter_static=True, use_right_image=True, seed=3, fisheye_mask=mask_path))
        for tag, c in cases.items():
            kw = {k: v for k, v in c.items() if k != "seed"}
            ds = KITTI360FisheyeDataset(**HK.dataset_cfg(raw, train, prefix='', **kw))
            out[tag + "_index"] = np.array([o["img_indexes"] + o["pose_indexes"] for o in ds.imdb], np.int64)
            if c["seed"] is not None:
                np.random.seed(c["seed"])
            for i in range(len(ds)):
                smp = ds[i]
                k = "%s_s%d_" % (tag, i)
                for f in (0, -1, 1):
                    # the frames are random bytes: stored as the sha256 of the uint8 frame the reference normalised
                    img = npy(smp[("image", f)])
                    u8 = np.round((img.transpose(1, 2, 0) * std + mean) * 255).astype(np.uint8)
                    assert np.abs(((u8.astype(np.float32) / 255 - mean) / std).transpose(2, 0, 1) - img).max() < 1e-5
                    out[k + "image_%d" % f] = np.array(hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest())
                out[k + "pose_m"] = np.asarray(smp[("relative_pose", -1)])
                out[k + "pose_p"] = np.asarray(smp[("relative_pose", 1)])
                out[k + "P2"], out[k + "original_P2"] = npy(smp["P2"]), np.asarray(smp["original_P2"])
                out[k + "calib_meta"] = np.array(json.dumps(smp["calib_meta"], sort_keys=True))
                pm = smp["patched_mask"]
                out[k + "patched_mask"] = (npy(pm) if isinstance(pm, torch.Tensor) else np.asarray(pm)).astype(np.uint8)
        cv2.imread = imread
        # ground truth: the fixture conditions, then the real _precompute
        from monodepth.data.datasets.fisheye_dataset import read_fisheycalib, extract_P_from_fisheye_calib
        from monodepth.data.datasets.utils import read_pc_from_bin
        calib_dir = os.path.join(raw, "calibration")
        lc = read_fisheycalib(os.path.join(calib_dir, "image_02.yaml"))
        P0, T = extract_P_from_fisheye_calib(lc), HK.velo_to_cam02(calib_dir)
        for i in HK.EVAL_FRAMES:
            velo = read_pc_from_bin(os.path.join(raw, "data_3d_raw", HK.SEQ, "velodyne_points/data", "%010d.bin" % i))
            u, v, _, _ = HK.gt_points(velo, T, P0, lc)
            assert ((u >= 0) & (u < HK.W) & (v >= 0) & (v < HK.H)).all(), "fixture: a point with z > 0 leaves the image"
            assert HK.float_sub2ind_unique(velo, T, P0, lc), "fixture: two points share a float sub2ind value"
        gt_file = os.path.join(d, "gt.npz")
        ev = Kitti360FisheyeEvaluator(raw, val, gt_file)
        for j, (g, m) in enumerate(zip(ev.gt_depths, ev.close_masks)):
            out["gt%d_idx" % j], out["gt%d_val" % j], out["gt%d_midx" % j] = HK.sparse(g, m)
            want_g, want_m = HK.ground_truth(read_pc_from_bin(os.path.join(
                raw, "data_3d_raw", HK.SEQ, "velodyne_points/data", "%010d.bin" % HK.EVAL_FRAMES[j])), T, P0, lc)
            assert np.array_equal(want_g, g) and np.array_equal(want_m, m), "helper ground truth != reference"
        # _single_loss on seeded predictions (a smaller map: cv2.resize to the ground truth's size inside, routed to
        # the single-channel restatement of oracle/eval_oracle.py)
        from oracle import eval_oracle as EO
        resize = cv2.resize
        cv2.resize = lambda src, dsize, interpolation=cv2.INTER_LINEAR: (
            EO.cv2_resize_linear(src, dsize[0], dsize[1]) if np.ndim(src) == 2 and interpolation == cv2.INTER_LINEAR
            else resize(src, dsize, interpolation))
        rng = np.random.RandomState(17)
        for j in range(len(ev.gt_depths)):
            pred = (rng.rand(175, 175) * 30 + 0.5).astype(np.float32)
            r = ev._single_loss(pred.copy(), ev.gt_depths[j], ev.close_masks[j])
            out["pred%d" % j] = pred
            out["loss%d" % j] = np.concatenate([[r["ratio"]], r["error"], r["abs_error"]]).astype(np.float64)
        cv2.resize = resize
        out["n_gt"] = np.array(len(ev.gt_depths))
    print("kitti360 fisheye: %d / %d / %d samples, gt hits %s" % (
        len(out["static_left_index"]), len(out["all_left_index"]), len(out["static_right_index"]),
        [len(out["gt%d_idx" % j]) for j in range(int(out["n_gt"]))]))
    np.savez_compressed(os.path.join(GOLD, "kitti360_fisheye.npz"), **out)


def gen_kitti360_persp():
    """the REAL KITTI360MonoDataset (kitti360_dataset.py:85-220) and Kitti360Evaluator (kitti_unsupervised_eval.py:164-212,
    project_depth_map with its Counter loop) over the seeded tree of tests/helpers_kitti360_persp.py: the filtered index,
    relative poses / P2 / camera choice for a fixed seed, the ground-truth maps of _precompute (flat indices + values)
    and _single_loss on seeded predictions.  Fixture conditions, asserted and printed per frame: at least 1000 pixels
    hit by two or more points, at least one merged edge pair, and the host mirror (monodepth_utils.project_depth_map of
    this package) equal to the reference's maps with zero mismatching pixels."""
    import tempfile
    import cv2
    from tests import helpers_kitti360_persp as HP
    from monodepth.data.datasets.kitti360_dataset import KITTI360MonoDataset
    from monodepth.evaluation.kitti_unsupervised_eval import Kitti360Evaluator
    from fsnet_amd.monodepth.networks.utils.monodepth_utils import project_depth_map as host_project
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        raw, train, val = HP.make_tree(d)
        cases = dict(static_left=dict(is_filter_static=True, use_right_image=False, seed=None),
                     all_left=dict(is_filter_static=False, use_right_image=False, seed=None),
                     static_right=dict(is_filter_static=True, use_right_image=True, seed=HP.GOLDEN_DRAW_SEED))
        for tag, c in cases.items():
            kw = {k: v for k, v in c.items() if k != "seed"}
            ds = KITTI360MonoDataset(**HP.dataset_cfg(raw, train, prefix='', **kw))
            out[tag + "_index"] = np.array([o["img_indexes"] + o["pose_indexes"] for o in ds.imdb], np.int64)
            if c["seed"] is not None:
                np.random.seed(c["seed"])
            cams = []
            for i in range(len(ds)):
                smp = ds[i]
                k = "%s_s%d_" % (tag, i)
                # which camera the sample came from: the frame the reference normalised, against both PNGs on disk
                img = npy(smp[("image", 0)])
                u8 = np.round((img.transpose(1, 2, 0) * std + mean) * 255).astype(np.uint8)
                from PIL import Image
                match = [np.array_equal(u8, np.array(Image.open(os.path.join(
                    raw, "data_2d_raw", HP.SEQ, cam, "data_rect", "%010d.png" % ds.imdb[i]["img_indexes"][0]))))
                    for cam in ("image_00", "image_01")]
                assert sum(match) == 1
                cams.append(match.index(True))
                out[k + "pose_m"] = np.asarray(smp[("relative_pose", -1)])
                out[k + "pose_p"] = np.asarray(smp[("relative_pose", 1)])
                out[k + "P2"], out[k + "original_P2"] = npy(smp["P2"]), np.asarray(smp["original_P2"])
                pm = smp["patched_mask"]
                pm = npy(pm) if isinstance(pm, torch.Tensor) else np.asarray(pm)
                assert pm.shape == (HP.H, HP.W) and (pm == 1).all()
            out[tag + "_cam"] = np.array(cams, np.int64)
        gt_file = os.path.join(d, "gt.npz")
        ev = Kitti360Evaluator(raw, val, gt_file)
        P = ev.cam_calib['P0'] @ ev.cam_calib['R0'] @ np.linalg.inv(ev.cam_calib['T_cam2velo'])
        assert np.array_equal(P, HP.velo_to_image(raw))
        counts = []
        for j, g in enumerate(ev.gt_depths):
            scan = HP.scan(raw, HP.EVAL_FRAMES[j])
            dup, pairs = HP.fixture_counts(scan, P)
            mine = host_project(scan, P, np.array([HP.H, HP.W])).astype(np.float32)
            bad = int((mine != g).sum())
            counts.append((dup, pairs, bad))
            assert g.dtype == np.float32 and g.shape == (HP.H, HP.W)
            assert dup >= 1000 and pairs >= 1 and bad == 0, (j, dup, pairs, bad)
            out["gt%d_idx" % j], out["gt%d_val" % j] = HP.sparse(g)
            assert np.array_equal(HP.dense(out["gt%d_idx" % j], out["gt%d_val" % j]), g)
        from oracle import eval_oracle as EO
        resize = cv2.resize
        cv2.resize = lambda src, dsize, interpolation=cv2.INTER_LINEAR: (
            EO.cv2_resize_linear(src, dsize[0], dsize[1]) if np.ndim(src) == 2 and interpolation == cv2.INTER_LINEAR
            else resize(src, dsize, interpolation))
        rng = np.random.RandomState(19)
        for j in range(len(ev.gt_depths)):
            pred = (rng.rand(47, 155) * 30 + 0.5).astype(np.float32)
            r = ev._single_loss(pred.copy(), ev.gt_depths[j])
            out["pred%d" % j] = pred
            out["loss%d" % j] = np.concatenate([[r["ratio"]], r["error"], r["abs_error"]]).astype(np.float64)
        cv2.resize = resize
        out["n_gt"] = np.array(len(ev.gt_depths))
    print("kitti360 perspective: %d / %d / %d samples, cameras %s" % (
        len(out["static_left_index"]), len(out["all_left_index"]), len(out["static_right_index"]),
        out["static_right_cam"].tolist()))
    for j, (dup, pairs, bad) in enumerate(counts):
        print("  frame %d: %d pixels hit twice or more, %d merged edge pairs, %d pixels where the host mirror differs "
              "from the reference, %d pixels hit" % (j, dup, pairs, bad, len(out["gt%d_idx" % j])))
    np.savez_compressed(os.path.join(GOLD, "kitti360_persp.npz"), **out)


def gen_nusc():
    """the REAL NusceneJsonDataset / NusceneDepthMonoDataset / NusceneSweepDepthMonoDataset (nuscene_dataset.py:14-238),
    NuscenesEvaluator._precompute and _single_loss (nuscenes_unsupervised_eval.py:17-255) and FastNuscEvaluationHook
    (base_evaluation_hooks.py:141-202) over the seeded tree of tests/helpers_nusc.py, with the devkit and pyquaternion
    stand-ins of tools/ref_shims (this project's reading of the two packages, not pinned against the real ones).
    The reference's generate_depth_map uses np.int, which NumPy 2 removed: set for this run.  Fixture conditions,
    asserted: per sample at least one exact .5 tie, one merged edge pair and 100 pixels hit twice or more in
    CAM_FRONT, and this package's explicit-order mirror equal to the reference's PNGs with zero differing pixels."""
    import tempfile
    import warnings
    import cv2
    from tests import helpers_nusc as HN
    from oracle import eval_oracle as EO
    np.int = int
    import monodepth.evaluation.nuscenes_unsupervised_eval as RE
    from monodepth.data.datasets.nuscene_dataset import (NusceneDepthMonoDataset, NusceneJsonDataset,
                                                         NusceneSweepDepthMonoDataset)
    from monodepth.pipeline_hooks.evaluation_hooks.base_evaluation_hooks import FastNuscEvaluationHook
    from vision_base.data.datasets.nuscenes_utils import NuScenes
    from fsnet_amd.monodepth.data.datasets.utils import read_png16
    from fsnet_amd.monodepth.evaluation import nuscenes_unsupervised_eval as ME
    out = {}
    resize = cv2.resize
    cv2.resize = lambda src, dsize, interpolation=cv2.INTER_LINEAR: (
        EO.cv2_resize_linear(src, dsize[0], dsize[1]) if np.ndim(src) == 2 and interpolation == cv2.INTER_LINEAR
        else resize(src, dsize, interpolation))
    with tempfile.TemporaryDirectory() as d:
        tree = HN.make_tree(d)
        nusc = NuScenes(version=HN.VERSION, dataroot=tree["dataroot"], verbose=False)
        resolved = []
        get = nusc.get
        nusc.get = lambda table, token: (resolved.append((table, token)), get(table, token))[1]
        # ---- datasets ------------------------------------------------------------------------------------------
        ds = NusceneJsonDataset(json_path=tree["json_train"], augmentation=HN.raw_augmentation(''))
        out["json_n"] = np.array(len(ds))
        for i in range(len(ds)):
            out["json_keys"] = np.array(HN.flatten_sample(ds[i], "json%d_" % i, out))
        val = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                                 augmentation=HN.raw_augmentation(''))
        out["jsonval_keys"] = np.array(HN.flatten_sample(val[3], "jsonval3_", out))
        tall = NusceneJsonDataset(json_path=tree["json_tall"], image_keys=['frame0'], frame_ids=[0],
                                  augmentation=HN.raw_augmentation(''))
        for i in range(2):
            pm = tall[i]["patched_mask"]
            assert pm.dtype == np.float64 and pm.shape == (HN.TALL_H, HN.TALL_W)
            out["tall%d_mask_rows" % i] = pm.min(1)
        assert out["tall0_mask_rows"][700:].max() == 0 and out["tall0_mask_rows"][:700].min() == 1
        assert out["tall1_mask_rows"].min() == 1
        for tag, cls in (("mono", NusceneDepthMonoDataset), ("sweep", NusceneSweepDepthMonoDataset)):
            for filt in (False, True):
                t = NusceneDepthMonoDataset.__init__
                dsm = cls(split_file=tree["split"], nuscenes_version=HN.VERSION, nuscenes_dir=tree["dataroot"],
                          is_filter_static=filt, filter_threshold=1.1005 if filt else 0.03,
                          augmentation=HN.raw_augmentation(''))
                assert dsm.nusc is nusc and t is NusceneDepthMonoDataset.__init__
                np.random.seed(5)
                k = "%s%d" % (tag, int(filt))
                out[k + "_n"] = np.array(len(dsm))
                for i in range(len(dsm)):
                    out[k + "_keys"] = np.array(HN.flatten_sample(dsm[i], "%s_%d_" % (k, i), out, digest_frames=True))
        # ---- ground-truth export ---------------------------------------------------------------------------------
        f64_maps = []
        ref_gdm = RE.generate_depth_map
        RE.generate_depth_map = lambda *a, **k: (f64_maps.append(ref_gdm(*a, **k)), f64_maps[-1])[1]
        gt_dir = os.path.join(d, "samples_depth_gt")
        ev = RE.NuscenesEvaluator(tree["dataroot"], tree["split"], gt_dir, nuscenes_version=HN.VERSION)
        RE.generate_depth_map = ref_gdm
        out["gt_f64"] = np.array(f64_maps).reshape(len(HN.EVAL), len(HN.CAMS), HN.H, HN.W)
        pngs, stats = [], []
        for j, i in enumerate(HN.EVAL):
            rec = get('sample', 'sample_%d' % i)
            lidar_data, lidar_mask = ME.get_lidar(nusc, rec)
            ref_data, ref_mask = RE.get_lidar(nusc, rec)
            assert np.array_equal(lidar_data, ref_data) and np.array_equal(lidar_mask, ref_mask)
            lidar = lidar_data[lidar_mask == 1, :]
            planes = []
            for c, cam in enumerate(HN.CAMS):
                samp = get('sample_data', rec['data'][cam])
                png = read_png16(samp['filename'].replace('samples', gt_dir).replace('.jpg', '.png'))
                sens = get('calibrated_sensor', samp['calibrated_sensor_token'])
                T = ME.camera_extrinsics(sens)
                M = ME.projection_matrix(T, np.array(sens['camera_intrinsic']))[:3]
                mine = ME.nusc_depth_u16(lidar, M, [HN.H, HN.W])
                bad = int((mine != png).sum())
                bad64 = int((ME.generate_depth_map(lidar, T, np.array(sens['camera_intrinsic']),
                                                   im_shape=[HN.H, HN.W]) != out["gt_f64"][j, c]).sum())
                assert png.dtype == np.uint16 and bad == 0 and bad64 == 0, (i, cam, bad, bad64)
                planes.append(png)
                if cam == 'CAM_FRONT':
                    x, y, z = (lidar[:, k].astype(np.float64) for k in range(3))
                    p = [M[k, 0] * x + M[k, 1] * y + M[k, 2] * z + M[k, 3] for k in range(3)]
                    keep = p[2] > 0
                    u, v = p[0][keep] / p[2][keep], p[1][keep] / p[2][keep]
                    col, row = np.rint(u) - 1, np.rint(v) - 1
                    ok = (col >= 0) & (row >= 0) & (col < HN.W) & (row < HN.H)
                    hits = np.bincount((row[ok] * HN.W + col[ok]).astype(np.int64), minlength=HN.H * HN.W).reshape(HN.H, HN.W)
                    ties = int((((u[ok] % 1) == 0.5) | ((v[ok] % 1) == 0.5)).sum())
                    pairs = int(((hits[:-1, HN.W - 1] > 0) & (hits[1:, 0] > 0)).sum())
                    stats.append((ties, pairs, int((hits >= 2).sum()), int(keep.sum()), int((~keep).sum())))
                    assert ties >= 7 and pairs >= 2 and stats[-1][2] >= 100 and stats[-1][4] > 0, stats[-1]
            pngs.append(planes)
        out["gt_png"] = np.array(pngs)
        # ---- _single_loss ------------------------------------------------------------------------------------------
        rng = np.random.RandomState(31)
        preds, losses = [], []
        for j in range(len(HN.EVAL)):
            for c in range(len(HN.CAMS)):
                pred = (rng.rand(13, 21) * 30 + 0.5).astype(np.float32)
                r = ev._single_loss(pred.copy(), (out["gt_png"][j, c] / 256.0).astype(np.float32))
                preds.append(pred)
                losses.append(np.concatenate([[r["ratio"]], r["error"], r["abs_error"]]).astype(np.float64))
        out["loss_pred"], out["loss"] = np.array(preds), np.array(losses)
        try:
            ev._single_loss(np.ones((13, 21), np.float32), np.zeros((HN.H, HN.W), np.float32))
            raise AssertionError("the empty valid set must raise")
        except ValueError:
            pass
        # ---- FastNuscEvaluationHook with a fixed-weight model ---------------------------------------------------------
        h, w = 64, 128
        m = ref_model(h, w, with_pose=False)
        m.load_state_dict(O.init_state(seed=2, with_pose=False), strict=True)
        logged = []
        hook = FastNuscEvaluationHook(
            test_run_hook_cfg=dict(name='vision_base.pipeline_hooks.train_val_hooks.base_validation_hooks.BaseValidationHook'),
            dataset_eval_cfg=dict(name='monodepth.evaluation.nuscenes_unsupervised_eval.NuscenesEvaluator',
                                  data_path=tree["dataroot"], split_file=tree["split"], gt_saved_dir=gt_dir,
                                  nuscenes_version=HN.VERSION),
            batch_size=5, num_workers=0)
        hook.dataset_eval_func.log = lambda writer, channel, me, mae, **k: logged.append((channel, me, mae))
        vds = NusceneJsonDataset(json_path=tree["json_val"], image_keys=['frame0'], frame_ids=[0],
                                 augmentation=HN.val_augmentation('', h, w))
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # no sample of the tree is without usable points
            hook(m, vds)
        assert [l[0] for l in logged] == HN.CAMS + ['all mean']
        out["hook_errors"] = np.array([l[1] for l in logged], np.float64)
        out["hook_abs_errors"] = np.array([l[2] for l in logged], np.float64)
        out["hook_hw"] = np.array([h, w])
        tables = sorted(set(resolved))
        out["resolved_tables"] = np.array([t for t, _ in tables])
        out["resolved_tokens"] = np.array([t for _, t in tables])
    cv2.resize = resize
    print("nusc: %d json samples, %d tokens resolved; CAM_FRONT per sample (ties, merged edge pairs, pixels hit twice or "
          "more, points in front, points behind): %s" % (int(out["json_n"]), len(tables), stats))
    print("  hook all-mean errors", out["hook_errors"][-1])
    np.savez_compressed(os.path.join(GOLD, "nusc_eval.npz"), **out)


def gen_loss_options():
    """optional terms of MonoDepth2Decoder.loss no shipped config enables: precomputed motion_mask
    (monodepth2_decoder.py:243-246) and the pose L1 term (:176-183, 322-326), from the REAL decoder"""
    B, H, W = 2, 64, 96
    data = O.synthetic_batch(B, H, W, seed=41)
    g = torch.Generator().manual_seed(8)
    mm = (torch.rand(B, H // 8, W // 8, generator=g) > 0.6).float()
    data["motion_mask"] = torch.nn.functional.interpolate(mm[:, None], size=(H, W), mode="nearest")[:, 0]   # blocky 0/1
    dec = ref_model(H, W, True).head
    dec.pose_loss_weight = 0.5
    outputs, leaves = {}, {}
    for s in range(4):
        h, w = H >> s, W >> s
        ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
        d = (4 + 25 * (1 - ys) + 3 * torch.rand(B, 1, h, w, generator=g)).requires_grad_(True)
        leaves[("depth", s)] = d
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        aa = (0.01 * torch.randn(B, 1, 3, generator=g)).requires_grad_(True)
        tr = (torch.tensor([[[0.02, -0.01, -0.6 if f > 0 else 0.6]]]).repeat(B, 1, 1) + 0.02 * torch.randn(B, 1, 3, generator=g)).requires_grad_(True)
        leaves[("aa", f)], leaves[("tr", f)] = aa, tr
        outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
    res = dec.loss(outputs, data)
    res['loss'].backward()
    out = {"H": H, "W": W, "seed": 41, "pose_loss_weight": 0.5, "total_loss": npy(res['loss']), "motion_mask": npy(data["motion_mask"])}
    for k, v in res['loss_dict'].items():
        out["ld_" + k.replace('/', '_')] = npy(v)
    for s in range(4):
        out["depth_%d" % s] = npy(leaves[("depth", s)])
        out["gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
    for f in (1, -1):
        tag = "p" if f > 0 else "m"
        out["aa_" + tag], out["tr_" + tag] = npy(leaves[("aa", f)]), npy(leaves[("tr", f)])
        out["gaa_" + tag], out["gtr_" + tag] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
        out["pose_" + tag] = npy(data[("relative_pose", f)])
    # oracle cross-check
    o2, lv = {}, {}
    for s in range(4):
        d = leaves[("depth", s)].detach().clone().requires_grad_(True); lv[s] = d
        o2[("depth", s, s)] = d; o2[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        o2[("cam_T_cam", f)] = outputs[("cam_T_cam", f)].detach()
    tot, ld = O.photometric_loss(o2, data)
    pl = sum((data[("relative_pose", f)] - o2[("cam_T_cam", f)]).abs().mean() for f in (1, -1))
    (tot + 0.5 * pl).backward()
    print("loss options: ref total %.9f oracle %.9f | gdepth0 rel dev %.2e" % (
        float(res['loss']), float(tot + 0.5 * pl),
        dev(lv[0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max())))
    np.savez_compressed(os.path.join(GOLD, "loss_options.npz"), **out)


def no_overlap_case(H=64, W=96, B=2, seed=43):
    """inputs of the overlapped_mask=False golden: large translations, so that a good part of the samples leaves the
    source frames (those are exactly the pixels the option changes)"""
    data = O.synthetic_batch(B, H, W, seed=seed)
    g = torch.Generator().manual_seed(18)
    depths = []
    for s in range(4):
        h, w = H >> s, W >> s
        ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
        depths.append(4 + 25 * (1 - ys) + 3 * torch.rand(B, 1, h, w, generator=g))
    poses = {}
    for f in (1, -1):
        aa = 0.03 * torch.randn(B, 1, 3, generator=g)
        tr = torch.tensor([[[0.9 if f > 0 else -0.9, -0.05, -0.8 if f > 0 else 0.8]]]).repeat(B, 1, 1) + 0.02 * torch.randn(B, 1, 3, generator=g)
        poses[f] = (aa, tr)
    return data, depths, poses


def gen_no_overlap_mask():
    """MonoDepth2Decoder.loss with overlapped_mask=False (configs/multi_dataset_example, nusc_wpose_example;
    monodepth2_decoder.py:110-116, 230-235) from the REAL decoder: totals, depth and pose gradients"""
    H, W = 64, 96
    data, depths, poses = no_overlap_case(H, W)
    dec = ref_model(H, W, True).head
    dec.overlapped_mask = False
    outputs, leaves = {}, {}
    for s in range(4):
        d = depths[s].clone().requires_grad_(True)
        leaves[("depth", s)] = d
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = mu.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        aa, tr = poses[f][0].clone().requires_grad_(True), poses[f][1].clone().requires_grad_(True)
        leaves[("aa", f)], leaves[("tr", f)] = aa, tr
        outputs[("cam_T_cam", f)] = mu.transformation_from_parameters(aa, tr, invert=(f < 0))
    torch.manual_seed(0)
    res = dec.loss(outputs, data)
    res['loss'].backward()
    assert not any(k[0] == "overlapped_mask" for k in outputs)
    out = {"H": H, "W": W, "total_loss": npy(res['loss'])}
    for k, v in res['loss_dict'].items():
        out["ld_" + k.replace('/', '_')] = npy(v)
    for s in range(4):
        out["gdepth_%d" % s] = npy(leaves[("depth", s)].grad)
    for f in (1, -1):
        tag = "p" if f > 0 else "m"
        out["gaa_" + tag], out["gtr_" + tag] = npy(leaves[("aa", f)].grad), npy(leaves[("tr", f)].grad)
    # how much the option matters on this case: the same inputs with the mask on
    dec.overlapped_mask = True
    o_on = {k: v.detach() for k, v in outputs.items() if k[0] in ("depth", "disp", "cam_T_cam")}
    torch.manual_seed(0)
    on = dec.loss(o_on, data)
    out["total_loss_masked"] = npy(on['loss'])
    out["outside_frac"] = np.float64(1.0 - float(torch.stack([o_on[("overlapped_mask", f, 0)].float().mean() for f in (1, -1)]).mean()))
    o2, lv = {}, {}
    for s in range(4):
        d = depths[s].clone().requires_grad_(True); lv[s] = d
        o2[("depth", s, s)] = d; o2[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        o2[("cam_T_cam", f)] = outputs[("cam_T_cam", f)].detach()
    tot, ld = O.photometric_loss(o2, data, overlapped_mask=False)
    tot.backward()
    print("no overlap mask: ref total %.9f (masked %.9f, %.1f %% of the samples outside) oracle %.9f | gdepth0 rel dev %.2e" % (
        float(res['loss']), float(on['loss']), 100 * float(out["outside_frac"]), float(tot),
        dev(lv[0].grad, leaves[("depth", 0)].grad) / float(leaves[("depth", 0)].grad.abs().max())))
    np.savez_compressed(os.path.join(GOLD, "no_overlap_mask.npz"), **out)


def thin(t, limit=4096):
    """every k-th element of the flattened tensor (k = the smallest stride that leaves <= `limit` values), float32;
    tests apply the same rule to what they compare"""
    a = t.detach().reshape(-1)
    k = max(1, -(-a.numel() // limit))
    return a[::k].to(torch.float32).numpy().copy()


def sigmoid_decoder_case():
    """seeded inputs of the sigmoid-disparity DepthDecoder golden (shared with tests/)"""
    g = torch.Generator().manual_seed(77)
    B, H, W = 2, 64, 128
    chans = [64, 64, 128, 256, 512]
    feats = [torch.randn(B, c, H >> (k + 1), W >> (k + 1), generator=g) * 0.5 for k, c in enumerate(chans)]
    sd = {k[len("head.depth_decoder."):]: v for k, v in O.init_state(seed=9, with_pose=False, num_out=1).items()
          if k.startswith("head.depth_decoder.")}
    P2 = torch.tensor([[[700.0, 0, 64, 0], [0, 700, 32, 0], [0, 0, 1, 0]], [[540.0, 0, 60, 0], [0, 540, 30, 0], [0, 0, 1, 0]]])
    wd = [torch.randn(B, 1, H >> s, W >> s, generator=g) for s in range(4)]
    wq = [torch.randn(B, 1, H >> s, W >> s, generator=g) for s in range(4)]
    return feats, sd, P2, wd, wq


def gen_sigmoid_decoder():
    """The base-class DepthDecoder (sigmoid disparity, depth_encoder.py:17-111) with and without base_fx: outputs,
    feature gradients and parameter-gradient norms of sum_s <depth_s, wd_s> * 1e-2 + <disp_s, wq_s>."""
    from monodepth.networks.models.heads.depth_encoder import DepthDecoder
    feats, sd, P2, wd, wq = sigmoid_decoder_case()
    out = {}
    for tag, base_fx in (("plain", None), ("fx", 600.0)):
        m = DepthDecoder(num_ch_enc=np.array([64, 64, 128, 256, 512]), scales=[0, 1, 2, 3], num_output_channels=1,
                         use_skips=True, min_depth=0.5, max_depth=100, base_fx=base_fx)
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        m.train()
        fl = [f.clone().requires_grad_(True) for f in feats]
        res = m(fl, P2 if base_fx is not None else None)
        loss = sum((res[("depth", s, s)] * wd[s]).sum() * 1e-2 + (res[("disp", s)] * wq[s]).sum() for s in range(4))
        loss.backward()
        o = O.depth_decoder_forward({("d." + k): v for k, v in sd.items()}, "d.", [f.clone() for f in feats], 0.5, 100.0,
                                    P2=P2 if base_fx is not None else None, base_fx=base_fx, sigmoid=True)
        print("sigmoid decoder [%s]: oracle depth dev %.2e disp dev %.2e" % (
            tag, dev(o[("depth", 0, 0)], res[("depth", 0, 0)]), dev(o[("disp", 0)], res[("disp", 0)])))
        out[tag + "_loss"] = npy(loss)
        for s in range(4):
            out["%s_depth%d" % (tag, s)] = thin(res[("depth", s, s)])
            out["%s_disp%d" % (tag, s)] = thin(res[("disp", s)])
        for k, f in enumerate(fl):
            out["%s_gfeat%d" % (tag, k)] = thin(f.grad)
        out[tag + "_gnorm"] = npy(torch.stack([p.grad.norm() for p in m.parameters()]))
    np.savez_compressed(os.path.join(GOLD, "sigmoid_decoder.npz"), **out)


def gen_frozen():
    """ResNet.train() with frozen_stages / norm_eval (resnet.py:169-197) inside the training step of the reference's
    own hook: 3 Adam steps of the dataset-pose meta-arch, with (a) stem + layer1 frozen, (b) every BatchNorm in eval
    mode.  Losses, gradient norms, parameter sums per step, final running statistics."""
    from vision_base.pipeline_hooks.train_val_hooks.base_training_hooks import BaseTrainingHook
    B, H, W = 2, 64, 128
    out = {}
    for tag, fs, ne in (("fs1", 1, False), ("ne", -1, True)):
        sd0 = O.init_state(seed=3, with_pose=False)
        # running statistics away from (0, 1): an eval-mode BatchNorm must really use them
        g = torch.Generator().manual_seed(5)
        for k in sd0:
            if k.endswith("running_mean"):
                sd0[k] = 0.1 * torch.randn(sd0[k].shape, generator=g)
            elif k.endswith("running_var"):
                sd0[k] = 0.5 + torch.rand(sd0[k].shape, generator=g)
        m = ref_model(H, W, False, frozen_stages=fs, norm_eval=ne)
        m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        hook = BaseTrainingHook(clip_gradients=35.0)
        tr = O.OracleTrainer(sd0, with_pose=False, frozen_stages=fs, norm_eval=ne)
        for it in range(3):
            data = O.synthetic_batch(B, H, W, seed=300 + it)
            # the hook's body (base_training_hooks.py:30-49) without its .cuda() calls
            opt.zero_grad()
            torch.manual_seed(0)
            res = m(dict(data), dict(is_training=True))
            res['loss'].mean().backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), hook.clip_gradients)
            opt.step()
            out["%s_loss_%d" % (tag, it)] = npy(res['loss'])
            out["%s_psum_%d" % (tag, it)] = npy(torch.stack([p.double().sum() for p in m.parameters()]))
            tot, ld, o_out, raw, norm = tr.step(data)
            print("[frozen %s] step %d: ref loss %.9f oracle %.9f" % (tag, it, float(res['loss']), float(tot)))
        sd_ref = m.state_dict()
        print("[frozen %s] max param dev oracle vs ref %.3e; running_mean dev %.3e; trainable %d of %d" % (
            tag, max(dev(tr.sd[k], sd_ref[k]) for k in tr.names),
            max(dev(tr.sd[k], sd_ref[k]) for k in sd_ref if k.endswith('running_mean')),
            sum(p.requires_grad for p in m.parameters()), len(list(m.parameters()))))
        out[tag + "_rm_final"] = npy(torch.cat([sd_ref[k].flatten() for k in sd_ref if k.endswith('running_mean')]))
        out[tag + "_rv_final"] = npy(torch.cat([sd_ref[k].flatten() for k in sd_ref if k.endswith('running_var')]))
        out[tag + "_nbt_final"] = npy(torch.stack([sd_ref[k] for k in sd_ref if k.endswith('num_batches_tracked')]))
    np.savez_compressed(os.path.join(GOLD, "frozen.npz"), **out)


def gen_concat():
    """vision_base ConcatDataset over three tiny children: which (child, local index) every global index maps to,
    and how common keywords / per-child overrides reach the children"""
    import json
    from vision_base.data.datasets.dataset_utils import ConcatDataset
    cfgs = [dict(name="tiny_ds.Tiny", n=5, tag="a"), dict(name="tiny_ds.Tiny", n=3, tag="b", scale=10),
            dict(name="tiny_ds.Tiny", n=7, tag="c")]
    ds = ConcatDataset([EasyDict(c) for c in cfgs], scale=2)
    rec = dict(cfgs=cfgs, common=dict(scale=2), length=int(len(ds)), items=[{k: (int(v) if k == "value" else v) for k, v in ds[i].items()} for i in range(len(ds))])
    json.dump(rec, open(os.path.join(GOLD, "concat_dataset.json"), "w"))
    print("concat dataset: %d items" % len(ds))


def gen_velo_gt():
    """KITTI ground-truth export (monodepth_utils.py:368-420 generate_depth_map, with its sub2ind quirk) over the seeded
    on-disk tree of tests/helpers_kitti.py: the reference's depth maps for the split's frames"""
    import tempfile
    if not hasattr(np, "int"):
        np.int = int
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers_kitti as HK
    from monodepth.networks.utils.monodepth_utils import generate_depth_map
    with tempfile.TemporaryDirectory() as d:
        raw, split = HK.make_tree(d)
        HK.add_velodyne(raw)
        gts = []
        for line in open(split):
            folder, frame_id, _ = line.split()
            gts.append(generate_depth_map(os.path.join(raw, folder.split("/")[0]),
                                          os.path.join(raw, folder, "velodyne_points/data", "%010d.bin" % int(frame_id)), 2, True))
    gts = np.array(gts)
    print("velodyne gt: %s, %.1f %% of the pixels hit, depth range %.2f..%.2f" % (
        gts.shape, 100 * float((gts > 0).mean()), float(gts[gts > 0].min()), float(gts.max())))
    np.savez_compressed(os.path.join(GOLD, "velo_gt.npz"), gt=gts)


def gen_teacher_keys():
    """monodepth/transform_teacher.py on a checkpoint of the reference depth+pose meta-arch: the key list of the
    teacher state_dict (order included) and a checksum per kept tensor."""
    import json
    import tempfile
    from monodepth.transform_teacher import transform_teacher_model
    m = ref_model(64, 128, True)
    m.load_state_dict({k: v.clone() for k, v in O.init_state(seed=1, with_pose=True).items()}, strict=True)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "stage1.pth"), os.path.join(d, "teacher.pth")
        torch.save({"model_state_dict": m.state_dict(), "optimizer_state_dict": {}}, src)
        transform_teacher_model(src, dst)
        out = torch.load(dst, map_location="cpu")
    rec = {"src_keys": list(m.state_dict().keys()), "dst_keys": list(out.keys()),
           "dst_sums": [float(v.double().sum()) for v in out.values()], "is_bare_state_dict": isinstance(out, dict)
           and "model_state_dict" not in out}
    json.dump(rec, open(os.path.join(GOLD, "teacher_keys.json"), "w"))
    print("teacher keys: %d of %d kept" % (len(rec["dst_keys"]), len(rec["src_keys"])))


def gen_onnx():
    """scripts/onnx_export.py:39-52 on the real MonoDepthWPose (CPU, eval mode): `dummy_forward(image)` and the
    reference's own `torch.onnx.export(..., opset_version=11)` of it — operator histogram, graph input / output
    signature and initializer shapes of the file the reference writes (read back with the wire-format reader; the
    `onnx` package is absent, so the exporter's onnxscript splice is skipped — see fsnet_amd/export/onnx_graph.py)."""
    import collections
    import io
    import json
    import warnings
    from fsnet_amd.export import onnx_graph as G
    from tests.helpers_onnx import case as onnx_case
    sd0, image = onnx_case()
    m = ref_model(64, 128, False)
    m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    m.eval()
    with torch.no_grad():
        pred = m.dummy_forward(image)
    assert list(pred.keys()) == ["depth"]
    m.forward = m.dummy_forward
    f = io.BytesIO()
    with warnings.catch_warnings(), G._without_onnx_package():
        warnings.simplefilter("ignore")
        torch.onnx.export(m, torch.zeros(1, 3, 64, 128), f, input_names=['input'], output_names=['output'],
                          opset_version=11, dynamo=False)
    model = G.read_model(f)
    G.check_model(model)
    g = model["graph"]
    rec = {"ir_version": model["ir_version"], "opsets": model["opsets"],
           "ops": dict(collections.Counter(n["op_type"] for n in g["nodes"])),
           "inputs": [v for v in g["inputs"] if v["name"] not in g["initializers"]],
           "outputs": [dict(name=v["name"], elem_type=v["elem_type"], rank=len(v["shape"])) for v in g["outputs"]],
           "initializer_shapes": sorted([list(a.shape) for a in g["initializers"].values()]),
           "n_bytes": len(f.getvalue())}
    json.dump(rec, open(os.path.join(GOLD, "onnx_graph.json"), "w"), indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(GOLD, "onnx_dummy_forward.npz"), depth=npy(pred["depth"]))
    print("onnx: %d nodes, %d initializers, depth range %.3f..%.3f" % (
        len(g["nodes"]), len(g["initializers"]), float(pred["depth"].min()), float(pred["depth"].max())))


def gen_postopt():
    """sparse-VO depth post-optimisation through the REAL reference post_optimization (postopt_utils.py:170-226) on
    CPU, with the skimage shim's rgb2lab; its own SLIC is wrapped to record labels (compacted to the non-empty
    segments, in index order) and centres.  The reference leaves the order of top-k ties open, so the VO points carry
    noise (distinct |log pred - log vo|).  (a) 96x320 at the hook defaults with > max_points valid VO points (the
    top-k branch); (b) 64x200 at the function defaults with fewer."""
    import time
    from monodepth.networks.utils import postopt_utils as PU
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers_postopt as HP
    rec = {}
    slic0 = PU.SLIC

    def slic_rec(*a, **k):
        centers, segments = slic0(*a, **k)
        H, W = a[0].shape[:2]
        lab = np.full((H, W), -1, np.int16)
        for i, s in enumerate(segments):
            lab[s[:, 0].numpy(), s[:, 1].numpy()] = i
        rec["labels"], rec["centres"] = lab, npy(centers).T.astype(np.float32)
        return centers, segments
    PU.SLIC = slic_rec
    out = {}
    cases = {"a": (96, 320, 21, 0.03, dict(HP.HOOK_DEFAULTS), 800),
             "b": (64, 200, 22, 0.02, dict(HP.FUNCTION_DEFAULTS, h_seg=6, w_seg=10), 800)}
    for tag, (H, W, seed, frac, params, max_points) in cases.items():
        image, _, pred, vo = HP.synthetic_scene(H, W, seed, vo_frac=frac, vo_noise=0.05)   # no top-k ties
        rgb = PU.denorm(image.transpose(1, 2, 0), rgb_mean=np.array([0.485, 0.456, 0.406]),
                        rgb_std=np.array([0.229, 0.224, 0.225]))
        t0 = time.time()
        ref = PU.post_optimization(rgb, PU.depth_image_to_point_cloud_array(pred), torch.from_numpy(pred), vo,
                                   max_points=max_points, **params)
        n_valid = int(((vo > 3) & (vo < 80)).sum())
        print("postopt %s: %dx%d, %d valid VO points, %d segments, %.1f s" % (
            tag, H, W, n_valid, rec["centres"].shape[0], time.time() - t0))
        mine, seg, centres, _, _ = HP.post_optimize(image, pred, vo, max_points=max_points, details=True, **params)
        print("  restatement: labels equal on %.5f, max rel depth dev %.3e" % (
            float((seg.numpy() == rec["labels"]).mean()), float((mine / ref - 1).abs().max())))
        out.update({"%s_image" % tag: image, "%s_depth" % tag: pred, "%s_vo" % tag: vo,
                    "%s_labels" % tag: rec["labels"], "%s_centres" % tag: rec["centres"],
                    "%s_refined" % tag: npy(ref).astype(np.float32),
                    "%s_params" % tag: np.array([H, W, params["h_seg"], params["w_seg"], params["iter_num"],
                                                 params["lambda0"], params["lambda1"], params["lambda2"],
                                                 max_points], np.float64)})
    PU.SLIC = slic0
    np.savez_compressed(os.path.join(GOLD, "postopt.npz"), **out)


def gen_motion_mask():
    """the REAL MotionMaskPrecomputeHook and MotionMaskARFlowPrecomputeHook (base_precompute_hooks.py:27-148) over a
    helpers_kitti.make_tree tree of 96x320 frames (two pyramid levels), on CPU (Tensor.cuda is a no-op here), with
    the cv2 shim's calcOpticalFlowFarneback (= the restatement of tests/helpers_optflow.py), BGR2GRAY, imwrite and
    imread.  The ARFlow hook reads seeded flow PNGs through the REAL dataset (is_precompute_flow).  Records the written
    files (names and masks), the samples' P2 / original_P2 / relative poses, and a checksum of the Farneback flows;
    the frames and flow files are regenerated from their seeds by the test."""
    import tempfile
    from PIL import Image
    from tests import helpers_kitti as HK
    from tests import helpers_optflow as HO
    from monodepth.pipeline_hooks.precomputing_hooks.base_precompute_hooks import (
        MotionMaskARFlowPrecomputeHook, MotionMaskPrecomputeHook)
    H, W = HO.GOLDEN_HW
    out = {}
    with tempfile.TemporaryDirectory() as d:
        raw, split = HK.make_tree(d, seed=HO.GOLDEN_TREE_SEED, H=H, W=W)
        cfg = HO.raw_dataset_cfg(raw, split, prefix='')
        for tag, fcfg in (("box", HO.GOLDEN_FLOW_CFG), ("gauss", HO.GOLDEN_FLOW_CFG_G)):
            odir = os.path.join(d, "mm_" + tag)
            os.makedirs(odir)
            hook = MotionMaskPrecomputeHook(cfg, fcfg, distance_threshold=HO.GOLDEN_THR[0], output_dir=odir)
            hook()
            names = sorted(os.listdir(odir))
            out["%s_names" % tag] = np.array(names)
            out["%s_masks" % tag] = np.stack([np.array(Image.open(os.path.join(odir, f))) for f in names])
            sums = []
            for i in range(len(hook.dataset)):
                smp = hook.dataset[i]
                g0, g1 = HO.gray(smp[("image", 0)]), HO.gray(smp[("image", 1)])
                sums.append(float(np.abs(HO.farneback(g0, g1, **fcfg)).astype(np.float64).sum()))
            out["%s_flow_abs_sum" % tag] = np.array(sums)
        n = len(hook.dataset)
        for i in range(n):
            smp = hook.dataset[i]
            out["s%d_P2" % i] = np.asarray(smp["P2"], np.float64)
            out["s%d_original_P2" % i] = np.asarray(smp["original_P2"], np.float64)
            out["s%d_pose" % i] = np.asarray(smp[("relative_pose", 1)])
        fdir = os.path.join(d, "flow")
        HO.write_flow_pngs(fdir, n, H, W)
        acfg = dict(cfg, is_precompute_flow=True, flow_path=fdir)
        odir = os.path.join(d, "mm_arflow")
        os.makedirs(odir)
        MotionMaskARFlowPrecomputeHook(acfg, {}, distance_threshold=HO.GOLDEN_THR[1], output_dir=odir)()
        names = sorted(os.listdir(odir))
        out["arflow_names"] = np.array(names)
        out["arflow_masks"] = np.stack([np.array(Image.open(os.path.join(odir, f))) for f in names])
    out["n"] = np.int64(n)
    for tag in ("box", "gauss", "arflow"):
        print("motion mask %s: %d files, %.4f of the pixels masked" % (tag, len(out[tag + "_names"]),
                                                                        float(out[tag + "_masks"].mean())))
    np.savez_compressed(os.path.join(GOLD, "motion_mask.npz"), **out)


def gen_dla_up():
    """The reference's REAL dla_utils classes (DLASegUpsample and everything under it) on the CPU.  Their file imports
    ModulatedDeformConvPack from the reference's deform_conv.py, which needs a CUDA torch (line 11 compares
    torch.version.cuda with a string) and the compiled extension: torch.version.cuda is set, a stand-in deform_conv_ext
    module is inserted, and the module-level modulated_deform_conv is pointed at the f64 restatement of
    tests/helpers_dcn.py.  So the wiring, the names and the initialisation are the real classes'; the arithmetic of the
    op is the restatement's.  Stored: the f64 output, the fp32 run's output (the yardstick), and for every parameter and
    input the f64 gradient norm and the L2 norm of the fp32 run's gradient deviation."""
    from tests import helpers_dcn as HD
    torch.version.cuda = torch.version.cuda or "11.0"
    pkg = "vision_base.networks.ops.dcn"
    sys.modules.setdefault(pkg + ".deform_conv_ext", types.ModuleType(pkg + ".deform_conv_ext"))
    import importlib
    dc = importlib.import_module(pkg + ".deform_conv")
    du = importlib.import_module("vision_base.networks.models.backbone.dla_utils")
    seen = []

    def restated(x, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups):
        assert groups == 1
        seen.append(float(offset.detach().abs().mean()))
        return HD.dcn_ref(x, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)
    dc.modulated_deform_conv = restated

    cfg = dict(HD.DLA_UP, input_channels=list(HD.DLA_UP["input_channels"]))
    ref = du.DLASegUpsample(**cfg)
    keys = list(ref.state_dict())
    assert all(float(m.conv_offset.weight.detach().abs().max()) == 0.0 for m in ref.modules()
               if isinstance(m, dc.ModulatedDeformConvPack))            # the reference's initialisation
    ref.load_state_dict(HD.dla_up_state(ref), strict=True)
    pyramid, cot = HD.dla_up_inputs()
    out64, g64 = HD.dla_up_run(ref, pyramid, cot, torch.float64)
    layers = len(seen)
    assert layers > 0 and min(seen) >= HD.DLA_UP_MIN_OFFSET, seen
    out32, g32 = HD.dla_up_run(ref, pyramid, cot, torch.float32)
    names = sorted(g64)
    gold = {
        "keys": np.array(keys), "shapes": np.array([",".join(map(str, ref.state_dict()[k].shape)) for k in keys]),
        "out": npy(out64), "out_fp32": npy(out32),
        "grad_names": np.array(names),
        "grad_norm": np.array([float(g64[k].norm()) for k in names]),
        "grad_fp32_dev": np.array([float((g32[k].double() - g64[k]).norm()) for k in names]),
        "offset_mean_abs": np.array(seen[:layers]),
    }
    path = os.path.join(GOLD, "dla_up.npz")
    np.savez_compressed(path, **gold)
    print("dla_up: %d DCN layers, mean |offset| %.2f .. %.2f px, out %s, fp32 deviation max %.2e, %d gradients, %d KiB" % (
        layers, min(seen), max(seen), tuple(out64.shape), float((out32.double() - out64).abs().max()), len(names),
        os.path.getsize(path) // 1024))


def gen_dla():
    """The reference's REAL dla.py classes on the CPU (tests/helpers_dla.py holds the inputs and the run helper).  Stored,
    as float32 roundings of the f64 results where they are arrays: the state_dict keys and shapes of the ten factories;
    per-key sum and abs-sum of a freshly initialised dla34 under one torch seed; and for DLA-34 and a small Bottleneck /
    residual_root network one training-mode forward and backward at N = 2, 64 x 64 — the f64 features, per level the
    (max, rms) deviation of the fp32 run and of the fp32 run whose convolutions read bf16-rounded operands, for every
    parameter and the input the f64 gradient norm and the L2 norm of both runs' gradient deviations, the names without
    gradient, every BatchNorm buffer after the forward and the two runs' deviations of the running statistics."""
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import helpers_dla as HL
    ref = importlib.import_module("vision_base.networks.models.backbone.dla")
    gold = {"factories": np.array(HL.FACTORIES)}
    for name in HL.FACTORIES:
        sd = HL.build_factory(ref, name).state_dict()
        gold[name + "/keys"] = np.array(list(sd))
        gold[name + "/shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    torch.manual_seed(HL.INIT_SEED)
    sd = HL.build_factory(ref, "dla34").state_dict()
    gold["init/sum"] = np.array([float(v.double().sum()) for v in sd.values()])
    gold["init/abs_sum"] = np.array([float(v.double().abs().sum()) for v in sd.values()])
    for which in HL.NETS:
        x, cots = HL.net_inputs(which)
        runs = {}
        for tag, dtype, rounded in (("f64", torch.float64, False), ("fp32", torch.float32, False), ("bf16", torch.float32, True)):
            m = HL.build_net(ref, which)
            m.load_state_dict(HL.net_state(m, which), strict=True)
            if rounded:
                HL.round_conv_operands_to_bf16(m)
            runs[tag] = HL.run_net(m, x, cots, dtype)
        feats, g64, none, bufs = runs["f64"]
        names = sorted(g64)
        gold[which + "/keys"] = np.array(list(m.state_dict()))
        gold[which + "/none_names"] = np.array(none)
        gold[which + "/grad_names"] = np.array(names)
        gold[which + "/grad_norm"] = np.array([float(g64[k].norm()) for k in names])
        for i, f in enumerate(feats):
            gold["%s/feat%d" % (which, i)] = npy(f).astype(np.float32)
        gold[which + "/buf_names"] = np.array(sorted(bufs))
        for k in bufs:
            gold["%s/buf/%s" % (which, k)] = npy(bufs[k]).astype(np.int64 if k.endswith("tracked") else np.float32)
        for tag in ("fp32", "bf16"):
            f2, g2, none2, b2 = runs[tag]
            assert none2 == none and sorted(g2) == names
            gold["%s/feat_dev_%s" % (which, tag)] = np.array([HL.deviation(a, b) for a, b in zip(f2, feats)])
            gold["%s/grad_dev_%s" % (which, tag)] = np.array([float((g2[k].double() - g64[k]).norm()) for k in names])
            gold["%s/buf_dev_%s" % (which, tag)] = np.array([HL.buffer_deviation(b2, bufs, sfx) for sfx in ("running_mean", "running_var")])
        print("dla %s: %d features, %d gradients, %d without; fp32 feature deviation max %.1e, bf16-operand %.1e" % (
            which, len(feats), len(names), len(none), gold[which + "/feat_dev_fp32"][:, 0].max(),
            gold[which + "/feat_dev_bf16"][:, 0].max()))
    path = os.path.join(GOLD, "dla.npz")
    np.savez_compressed(path, **gold)
    print("dla.npz: %d KiB" % (os.path.getsize(path) // 1024))


if __name__ == "__main__":
    if "--only-dla" in sys.argv:
        gen_dla()
        sys.exit(0)
    if "--only-dla-up" in sys.argv:
        gen_dla_up()
        sys.exit(0)
    if "--only-motion-mask" in sys.argv:
        gen_motion_mask()
        sys.exit(0)
    if "--only-nsrc" in sys.argv:
        gen_loss_chain_nsrc()
        sys.exit(0)
    if "--only-fisheye-nsrc" in sys.argv:
        gen_fisheye_nsrc()
        sys.exit(0)
    if "--only-postopt" in sys.argv:
        gen_postopt()
        sys.exit(0)
    if "--only-onnx" in sys.argv:
        gen_onnx()
        sys.exit(0)
    if "--only-velo" in sys.argv:
        gen_velo_gt()
        sys.exit(0)
    if "--only-noov" in sys.argv:
        gen_no_overlap_mask()
        sys.exit(0)
    if "--only-concat" in sys.argv:
        gen_concat()
        sys.exit(0)
    if "--only-frozen" in sys.argv:
        gen_frozen()
        sys.exit(0)
    if "--only-sigmoid" in sys.argv:
        gen_sigmoid_decoder()
        sys.exit(0)
    if "--only-distill-unscaled" in sys.argv:
        gen_distill_unscaled()
        sys.exit(0)
    if "--only-teacher" in sys.argv:
        gen_teacher_keys()
        sys.exit(0)
    if "--only-augment" in sys.argv:
        gen_augment()
        sys.exit(0)
    if "--only-augment-resize" in sys.argv:
        gen_augment_resize()
        sys.exit(0)
    if "--only-augment-mask" in sys.argv:
        gen_augment_mask()
        sys.exit(0)
    if "--only-augment-ext" in sys.argv:
        gen_augment_ext()
        sys.exit(0)
    if "--only-fisheye" in sys.argv:
        gen_fisheye()
        sys.exit(0)
    if "--only-options" in sys.argv:
        gen_loss_options()
        sys.exit(0)
    if "--only-kitti360" in sys.argv:
        gen_kitti360_fisheye()
        sys.exit(0)
    if "--only-nusc" in sys.argv:
        gen_nusc()
        sys.exit(0)
    if "--only-kitti360-persp" in sys.argv:
        gen_kitti360_persp()
        sys.exit(0)
    if "--only-kitti" in sys.argv:
        gen_kitti_dataset()
        sys.exit(0)
    if "--only-kitti-eigen" in sys.argv:
        gen_kitti_eigen_test_dataset()
        sys.exit(0)
    if "--only-supervised-eval" in sys.argv:
        gen_supervised_eval()
        sys.exit(0)
    if "--only-r50fx" in sys.argv:
        gen_model_r50fx()
        sys.exit(0)
    gen_ops()
    gen_loss_chain()
    gen_loss_chain_nsrc()
    gen_model(True, "depthpose")
    gen_model(False, "wpose")
    gen_eval()
    gen_distill()
    gen_distill_unscaled()
    gen_augment()
    gen_fisheye()
    gen_fisheye_nsrc()
    gen_model_r50fx()
    gen_kitti_dataset()
    gen_kitti_eigen_test_dataset()
    gen_supervised_eval()
    gen_kitti360_fisheye()
    gen_kitti360_persp()
    gen_nusc()
    gen_loss_options()
    gen_teacher_keys()
    gen_sigmoid_decoder()
    gen_frozen()
    gen_concat()
    gen_augment_resize()
    gen_augment_mask()
    gen_no_overlap_mask()
    gen_velo_gt()
    gen_postopt()
    gen_motion_mask()
    gen_dla_up()
    gen_dla()
    gen_augment_ext()
    for f in sorted(os.listdir(GOLD)):
        print(f, os.path.getsize(os.path.join(GOLD, f)) // 1024, "KiB")
