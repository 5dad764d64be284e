"""TEST INFRASTRUCTURE ONLY — the is_unscaled_distill term of compute_distill_loss (reference monodepth2_decoder.py:
185-203) restated in torch, in float32 (the reference's own arithmetic) and float64 (the yardstick), the seeded cases
the CPU and GPU tests share, and the layout of tests/golden/distill_unscaled.npz (tools/gen_golden.py:
gen_distill_unscaled writes it from the REAL MonoDepth2Decoder / DistillWPoseMeta).

    ratio = mean_j p_j / (t_j + 1e-5) per (sample, channel) plane;  x = ratio t - p
    loss  = mean |x| / u + log(u + 1e-5)      (no uncertainty: mean |x|)
"""
import functools

import numpy as np
import torch

MIN_ABS_X = 1e-3          # every case keeps |x| this far from the kink of |x| (float64), no element excused
ULP = 2.0 ** -23

# name -> list of [planes, 1, h, w] per scale; "three_blocks" is placed on the kernels' chunk seams (see shapes())
_SHAPES = {
    "below_wave": [(1, 1, 3, 5)],
    "sibling": [(3, 1, 24, 40)],
    "odd": [(2, 1, 17, 63)],                 # odd n: the second plane starts 4-byte aligned
    "four_scales": [(2, 1, 24, 40), (2, 1, 12, 20), (2, 1, 6, 10), (2, 1, 3, 5)],
}
SMALL = ("below_wave", "sibling", "odd", "four_scales")       # the cases the golden file pins
ALL = SMALL + ("three_blocks",)
SAMPLES = 8               # elements of a gradient the golden file keeps (evenly spaced), beside its sum and |.| sum


def shapes(name, chunk=None):
    if name == "three_blocks":
        assert chunk, "three_blocks needs the kernels' chunk (fs_distill_unscaled_chunk)"
        n = 2 * int(chunk) + 5                 # a plane over three blocks, the last one ragged
        h = next((d for d in (3, 5, 7, 11, 13) if n % d == 0), 1)
        return [(2, 1, h, n // h)]
    return list(_SHAPES[name])


def restate(pred, teacher, uncertain=None, dtype=torch.float32, gout=1.0):
    """-> (loss, d_pred, d_uncertain | None) of one scale, the reference's lines in `dtype` with autograd's backward"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    t = teacher.detach().to(dtype)
    u = None if uncertain is None else uncertain.detach().to(dtype).clone().requires_grad_(True)
    ratio = (p / (t + 1e-5)).mean(dim=[2, 3], keepdim=True)
    error = (ratio * t - p).abs()
    loss = (error / u + torch.log(u + 1e-5) if u is not None else error).mean()
    (loss * gout).backward()
    return loss.detach(), p.grad, None if u is None else u.grad


def min_abs_x(pred, teacher):
    p, t = pred.double(), teacher.double()
    ratio = (p / (t + 1e-5)).mean(dim=[2, 3], keepdim=True)
    return float((ratio * t - p).abs().min())


def _draw(shape_list, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for sh in shape_list:
        p = torch.rand(*sh, generator=gen) * 50 + 1
        t = torch.rand(*sh, generator=gen) * 50 + 1
        u = torch.rand(*sh, generator=gen) * 0.9 + 0.05
        out.append((p, t, u))
    return out


@functools.lru_cache(maxsize=None)
def case(name, chunk=None):
    """-> dict(seed, pred[s], teacher[s], uncertain[s]) of fp32 CPU tensors, pred / teacher in [1, 51), uncertain in
    [0.05, 0.95): the first seed in 0, 1, 2, ... whose every element has |x| >= MIN_ABS_X in float64.  Shared: do not
    write into the tensors."""
    sl = shapes(name, chunk)
    for seed in range(64):
        drawn = _draw(sl, seed)
        if all(min_abs_x(p, t) >= MIN_ABS_X for p, t, _ in drawn):
            return dict(seed=seed, pred=[d[0] for d in drawn], teacher=[d[1] for d in drawn],
                        uncertain=[d[2] for d in drawn])
    raise AssertionError("no seed below 64 keeps |x| >= %g for %s" % (MIN_ABS_X, name))


@functools.lru_cache(maxsize=None)
def references(name, chunk=None, with_unc=True, gout=1.0):
    """per scale: dict(f32=(loss, dp, du), f64=(loss, dp, du)) of restate(); computed once per case"""
    c = case(name, chunk)
    out = []
    for s in range(len(c["pred"])):
        u = c["uncertain"][s] if with_unc else None
        out.append(dict(f32=restate(c["pred"][s], c["teacher"][s], u, torch.float32, gout),
                        f64=restate(c["pred"][s], c["teacher"][s], u, torch.float64, gout)))
    return out


def yardstick(f32, f64):
    """e = max(|fp32 restatement - float64|_max, 2^-23 max |float64 value|)"""
    f32, f64 = torch.as_tensor(f32).double(), torch.as_tensor(f64).double()
    return max(float((f32 - f64).abs().max()), ULP * float(f64.abs().max()))


# ---- golden file layout ---------------------------------------------------------------------------------------
def golden_rows():
    """(case name, scale index) of every row of the k_* arrays"""
    return [(name, s) for name in SMALL for s in range(len(_SHAPES[name]))]


def digest(g):
    """a gradient tensor as SAMPLES evenly spaced elements, its sum and its sum of magnitudes (float64 ndarray)"""
    g = g.detach().double().flatten()
    idx = np.linspace(0, g.numel() - 1, SAMPLES).round().astype(np.int64)
    return np.concatenate([g[torch.from_numpy(idx)].numpy(), [float(g.sum()), float(g.abs().sum())]])


def digest_tolerance(n, tol):
    """bound on each entry of digest() when every element is within `tol`; the stored digest is float32"""
    return np.array([tol] * SAMPLES + [n * tol, n * tol])


# ---- model level: DistillWPoseMeta.forward_train with the flag ---------------------------------------------------
MODEL = dict(B=2, H=64, W=128, seed=21, teacher_seed=22, batch_seed=400)      # gen_distill's step


def distill_loss_unscaled(pred, teacher, uncertain=None):
    t = teacher.detach()
    ratio = (pred / (t + 1e-5)).mean(dim=[2, 3], keepdim=True)
    error = (ratio * t - pred).abs()
    return (error / uncertain + torch.log(uncertain + 1e-5) if uncertain is not None else error).mean()


def forward_train_unscaled(sd, data, is_uncertain_distill=True, distillation_loss_weight=0.3, scales=(0, 1, 2, 3),
                           frame_ids=(0, 1, -1), min_depth=0.5, max_depth=100.0):
    """oracle/distill_oracle.forward_train with the distillation term replaced; its own pieces otherwise"""
    from oracle import distill_oracle as D
    from oracle import fsnet_oracle as O
    feats = O.resnet_forward(sd, "depth_backbone.", data[("image", 0)], 18)
    outputs = D.decoder_uncertain_forward(sd, "head.depth_decoder.", feats, min_depth, max_depth, scales)
    with torch.no_grad():
        tf = O.resnet_forward(sd, "teacher_net.depth_backbone.", data[("image", 0)], 18, train=False)
        to = O.depth_decoder_forward(sd, "teacher_net.depth_decoder.", tf, min_depth, max_depth, scales, train=False)
    for s in scales:
        outputs[("teacher_depth", s, s)] = to[("depth", s, s)]
    for f in frame_ids[1:]:
        outputs[("cam_T_cam", f)] = data[("relative_pose", f)]
    total, losses = O.photometric_loss(outputs, data, frame_ids, scales, True, None)
    for s in scales:
        dl = distill_loss_unscaled(outputs[("depth", s, s)], outputs[("teacher_depth", s, s)],
                                   outputs[("uncertain_z", s)] if is_uncertain_distill else None)
        losses["distilation/%d" % s] = dl.detach()
        total = total + dl * distillation_loss_weight
    losses["total_loss"] = total.detach()
    return total, losses, outputs
