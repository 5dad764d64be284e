"""Training with one, three and four temporal source frames (train_cfg.frame_ids of other lengths than three) through the
meta-archs, the training hook and the N-frame loss kernels (photo_multi.hip), against the CPU oracle on the same batch.
fp32, B = 2, 64 x 128, O.init_state(seed=3); bounds: those of tests/test_model_gpu.py::test_fp32_gradients_match_oracle
(loss 1e-5 relative, every parameter gradient 2e-2 relative L2), tests/test_graph_gpu.py::test_graph_replay_matches_eager
(graph against eager inside the larger of a floor and five times the spread of two eager runs) and
tests/test_model_gpu.py::test_bf16_training_step_close_to_fp32_oracle (the bf16 policy band)."""
import pytest
import torch

from oracle import fsnet_oracle as O

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 128


def to_dev(data, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in data.items()}


def build_model(with_pose, fids, dev, dtype, sd0):
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.utils.builder import build
    RT.set_compute_dtype(dtype)
    RT.tie_noise = False
    m = build(**meta_arch_cfg(H, W, with_pose=with_pose, frame_ids=fids))
    m.load_state_dict({k: v.clone() for k, v in sd0.items()}, strict=True)
    return m.to(dev).train()


def oracle_step(sd0, data, with_pose, fids):
    """-> total, {name: gradient} of O.forward_train with these frame_ids"""
    sd = {k: v.clone() for k, v in sd0.items()}
    names = [k for k in sd if O.is_param(k)]
    for k in names:
        sd[k] = sd[k].requires_grad_(True)
    total, _, _ = O.forward_train(sd, data, 18, with_pose, frame_ids=tuple(fids))
    grads = torch.autograd.grad(total.mean(), [sd[k] for k in names], allow_unused=True)
    return total.detach(), {k: (g if g is not None else torch.zeros_like(sd[k])) for k, g in zip(names, grads)}


@pytest.mark.parametrize("with_pose,fids", [(True, [0, -1]), (True, [0, -2, -1, 1]), (True, [0, -2, -1, 1, 2]),
                                            (False, [0, -1])],
                         ids=["meta-1", "meta-3", "meta-4", "wpose-1"])
def test_fp32_loss_and_gradients_match_oracle(dev, with_pose, fids):
    from fsnet_amd.hip import ops
    sd0 = O.init_state(seed=3, with_pose=with_pose)
    m = build_model(with_pose, fids, dev, torch.float32, sd0)
    data = O.synthetic_batch(B, H, W, seed=7, frame_ids=tuple(fids))
    try:
        out = m(to_dev(data, dev), dict(is_training=True))
        out["loss"].backward()
        torch.cuda.synchronize()
    finally:
        from fsnet_amd.engine.runtime import RT
        RT.set_compute_dtype(torch.bfloat16)
    assert isinstance(m.head._pl, ops.PhotometricLossMulti) and m.head._pl.nsrc == len(fids) - 1
    total, raw = oracle_step(sd0, data, with_pose, fids)
    print("loss %.8f oracle %.8f" % (float(out["loss"]), float(total)))
    assert abs(float(out["loss"]) - float(total)) < 1e-5 * abs(float(total))
    worst = 0.0
    for k, p in m.named_parameters():
        ref = raw[k]
        if ref.norm() < 1e-7:
            continue
        rel = float((p.grad.cpu() - ref).norm() / ref.norm())
        worst = max(worst, rel)
        assert rel < 2e-2, (k, rel)
    print("worst per-parameter gradient rel-L2 deviation:", worst)


def _run_hook(dev, graph_warmup, fids, steps=3):
    from fsnet_amd.configs import training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    sd0 = O.init_state(seed=3, with_pose=True)
    m = build_model(True, fids, dev, torch.float32, sd0)
    tc = training_cfg()
    opt = build_optimizer(m, **tc.optimizer)
    hook = build(**tc.training_hook)
    hook.graph_warmup = graph_warmup
    losses = []
    try:
        for it in range(steps):
            out = hook(dict(O.synthetic_batch(B, H, W, seed=50 + it, frame_ids=tuple(fids))), m, opt)
            losses.append(out["loss"].detach().clone())
        torch.cuda.synchronize()
    finally:
        RT.set_compute_dtype(torch.bfloat16)
    params = torch.cat([p.detach().double().flatten() for p in m.parameters()]).cpu()
    rm = torch.cat([v.double().flatten() for k, v in m.state_dict().items() if "running_" in k]).cpu()
    return torch.stack(losses).cpu(), params, rm, hook


def test_three_source_step_captures_and_replays(dev):
    """[0, -2, -1, 1] through BaseTrainingHook: steps 0 and 1 eager, step 2 captured and run as the first replay"""
    fids = [0, -2, -1, 1]
    le, pe, re_, he = _run_hook(dev, 99, fids)
    l2, p2, r2, _ = _run_hook(dev, 99, fids)
    lg, pg, rg, hg = _run_hook(dev, 2, fids)
    assert he.graph_captures == 0 and hg.graph_captures == 1

    def d(a, b, rel_floor=0.0):
        return float(((a - b).abs() / a.abs().clamp_min(rel_floor)).max()) if rel_floor else float((a - b).abs().max())
    print("loss %.2e (eager spread %.2e) params %.2e (%.2e) running %.2e (%.2e)" % (
        d(le, lg, 1e-9), d(le, l2, 1e-9), d(pe, pg), d(pe, p2), d(re_, rg, 1.0), d(re_, r2, 1.0)))
    assert d(le, lg, 1e-9) < max(1e-3, 5 * d(le, l2, 1e-9)), (le, lg, l2)
    assert d(pe, pg) < max(2e-3, 5 * d(pe, p2)), (d(pe, pg), d(pe, p2))
    assert d(re_, rg, 1.0) < max(3e-2, 5 * d(re_, r2, 1.0)), (d(re_, rg, 1.0), d(re_, r2, 1.0))


def test_bf16_three_source_step_close_to_fp32_oracle(dev):
    """one bf16 step of [0, -2, -1, 1] inside the band of test_bf16_training_step_close_to_fp32_oracle: loss 5e-3
    relative, convolution weight gradients cosine > 0.85 and norm within 0.9 .. 1.2 of the oracle's"""
    fids = [0, -2, -1, 1]
    sd0 = O.init_state(seed=3, with_pose=True)
    data = O.synthetic_batch(B, H, W, seed=7, frame_ids=tuple(fids))
    m = build_model(True, fids, dev, torch.bfloat16, sd0)
    out = m(to_dev(data, dev), dict(is_training=True))
    out["loss"].backward()
    torch.cuda.synchronize()
    total, raw = oracle_step(sd0, data, True, fids)
    dev_l = abs(float(out["loss"].detach()) - float(total)) / abs(float(total))
    print("bf16 loss rel dev %.5f" % dev_l)
    gmax = max(float(r.norm()) for r in raw.values())
    mincos, ratios = 1.0, []
    for k, p in m.named_parameters():
        ref = raw[k]
        if float(ref.norm()) < 1e-3 * gmax or ref.dim() != 4:
            continue
        g = p.grad.cpu()
        mincos = min(mincos, float((g * ref).sum() / (g.norm() * ref.norm())))
        ratios.append(float(g.norm() / ref.norm()))
    print("bf16 conv gradients: min cosine %.4f, norm ratio %.3f .. %.3f" % (mincos, min(ratios), max(ratios)))
    assert dev_l < 5e-3
    assert mincos > 0.85
    assert 0.9 < min(ratios) and max(ratios) < 1.2


DRIVER_CFG = '''
from easydict import EasyDict as edict
from fsnet_amd.configs import meta_arch_cfg, training_cfg
cfg = edict()
cfg.path = edict(checkpoint_path=%r)
cfg.trainer = edict(gpu=0, max_epochs=1, disp_iter=1000, save_iter=1, test_iter=0, max_iters=0,
                    training_hook=training_cfg().training_hook)
cfg.optimizer = edict(name='adam', lr=1e-4, weight_decay=0)
cfg.scheduler = edict(name='StepLR', step_size=15)
cfg.data = edict(batch_size=2, num_workers=0)
cfg.train_dataset = edict(name='fsnet_amd.vision_base.data.datasets.synthetic.SyntheticTripletDataset', size=6,
                          height=64, width=128, frame_idxs=%r)
cfg.meta_arch = meta_arch_cfg(64, 128, with_pose=%r, frame_ids=%r)
'''


@pytest.mark.parametrize("with_pose,fids", [(False, [0, -1]), (True, [0, -2, -1, 1]), (False, [0, -2, -1, 1, 2])],
                         ids=["wpose-1", "meta-3", "wpose-4"])
def test_driver_trains_with_other_frame_counts(dev, with_pose, fids):
    """a config that differs from the driver test's only in frame_ids / frame_idxs, through scripts/train.py"""
    import os
    import tempfile
    from fsnet_amd.hip import ops
    from fsnet_amd.scripts import train
    with tempfile.TemporaryDirectory() as d:
        cfgp = os.path.join(d, "cfg.py")
        open(cfgp, "w").write(DRIVER_CFG % (os.path.join(d, "ck"), fids, with_pose, fids))
        model = train.main(["--config", cfgp])
        files = os.listdir(os.path.join(d, "ck"))
        ck = torch.load(os.path.join(d, "ck", [f for f in files if f.endswith("_latest.pth")][0]), map_location="cpu")
    assert isinstance(model.head._pl, ops.PhotometricLossMulti) and model.head._pl.nsrc == len(fids) - 1
    assert float(ck["optimizer_state_dict"]["state"][0]["step"]) == 3.0
    assert all(bool(torch.isfinite(v).all()) for v in ck["model_state_dict"].values() if v.is_floating_point())
