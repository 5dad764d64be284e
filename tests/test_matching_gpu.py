"""GPU checks of the matching encoder: fs_cost_volume against the reference's golden cost volumes (fp32 against the f64
evaluation, with the reference's own fp32 noise e as the yardstick), its graph capture, the whole module — forward,
BatchNorm statistics, every parameter's gradient — against the reference's autograd in fp32 and bf16, and the ordinary
ResNet path before and after a matching encoder has run."""
import os

import numpy as np
import pytest
import torch

from fsnet_amd.monodepth.networks.models.backbone.resnet_matching import ResnetEncoderMatching, intrinsics_4x4
from tests import helpers_matching as HM

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CAP = 1e-3        # share of cells in which a discrete output may differ from the golden


@pytest.fixture
def compute_dtype():
    from fsnet_amd.engine.runtime import RT
    before = RT.compute_dtype

    def setter(dtype):
        RT.set_compute_dtype(dtype)
    yield setter
    RT.set_compute_dtype(before)


def nhwc(t, dev, dtype=torch.float32):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def op_tensors(name, dev, dtype=torch.float32):
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES[name]
    g = np.load(os.path.join(GOLD, "matching_op_%s.npz" % name))
    inp = HM.op_inputs(name)
    K, inv_K = intrinsics_4x4(inp["P2"])
    t = dict(cur=nhwc(inp["cur"], dev, dtype), look=nhwc(inp["look"].reshape(B * F, C, h, w), dev, dtype),
             K=torch.from_numpy(K).float().to(dev), inv_K=torch.from_numpy(inv_K).float().to(dev),
             poses=inp["poses"].to(dev), bins=torch.from_numpy(g["bins"]).to(dev))
    Ci_p = (C + D + 7) // 8 * 8 + 8          # always some padding channels behind the cost volume
    return g, t, Ci_p


def run_op(t, Ci_p, want_volume=True):
    from fsnet_amd.hip import ops
    B, h, w, C = t["cur"].shape
    cat = torch.full((B, h, w, Ci_p), 7.0, dtype=t["cur"].dtype, device=t["cur"].device)
    out = ops.cost_volume(t["cur"], t["look"], t["K"], t["inv_K"], t["poses"], t["bins"], cat, want_volume=want_volume)
    return cat, out


@gpu
@pytest.mark.parametrize("name", sorted(HM.OP_CASES))
def test_cost_volume_matches_reference_golden(dev, name):
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES[name]
    g, t, Ci_p = op_tensors(name, dev)
    cat, (conf, lowest, vol, missing) = run_op(t, Ci_p)
    torch.cuda.synchronize()
    e = float(g["e"])
    miss_ref = torch.from_numpy(g["missing"].astype(np.float32))
    differ = missing.cpu() != miss_ref
    assert int(differ.sum()) <= CAP * differ.numel(), int(differ.sum())
    dev64 = (vol.cpu().double() - torch.from_numpy(g["cost_f64"]))[~differ].abs().max()
    print("case %s: kernel vs f64 %.3e, reference's own noise e %.3e, cells with another missing flag %d" % (
        name, float(dev64), e, int(differ.sum())))
    assert float(dev64) <= 4 * e, (float(dev64), e)
    conf_ref = torch.from_numpy(g["confidence"].astype(np.float32))
    conf_same = conf.cpu() == conf_ref
    assert int((~conf_same).sum()) <= CAP * conf_ref.numel()
    low_ref = torch.from_numpy(g["lowest_cost"])
    low_same = (lowest.cpu() - low_ref).abs() <= 1e-6 * low_ref.abs()
    assert int((~low_same).sum()) <= CAP * low_ref.numel(), int((~low_same).sum())
    # the slice written into the concat buffer: cost * confidence; padding zero; the caller's channels untouched
    cat = cat.cpu()
    want = torch.from_numpy(g["cost_f64"]) * conf_ref.double().unsqueeze(1)
    ok = (~differ) & conf_same.unsqueeze(1)
    got = cat[..., C:C + D].permute(0, 3, 1, 2).double()
    assert float((got - want)[ok].abs().max()) <= 4 * e
    assert Ci_p > C + D and float(cat[..., C + D:].abs().max()) == 0.0
    assert bool((cat[..., :C] == 7.0).all())
    if zero is not None:
        # the all-zero pose is skipped on the device: sample `zero[0]` equals the same sample with that frame removed
        b, f = zero
        keep = [k for k in range(F) if k != f]
        t1 = dict(t, cur=t["cur"][b:b + 1], look=t["look"].view(B, F, h, w, C)[b, keep].contiguous(), K=t["K"][b:b + 1],
                  inv_K=t["inv_K"][b:b + 1], poses=t["poses"][b:b + 1, keep].contiguous())
        _, (_, _, vol1, _) = run_op(t1, Ci_p)
        assert torch.equal(vol1[0], vol[b])


@gpu
def test_cost_volume_bf16_features_fp32_costs(dev):
    """bf16 features, every cost operation in fp32: against the host form evaluated on the same bf16-rounded features in
    f64, the deviation is fp32 noise (the 4 e of the fp32 case), not bf16's"""
    from fsnet_amd.monodepth.networks.models.backbone.resnet_matching import match_features_host
    name = "a"
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES[name]
    g, t, Ci_p = op_tensors(name, dev, torch.bfloat16)
    cat, (conf, lowest, vol, missing) = run_op(t, Ci_p)
    inp = HM.op_inputs(name)
    K, inv_K = intrinsics_4x4(inp["P2"])
    c64, m64 = match_features_host(inp["cur"].bfloat16(), inp["look"].bfloat16(), inp["poses"], torch.from_numpy(K),
                                   torch.from_numpy(inv_K), torch.from_numpy(g["bins"]), dtype=torch.float64)
    differ = missing.cpu().double() != m64
    assert int(differ.sum()) <= CAP * differ.numel()
    d = float((vol.cpu().double() - c64)[~differ].abs().max())
    print("bf16 features: kernel vs f64 on the rounded features %.3e (e %.3e)" % (d, float(g["e"])))
    assert d <= 4 * float(g["e"])
    got = cat[..., C:C + D].float().cpu().permute(0, 3, 1, 2)
    want = (vol * conf.unsqueeze(1)).bfloat16().float().cpu()
    assert torch.equal(got, want)
    assert float(cat[..., C + D:].float().abs().max()) == 0.0 and bool((cat[..., :C].float() == 7.0).all())


@gpu
def test_cost_volume_graph_replay_follows_the_pose_tensor(dev):
    """captured on one stream, replayed after the poses were overwritten in place — one frame with the all-zero matrix:
    the replay equals the eager result, so the missing-frame decision is taken on the device"""
    from fsnet_amd.hip import ops
    g, t, Ci_p = op_tensors("c", dev)
    B, h, w, C = t["cur"].shape
    new_poses = t["poses"].flip(1).clone()
    new_poses[0, 1] = 0.0
    eager_cat, eager = run_op(dict(t, poses=new_poses), Ci_p)
    cat = torch.full((B, h, w, Ci_p), 7.0, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.cost_volume(t["cur"], t["look"], t["K"], t["inv_K"], t["poses"], t["bins"], cat, want_volume=True)   # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.cost_volume(t["cur"], t["look"], t["K"], t["inv_K"], t["poses"], t["bins"], cat, want_volume=True)
    t["poses"].copy_(new_poses)
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert torch.equal(cat, eager_cat)
    # and the zero frame did change the result
    _, first = run_op(dict(t, poses=g_poses(g, dev)), Ci_p)
    assert not torch.equal(first[2], eager[2])


def g_poses(g, dev):
    return torch.from_numpy(g["poses"]).to(dev)


# ---------------------------------------------------------------------------------------------- the module
def build_module(dev, train):
    m = HM.MODULE
    net = ResnetEncoderMatching(m["depth"], False, m["H"], m["W"], min_depth_bin=HM.MIN_BIN, max_depth_bin=HM.MAX_BIN,
                                num_depth_bins=m["D"])
    net.load_state_dict(HM.init_state(net.state_dict(), seed=11), strict=True)
    net = net.to(dev)
    assert net.is_cuda and net.depth_bins.is_cuda
    return net.train() if train else net.eval()


_RUNS = {}


def train_run(dev, dtype):
    """one .train() forward + backward of the module in `dtype`, computed once per dtype and shared by the tests"""
    from fsnet_amd.engine.runtime import RT
    if dtype not in _RUNS:
        RT.set_compute_dtype(dtype)
        net = build_module(dev, train=True)
        cur, look, poses, P2 = [t.to(dev) for t in HM.module_inputs()]
        feats, lowest, conf = net(cur, look, poses, P2)
        loss = sum(f.float().pow(2).mean() for f in feats)
        loss.backward()
        torch.cuda.synchronize()
        _RUNS[dtype] = dict(net=net, feats=[f.detach().float().cpu() for f in feats], lowest=lowest.cpu(), conf=conf.cpu(),
                            loss=float(loss))
    return _RUNS[dtype]


def feature_devs(feats, g, tag):
    """max |feature - golden| relative to the golden feature's largest magnitude, per level (on the thinned sample)"""
    out = []
    for i, f in enumerate(feats):
        ref = g["%s_feat%d" % (tag, i)]
        got = HM.thin(f.numpy(), 16384)
        assert got.shape == ref.shape
        out.append((float(np.abs(got - ref).max()), float(np.abs(ref).max())))
    return out


def gradient_devs(net, g):
    """per parameter: (rel-L2 deviation on the golden's sample of the gradient, relative deviation of its norm)"""
    names = [str(k) for k in g["grad_names"]]
    params = dict(net.named_parameters())
    out = {}
    for k, n in zip(names, g["grad_norms"]):
        ref = g["grad/" + k].astype(np.float64)
        assert params[k].grad is not None, k
        got = HM.thin(params[k].grad.float().cpu().numpy(), 1024).astype(np.float64)
        if n < 1e-7:
            continue
        out[k] = (float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)),
                  abs(float(params[k].grad.double().norm()) - n) / n)
    return out


def discrete_ok(got, ref):
    return int((got != ref).sum()) <= CAP * ref.numel()


@gpu
def test_module_fp32_train_forward_matches_reference(dev, compute_dtype):
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    run = train_run(dev, torch.float32)
    assert [tuple(f.shape) for f in run["feats"]] == [(2, 64, 32, 48), (2, 64, 16, 24), (2, 128, 8, 12), (2, 256, 4, 6),
                                                      (2, 512, 2, 3)]
    devs = feature_devs(run["feats"], g, "train")
    print("fp32 train features: max abs deviation per level", ["%.2e (max %.2f)" % d for d in devs])
    for d, _ in devs:
        assert d < 2e-3                                   # the bound tests/test_model_gpu.py applies to encoder features
    assert abs(run["loss"] - float(g["loss"])) < 2e-4 * float(g["loss"])
    assert discrete_ok(run["conf"], torch.from_numpy(g["train_conf"].astype(np.float32)))
    low_ref = torch.from_numpy(g["train_lowest"])
    assert int(((run["lowest"] - low_ref).abs() > 1e-6 * low_ref).sum()) <= CAP * low_ref.numel()
    assert 0.0 < float(run["conf"].mean()) < 1.0


@gpu
def test_module_fp32_running_statistics_after_two_updates(dev, compute_dtype):
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    sd = train_run(dev, torch.float32)["net"].state_dict()
    rm = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_mean")]).cpu()
    rv = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_var")]).cpu()
    nbt = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    # stem and layer1 saw the current images, then the B*F lookup images as one group; layer2-4 one batch
    assert nbt == [int(x) for x in g["num_batches_tracked"]] and sorted(set(nbt)) == [1, 2]
    assert float((rm - torch.from_numpy(g["running_mean"])).abs().max()) < 5e-3
    assert float(((rv - torch.from_numpy(g["running_var"])).abs() / torch.from_numpy(g["running_var"])).max()) < 5e-3


@gpu
def test_module_fp32_gradients_match_reference_autograd(dev, compute_dtype):
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    net = train_run(dev, torch.float32)["net"]
    assert bool(g["prematching_grad_is_none"])
    assert all(p.grad is None for p in net.prematching_conv.parameters())
    devs = gradient_devs(net, g)
    assert len(devs) >= 55
    worst = max(devs.items(), key=lambda kv: kv[1][0])
    print("fp32 gradients: worst rel-L2 %.3e (%s), worst norm deviation %.3e" % (
        worst[1][0], worst[0], max(v[1] for v in devs.values())))
    for k, (rel, nrm) in devs.items():
        assert rel < 2e-2 and nrm < 2e-2, (k, rel, nrm)   # tests/test_model_gpu.py's bound on parameter gradients


@gpu
def test_module_fp32_eval_forward_matches_reference(dev, compute_dtype):
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    compute_dtype(torch.float32)
    net = build_module(dev, train=False)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    cur, look, poses, P2 = [t.to(dev) for t in HM.module_inputs()]
    with torch.no_grad():
        feats, lowest, conf = net(cur, look, poses, P2)
    torch.cuda.synchronize()
    devs = feature_devs([f.float().cpu() for f in feats], g, "eval")
    print("fp32 eval features: max abs deviation per level", ["%.2e (max %.2f)" % d for d in devs])
    for d, _ in devs:
        assert d < 2e-3
    assert discrete_ok(conf.cpu(), torch.from_numpy(g["eval_conf"].astype(np.float32)))
    low_ref = torch.from_numpy(g["eval_lowest"])
    assert int(((lowest.cpu() - low_ref).abs() > 1e-6 * low_ref).sum()) <= CAP * low_ref.numel()
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k               # nothing is updated in eval mode
    assert feats is net.features and not feats[0].requires_grad


# bf16 against the fp32 golden, measured once on an MI355X for exactly this module, input and seed; each bound is twice
# the measured maximum (measured, bound).  The gradients of this loss are badly conditioned — BatchNorm in training mode
# over 12 to 1 536 values per channel — and bf16 moves every layer's by a similar amount, layer4's (which no new code
# touches in the backward) as much as the stem's: median rel-L2 0.259.
BF16_FEATURE = (0.0577, 0.1154)     # max |feature - golden| / max |golden|, worst level (0.0041 at level 0 ... 0.0577 at level 4)
BF16_GRAD = (0.3959, 0.7918)        # worst per-parameter rel-L2 of a gradient (layer1.1.0.conv1.weight)
BF16_NORM = (0.0615, 0.1230)        # worst relative deviation of a gradient's norm
# The confidence mask is geometry plus `cost > 0` and keeps the cap of the fp32 tests (measured: 0 cells differ).  The
# lowest-cost map is an argmin over costs of bf16-rounded features: 17 of 768 cells choose another bin than the fp32
# golden; bounded like the continuous outputs, at twice the measured count.
BF16_LOWEST_CELLS = (17, 34)


@gpu
def test_module_bf16_forward_and_gradients(dev, compute_dtype):
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    run = train_run(dev, torch.bfloat16)
    fd = [d / m for d, m in feature_devs(run["feats"], g, "train")]
    gd = gradient_devs(run["net"], g)
    worst_g, worst_n = max(v[0] for v in gd.values()), max(v[1] for v in gd.values())
    flips = int((run["conf"] != torch.from_numpy(g["train_conf"].astype(np.float32))).sum())
    low_ref = torch.from_numpy(g["train_lowest"])
    low_flips = int(((run["lowest"] - low_ref).abs() > 1e-6 * low_ref).sum())
    print("bf16 gradients, six worst rel-L2:", sorted(((round(v[0], 4), k) for k, v in gd.items()), reverse=True)[:6],
          "median %.4f" % float(np.median([v[0] for v in gd.values()])))
    print("bf16: feature deviation / max per level %s; gradients worst rel-L2 %.4f, worst norm deviation %.4f; "
          "confidence cells that differ %d, lowest-cost cells that differ %d of %d" % (
              ["%.4f" % d for d in fd], worst_g, worst_n, flips, low_flips, low_ref.numel()))
    assert all(p.grad is None for p in run["net"].prematching_conv.parameters())
    assert len(gd) >= 55
    assert flips <= CAP * low_ref.numel()
    assert low_flips <= BF16_LOWEST_CELLS[1]
    assert max(fd) < BF16_FEATURE[1]
    assert worst_g < BF16_GRAD[1] and worst_n < BF16_NORM[1]


@gpu
def test_plain_resnet_is_bit_identical_around_a_matching_encoder(dev, compute_dtype):
    """the engine additions (a pass that stops after stage 0, a pass entered at stage 1) leave the ordinary path alone"""
    from fsnet_amd.vision_base.networks.models.backbone.resnet import resnet
    compute_dtype(torch.float32)
    torch.manual_seed(5)
    net = resnet(18, pretrained=False, norm_eval=False).to(dev).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    x = HM.module_inputs()[0].to(dev)

    def step():
        net.load_state_dict(state)
        for p in net.parameters():
            p.grad = None
        feats = net(x)
        sum(f.float().pow(2).mean() for f in feats).backward()
        torch.cuda.synchronize()
        return [f.detach().clone() for f in feats], [p.grad.clone() for p in net.parameters()], \
            [v.clone() for v in net.state_dict().values()]

    before = step()
    m = build_module(dev, train=True)
    cur, look, poses, P2 = [t.to(dev) for t in HM.module_inputs()]
    feats, _, _ = m(cur, look, poses, P2)
    sum(f.float().pow(2).mean() for f in feats).backward()
    torch.cuda.synchronize()
    after = step()
    for a, b in zip(before, after):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
