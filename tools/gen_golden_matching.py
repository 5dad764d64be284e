"""Golden vectors of the matching encoder from the REAL reference class on the CPU.

Dev-only, like tools/gen_golden.py and with the same import shims (Tensor.cuda / Module.cuda as no-ops,
tools/ref_shims): imports monodepth.networks.models.backbone.resnet_matching.ResnetEncoderMatching from the
reference checkout, feeds it the seeded inputs and weights of tests/helpers_matching.py and writes
tests/golden/matching_*.npz.  Next to every fp32 cost volume it stores the same algorithm evaluated in f64 and
e = max |fp32 - f64|, the reference's own rounding noise, which the tests use as their yardstick.  A case whose
fp32 and f64 discrete outputs (missing, confidence, argmin) differ anywhere is refused: the inputs must keep the
reference itself inside the tests' cap on differing cells.

    python tools/gen_golden_matching.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools", "ref_shims"), "/root/reference", ROOT, os.path.join(ROOT, "tests")]
tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = type("SummaryWriter", (), {})
sys.modules["torch.utils.tensorboard"] = tb
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self

from monodepth.networks.models.backbone.resnet_matching import ResnetEncoderMatching as RefMatching  # noqa: E402
import helpers_matching as HM  # noqa: E402
from fsnet_amd.monodepth.networks.models.backbone.resnet_matching import intrinsics_4x4, match_features_host  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def npy(t):
    return t.detach().cpu().numpy()


def finish(ref, cost, missing):
    """the lines of the reference's forward behind match_features (resnet_matching.py:227-237) -> confidence, argmin,
    lowest cost, masked volume"""
    conf = ref.compute_confidence_mask(cost * (1 - missing))
    viz = cost.clone()
    viz[viz == 0] = 100
    _, argmin = torch.min(viz, 1)
    lowest = ref.indices_to_disparity(argmin)
    return conf, argmin, lowest, cost * conf.unsqueeze(1)


def gen_op(name):
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES[name]
    inp = HM.op_inputs(name)
    ref = RefMatching(18, False, 4 * h, 4 * w, min_depth_bin=near, max_depth_bin=HM.MAX_BIN, num_depth_bins=D,
                      depth_binning=binning)
    with torch.no_grad():
        cost, missing = ref.match_features(inp["cur"], inp["look"], inp["poses"], inp["P2"])
        conf, argmin, lowest, masked = finish(ref, cost, missing)
        # the same algorithm in f64 (fp32 inputs widened; intrinsics and their pseudo-inverse never rounded to fp32)
        K, inv_K = intrinsics_4x4(inp["P2"])
        c64, m64 = match_features_host(inp["cur"], inp["look"], inp["poses"], torch.from_numpy(K), torch.from_numpy(inv_K),
                                       ref.depth_bins, dtype=torch.float64)
        conf64, argmin64, _, _ = finish(ref, c64, m64)
        # this repository's fp32 host form against the reference (printed; tests/test_matching_cpu.py asserts it)
        K32, iK32 = torch.from_numpy(K).float(), torch.from_numpy(inv_K).float()
        ch, mh = match_features_host(inp["cur"], inp["look"], inp["poses"], K32, iK32, ref.depth_bins)
    flips = int((missing != m64.float()).sum()), int((conf != conf64.float()).sum()), int((argmin != argmin64).sum())
    e = float((cost.double() - c64).abs().max())
    print("op case %s: cells %d, missing share %.3f, confidence share %.3f, flips fp32/f64 (missing, conf, argmin) %s, "
          "e = %.3e, host form vs reference: max dev %.3e, mask flips %d" % (
              name, cost.numel(), float(missing.mean()), float(conf.mean()), flips, e,
              float((ch - cost).abs().max()), int((mh != missing).sum())))
    if any(flips):
        raise SystemExit("case %s: the reference's fp32 and f64 discrete outputs differ — choose other inputs" % name)
    np.savez_compressed(
        os.path.join(GOLD, "matching_op_%s.npz" % name), poses=npy(inp["poses"]), P2=npy(inp["P2"]),
        bins=npy(ref.depth_bins), cur_sum=np.float64(inp["cur"].double().sum()), look_sum=np.float64(inp["look"].double().sum()),
        cost=npy(cost), cost_f64=npy(c64), missing=npy(missing).astype(np.uint8), confidence=npy(conf).astype(np.uint8),
        argmin=npy(argmin).astype(np.int16), lowest_cost=npy(lowest), e=np.float64(e))


def gen_module():
    m = HM.MODULE
    cur, look, poses, P2 = HM.module_inputs()

    def fresh():
        torch.manual_seed(0)
        ref = RefMatching(m["depth"], False, m["H"], m["W"], min_depth_bin=HM.MIN_BIN, max_depth_bin=HM.MAX_BIN,
                          num_depth_bins=m["D"])
        ref.load_state_dict(HM.init_state(ref.state_dict(), seed=11), strict=True)
        return ref

    ref = fresh()
    out = {}
    sd = ref.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array(json.dumps([list(v.shape) for v in sd.values()]))
    bn = ref.layer0[1]
    out["bn_training_after_init"] = np.array(bn.training)
    ref.train()
    out["bn_training_after_train"] = np.array(bn.training)
    feats, lowest, conf = ref(cur, look, poses, P2)
    loss = sum(f.float().pow(2).mean() for f in feats)
    loss.backward()
    for i, f in enumerate(feats):
        out["train_feat%d" % i] = HM.thin(npy(f), 16384)
    out["train_lowest"], out["train_conf"], out["loss"] = npy(lowest), npy(conf).astype(np.uint8), np.float64(loss.item())
    names, norms = [], []
    for k, p in ref.named_parameters():
        if p.grad is None:
            assert k.startswith("prematching_conv"), k
            continue
        names.append(k)
        norms.append(float(p.grad.double().norm()))
        out["grad/" + k] = HM.thin(npy(p.grad), 1024)
    out["grad_names"], out["grad_norms"] = np.array(names), np.array(norms)
    out["prematching_grad_is_none"] = np.array(all(p.grad is None for p in ref.prematching_conv.parameters()))
    sd = ref.state_dict()
    out["running_mean"] = np.concatenate([npy(v).reshape(-1) for k, v in sd.items() if k.endswith("running_mean")])
    out["running_var"] = np.concatenate([npy(v).reshape(-1) for k, v in sd.items() if k.endswith("running_var")])
    out["num_batches_tracked"] = np.array([int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")])
    with torch.no_grad():
        cf = ref.features[1]
        conf_share = float(conf.mean())
    ref = fresh().eval()
    with torch.no_grad():
        feats, lowest, conf = ref(cur, look, poses, P2)
    for i, f in enumerate(feats):
        out["eval_feat%d" % i] = HM.thin(npy(f), 16384)
    out["eval_lowest"], out["eval_conf"] = npy(lowest), npy(conf).astype(np.uint8)
    print("module: %d state_dict keys, loss %.6f, %d gradients, train confidence share %.3f, eval %.3f, feature1 max %.3f" % (
        len(out["keys"]), out["loss"], len(names), conf_share, float(conf.mean()), float(cf.abs().max())))
    np.savez_compressed(os.path.join(GOLD, "matching_module.npz"), **out)


def gen_bins():
    out = {}
    for binning in ("linear", "inverse"):
        ref = RefMatching(18, False, 64, 96, min_depth_bin=HM.MIN_BIN, max_depth_bin=HM.MAX_BIN, num_depth_bins=96,
                          depth_binning=binning)
        out[binning] = npy(ref.depth_bins)
        idx = torch.arange(96).view(1, 8, 12) % 96
        out[binning + "_disp"] = npy(ref.indices_to_disparity(idx))
        ref.adaptive_bins = True
        ref.compute_depth_bins(0.9, 33.0)
        out[binning + "_adaptive"] = npy(ref.depth_bins)
    np.savez_compressed(os.path.join(GOLD, "matching_bins.npz"), **out)


if __name__ == "__main__":
    gen_bins()
    for name in sorted(HM.OP_CASES):
        gen_op(name)
    gen_module()
