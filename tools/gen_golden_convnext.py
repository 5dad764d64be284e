"""Golden vectors of the ConvNeXt backbone from the REAL reference classes on the CPU.

Dev-only, like tools/gen_golden_matching.py and with the same import shims (tools/ref_shims): imports
vision_base.networks.models.backbone.convnext from the reference checkout, builds the two small networks of
tests/helpers_convnext.py with its seeded state and inputs, and writes tests/golden/convnext.npz:

  <net>/keys, <net>/none_names             state_dict keys in order; parameters without a gradient
  <net>/feat<i>                            f64 features
  <net>/full_names, <net>/grad/<name>      f64 gradients of the parameters convnext.hip writes (depthwise, LayerNorm, gamma)
  <net>/gemm_names, /gemm_norm, /gemm_proj f64 gradient norm and one seeded projection of the GEMM parameters
  <net>/feat_dev_<y>, /full_dev_<y>        (max, rms) deviation of yardstick run y from f64, per feature / full gradient
  <net>/gemm_dev_<y>                       L2 norm of the yardstick's gradient deviation, per GEMM parameter
  init/keys, init/sums                     per-key sums of convnext_tiny(in_chans=6) under torch seed INIT_SEED
The yardsticks y: "fp32", the reference's fp32 run; "bf16", its fp32 run with every Conv2d / Linear input and weight
rounded to bf16.

    python tools/gen_golden_convnext.py
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

from vision_base.networks.models.backbone import convnext as ref  # noqa: E402
from tests import helpers_convnext as HC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "convnext.npz")
torch.set_num_threads(8)


def make(which):
    m = HC.build_net(ref, which)
    m.load_state_dict(HC.net_state(m, which), strict=True)
    return m


def gen_net(which, out):
    x, cots = HC.net_inputs(which)
    f64, g64, none64 = HC.run_net(make(which), x, cots, torch.float64)
    out[which + "/keys"] = np.array(list(make(which).state_dict()))
    out[which + "/none_names"] = np.array(none64)
    for i, f in enumerate(f64):
        out["%s/feat%d" % (which, i)] = f.numpy()
    full = [k for k in g64 if not HC.is_gemm_param(k)]
    gemm = [k for k in g64 if HC.is_gemm_param(k)]
    proj = HC.projection_vectors([(k, tuple(g64[k].shape)) for k in gemm])
    out[which + "/full_names"], out[which + "/gemm_names"] = np.array(full), np.array(gemm)
    for k in full:
        out["%s/grad/%s" % (which, k)] = g64[k].numpy()
    out[which + "/gemm_norm"] = np.array([float(g64[k].norm()) for k in gemm])
    out[which + "/gemm_proj"] = np.array([float((g64[k] * proj[k]).sum()) for k in gemm])
    for tag, rounded in (("fp32", False), ("bf16", True)):
        m = make(which)
        if rounded:
            HC.round_operands_to_bf16(m)
        fy, gy, noney = HC.run_net(m, x, cots, torch.float32)
        assert noney == none64
        out["%s/feat_dev_%s" % (which, tag)] = np.array([HC.deviation(a, b) for a, b in zip(fy, f64)])
        out["%s/full_dev_%s" % (which, tag)] = np.array([HC.deviation(gy[k], g64[k]) for k in full])
        out["%s/gemm_dev_%s" % (which, tag)] = np.array([float((gy[k].double() - g64[k]).norm()) for k in gemm])
        print(which, tag, "feature deviations", out["%s/feat_dev_%s" % (which, tag)].tolist())


def main():
    out = {}
    for which in HC.NETS:
        gen_net(which, out)
    torch.manual_seed(HC.INIT_SEED)
    m = ref.convnext_tiny(in_chans=6)
    sd = m.state_dict()
    out["init/keys"] = np.array(list(sd))
    out["init/sums"] = np.array([float(v.double().sum()) for v in sd.values()])
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")
    assert os.path.getsize(GOLD) < (1 << 20)


if __name__ == "__main__":
    main()
