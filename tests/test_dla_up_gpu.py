"""The mirrored DLA upsampler on the GPU (its 16 modulated deformable convolutions on the HIP kernels, fp32 compute)
against tests/golden/dla_up.npz: the reference's real classes run in f64 over the restatement of tests/helpers_dcn.py.

The bound is F * e as in tests/test_dcn_gpu.py, with e the deviation of the fp32 run of the reference classes from
their f64 run — sixteen training-mode BatchNorms over as few as eight values per channel amplify any rounding, the
yardstick's as much as the kernels'.  The fixture holds the output in full and, for every parameter and input, the f64
gradient norm n and the L2 norm d of the fp32 run's gradient deviation: | ||g|| - n | <= ||g - g64|| by the triangle
inequality, and that is held to F * d.  Measured on an MI355X (RATIO line): out 1.01 (e 9.8e-03); gradient norms worst 1.28
(dla_up.ida_0.proj_1.conv.bias — a bias in front of a BatchNorm, whose true gradient is zero: both sides hold cancellation
noise), median 0.17.  F is twice that, rounded up."""
import os

import numpy as np
import pytest
import torch

from tests import helpers_dcn as HD

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dla_up.npz")
FACTOR = {"out": 3, "grad": 3}


def test_dla_upsampler_against_reference_classes(dev):
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.models.backbone.dla_utils import DLASegUpsample
    gold = np.load(GOLD)
    before = RT.compute_dtype
    RT.set_compute_dtype("fp32")
    try:
        m = DLASegUpsample(**dict(HD.DLA_UP, input_channels=list(HD.DLA_UP["input_channels"])))
        assert list(m.state_dict()) == [str(k) for k in gold["keys"]]
        m.load_state_dict(HD.dla_up_state(m), strict=True)
        pyramid, cot = HD.dla_up_inputs()
        out, grads = HD.dla_up_run(m, pyramid, cot, torch.float32, device=dev)
        torch.cuda.synchronize()
    finally:
        RT.set_compute_dtype(before)
    want = torch.from_numpy(gold["out"])
    e_max, e_rms = HD.deviation(torch.from_numpy(gold["out_fp32"]), want)
    d_max, d_rms = HD.deviation(out.cpu(), want)
    r_out = max(d_max / e_max, d_rms / e_rms)
    names = [str(k) for k in gold["grad_names"]]
    assert sorted(grads) == names
    r_grad = {}
    for k, n, d in zip(names, gold["grad_norm"], gold["grad_fp32_dev"]):
        assert bool(torch.isfinite(grads[k]).all()), k
        r_grad[k] = abs(float(grads[k].double().norm()) - float(n)) / float(d)
    worst = max(r_grad, key=r_grad.get)
    print("RATIO dla_up fp32 out %.2f (e %.1e) grad-norm worst %.2f (%s) median %.2f" % (
        r_out, e_max, r_grad[worst], worst, float(np.median(list(r_grad.values())))))
    assert r_out <= FACTOR["out"], (r_out, e_max)
    bad = {k: v for k, v in r_grad.items() if not v <= FACTOR["grad"]}
    assert not bad, bad
