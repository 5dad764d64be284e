"""BatchNorm + ReLU folded into the consuming convolution's operand staging (fs_bn_finalize + FsConvArgs.pro_mode +
FsWgradArgs.pro_a + the data gradient's derived ReLU mask) against the same step with the BatchNorm pass of its own
(reference: BasicBlock conv1 -> bn1 -> relu -> conv2, vision_base/networks/models/backbone/resnet.py:33-50).  Both
round the normalised activation to bf16 once, from the same bf16 convolution output: the two training steps must agree
to rounding, far inside the mixed-precision band of tests/test_model_gpu.py."""
import pytest
import torch

from oracle import fsnet_oracle as O

pytestmark = pytest.mark.gpu


def _step(dev, fold, H, W, B, groups_pose=True):
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.engine import nets
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.hip.conv import LaunchProfile
    from fsnet_amd.vision_base.utils.builder import build
    old = nets.FOLD_BN
    nets.FOLD_BN = fold
    try:
        RT.set_compute_dtype(torch.bfloat16)
        RT.tie_noise = False
        m = build(**meta_arch_cfg(H, W, with_pose=True))
        m.load_state_dict(O.init_state(seed=21, with_pose=True), strict=True)
        m = m.to(dev).train()
        m.ensure_arena()
        data = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in O.synthetic_batch(B, H, W, seed=77).items()}
        LaunchProfile.begin()
        m._arena.zero_grads()
        out = m(data, dict(epoch_num=0, global_step=0, is_training=True))
        out["loss"].backward()
        from fsnet_amd.engine.handover import HO
        HO.join_companions_final()
        LaunchProfile.end()
        kinds = [k for (k, _, _, _) in LaunchProfile.tagged]
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters()}
        bufs = {k: v.detach().float().cpu().clone() for k, v in m.named_buffers()}
        return float(out["loss"].detach()), grads, bufs, kinds
    finally:
        nets.FOLD_BN = old
        RT.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("H,W,B", [(192, 640, 12), (96, 320, 4)])
def test_folded_batchnorm_step_equals_separate_pass(dev, H, W, B):
    l0, g0, b0, k0 = _step(dev, False, H, W, B)
    l1, g1, b1, k1 = _step(dev, True, H, W, B)
    # forward: bn1 of all 8 BasicBlocks of both encoders is applied by conv2's prologue (16 passes fewer, no finalize
    # launch in their place); with the two encoders as the lanes of one pass (RT.lanes) every such launch carries both
    # networks: half the count.  (The backward's second passes stay passes: the fold of rounds 3-4 was removed.)
    from fsnet_amd.engine.runtime import RT
    per = 2 if RT.lanes else 1
    assert k0.count("bn_apply") - k1.count("bn_apply") == 16 // per, (k0.count("bn_apply"), k1.count("bn_apply"))
    assert k0.count("bn_bwd_apply") == k1.count("bn_bwd_apply")
    assert abs(l1 - l0) <= 2e-3 * abs(l0), (l0, l1)
    gmax = max(v.norm().item() for v in g0.values())
    worst, dots = 0.0, [0.0, 0.0, 0.0]
    for k in g0:
        a, b = g0[k], g1[k]
        den = a.norm().item()
        dots[0] += torch.dot(a.flatten(), b.flatten()).item(); dots[1] += den ** 2; dots[2] += b.norm().item() ** 2
        if den < 1e-5 * gmax:
            # (convolution biases in front of a BatchNorm: their true gradient is zero, what is there is rounding)
            assert b.norm().item() < 1e-4 * gmax, k
            continue
        rel = (a - b).norm().item() / den
        worst = max(worst, rel)
        cos = torch.dot(a.flatten(), b.flatten()).item() / (den * b.norm().item() + 1e-30)
        # a bf16 activation that rounds the other way can flip a ReLU decision downstream: O(1) changes of single
        # elements (DESIGN section 3, bf16 policy) — per parameter the two steps stay far closer to each other than
        # either is to the fp32 oracle (cosine > 0.8 there)
        assert cos > 0.95 and rel < 0.35, (k, cos, rel)
    assert dots[0] / (dots[1] ** 0.5 * dots[2] ** 0.5) > 0.98         # the whole gradient
    # running statistics follow the same batch statistics
    for k in b0:
        # (deep layers see inputs that differ by the flipped roundings upstream: 2 % of the buffer's scale)
        assert (b0[k] - b1[k]).abs().max().item() <= 2e-2 * b0[k].abs().max().item() + 1e-4, k
