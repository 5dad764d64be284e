"""CPU checks of the matching encoder (ResnetEncoderMatching): state_dict against the list recorded from the reference,
depth bins, the host form of match_features and the small methods against tests/golden/matching_*.npz, the new entry
point's declaration, and the registry path."""
import json
import os

import numpy as np
import pytest
import torch

from fsnet_amd.monodepth.networks.models.backbone.resnet_matching import ResnetEncoderMatching
from tests import helpers_matching as HM
from tests.test_abi import ctype_of, declared_functions

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAME = "fsnet_amd.monodepth.networks.models.backbone.resnet_matching.ResnetEncoderMatching"


def module(**kw):
    m = HM.MODULE
    args = dict(min_depth_bin=HM.MIN_BIN, max_depth_bin=HM.MAX_BIN, num_depth_bins=m["D"])
    args.update(kw)
    return ResnetEncoderMatching(m["depth"], False, m["H"], m["W"], **args)


def test_state_dict_equals_the_reference_list():
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    m = module()
    sd = m.state_dict()
    assert len(sd) == 124
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["shapes"]))
    for k in ("layer0.0.weight", "layer0.1.running_var", "layer1.1.0.conv1.weight", "layer4.1.bn2.bias",
              "prematching_conv.0.bias", "reduce_conv.0.weight"):
        assert k in sd
    m.load_state_dict(HM.init_state(sd, seed=11), strict=True)
    assert [k for k, _ in m.named_parameters() if k not in g["grad_names"]] == ["prematching_conv.0.weight",
                                                                                "prematching_conv.0.bias"]


def test_batchnorm_modes_follow_the_reference():
    g = np.load(os.path.join(GOLD, "matching_module.npz"))
    m = module()
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(bns) == 20
    assert all(b.training == bool(g["bn_training_after_init"]) for b in bns) and not bns[0].training
    m.train()
    assert all(b.training == bool(g["bn_training_after_train"]) for b in bns) and bns[0].training
    m.eval()
    assert not any(b.training for b in bns)


def test_num_ch_enc_and_reduce_conv_width():
    assert list(module().num_ch_enc) == [64, 64, 128, 256, 512]
    m50 = ResnetEncoderMatching(50, False, 64, 96, num_depth_bins=8)
    assert list(m50.num_ch_enc) == [64, 256, 512, 1024, 2048]
    assert tuple(m50.reduce_conv[0].weight.shape) == (256, 264, 3, 3)
    assert tuple(m50.prematching_conv[0].weight.shape) == (16, 64, 1, 1)


@pytest.mark.parametrize("binning", ["linear", "inverse"])
def test_depth_bins_and_adaptive_bins(binning):
    g = np.load(os.path.join(GOLD, "matching_bins.npz"))
    m = ResnetEncoderMatching(18, False, 64, 96, min_depth_bin=HM.MIN_BIN, max_depth_bin=HM.MAX_BIN, num_depth_bins=96,
                              depth_binning=binning)
    assert m.depth_bins.dtype == torch.float32 and np.array_equal(m.depth_bins.numpy(), g[binning])
    assert tuple(m.warp_depths.shape) == (96, 1, 16, 24) and torch.equal(m.warp_depths[:, 0, 3, 5], m.depth_bins)
    idx = torch.arange(96).view(1, 8, 12) % 96
    assert np.array_equal(m.indices_to_disparity(idx).numpy(), g[binning + "_disp"])
    held = m.depth_bins
    m.adaptive_bins = True
    m.compute_depth_bins(0.9, 33.0)
    assert m.depth_bins is held, "adaptive bins are written into the same tensor"
    assert np.array_equal(m.depth_bins.numpy(), g[binning + "_adaptive"])
    assert torch.equal(m.warp_depths[:, 0, 0, 0], m.depth_bins)


def test_unknown_binning_raises():
    with pytest.raises(NotImplementedError):
        ResnetEncoderMatching(18, False, 64, 96, depth_binning="log")


@pytest.mark.parametrize("name", sorted(HM.OP_CASES))
def test_host_match_features_equals_golden(name):
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES[name]
    g = np.load(os.path.join(GOLD, "matching_op_%s.npz" % name))
    inp = HM.op_inputs(name)
    assert abs(float(inp["cur"].double().sum()) - float(g["cur_sum"])) < 1e-6 * abs(float(g["cur_sum"]))
    assert abs(float(inp["look"].double().sum()) - float(g["look_sum"])) < 1e-6 * abs(float(g["look_sum"]))
    m = ResnetEncoderMatching(18, False, 4 * h, 4 * w, min_depth_bin=near, max_depth_bin=HM.MAX_BIN, num_depth_bins=D,
                              depth_binning=binning)
    assert np.array_equal(m.depth_bins.numpy(), g["bins"])
    cost, missing = m.match_features(inp["cur"], inp["look"], inp["poses"], inp["P2"])
    assert tuple(cost.shape) == (B, D, h, w) and cost.dtype == torch.float32
    miss_ref = torch.from_numpy(g["missing"].astype(np.float32))
    differ = missing != miss_ref
    assert int(differ.sum()) <= 1e-3 * differ.numel()
    e = float(g["e"])
    dev = (cost.double() - torch.from_numpy(g["cost_f64"]))[~differ].abs().max()
    print("case %s: host form vs f64 %.3e, reference's own e %.3e" % (name, float(dev), e))
    assert float(dev) <= 4 * e
    conf = m.compute_confidence_mask(cost * (1 - missing))
    assert int((conf != torch.from_numpy(g["confidence"].astype(np.float32))).sum()) <= 1e-3 * conf.numel()
    assert torch.equal(m.compute_confidence_mask(cost * (1 - missing), num_bins_threshold=D + 1), torch.zeros_like(conf))
    viz = cost.clone()
    viz[viz == 0] = 100
    argmin = viz.min(1)[1]
    same = argmin == torch.from_numpy(g["argmin"].astype(np.int64))
    assert int((~same).sum()) <= 1e-3 * same.numel()
    lowest = m.indices_to_disparity(argmin)
    assert torch.equal(lowest[same], torch.from_numpy(g["lowest_cost"])[same])


def test_zero_pose_frame_is_skipped_on_the_host_form():
    h, w, D, C, B, F, binning, zero, near = HM.OP_CASES["a"]
    inp = HM.op_inputs("a")
    m = ResnetEncoderMatching(18, False, 4 * h, 4 * w, min_depth_bin=near, max_depth_bin=HM.MAX_BIN, num_depth_bins=D)
    both, _ = m.match_features(inp["cur"], inp["look"], inp["poses"], inp["P2"])
    one, _ = m.match_features(inp["cur"][1:], inp["look"][1:, :1], inp["poses"][1:, :1], inp["P2"][1:])
    assert torch.equal(both[1], one[0])


def test_entry_point_is_declared_with_matching_arguments():
    from fsnet_amd.hip.signatures import SIGNATURES
    fns = declared_functions()
    assert "fs_cost_volume" in fns and "fs_cost_volume" in SIGNATURES
    ret, args = fns["fs_cost_volume"]
    res, argtypes = SIGNATURES["fs_cost_volume"]
    assert ret == "int" and len(args) == len(argtypes) == 20
    for decl, ct in zip(args, argtypes):
        ty = decl.rsplit(" ", 1)[0]
        assert ctype_of(ty) == ct, (decl, ct)
    from fsnet_amd.hip import lib, ops
    assert lib.fs_cost_volume(*([None] * 11 + [1, 1, 8, 8, 64, 8, 72, 0, None])) == 1      # FS_EINVAL without a launch
    assert callable(ops.cost_volume)


def test_binding_refuses_shapes_outside_the_contract():
    from fsnet_amd.hip import ops
    B, F, h, w = 1, 1, 8, 8
    K = torch.eye(4).repeat(B, 1, 1)
    poses = torch.eye(4).repeat(B, F, 1, 1)

    def call(C=64, D=8, hh=h, ww=w):
        cur = torch.zeros(B, hh, ww, C)
        return ops.cost_volume(cur, torch.zeros(B * F, hh, ww, C), K, K, poses, torch.ones(D), torch.zeros(B, hh, ww, C + D))
    for kw in (dict(C=40), dict(D=129), dict(hh=4), dict(ww=4)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        ops.cost_volume(torch.zeros(B, h, w, 64), torch.zeros(B, h, w, 64), K, K, torch.zeros(B, 0, 4, 4), torch.ones(8),
                        torch.zeros(B, h, w, 72))


def test_registry_builds_the_class_and_module_moves_return_self():
    from fsnet_amd.vision_base.utils.builder import build
    m = build(name=NAME, depth=18, pretrained=False, input_height=64, input_width=96, num_depth_bins=8)
    assert isinstance(m, ResnetEncoderMatching) and m.matching_height == 16 and m.matching_width == 24
    assert m.cpu() is m and m.to("cpu") is m and not m.is_cuda
    assert m.set_missing_to_max and not m.adaptive_bins and m.depth_binning == "linear"
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 96), torch.zeros(1, 1, 3, 64, 96), torch.eye(4).view(1, 1, 4, 4), torch.zeros(1, 3, 4))
