"""Pins tests/helpers_photo64.py (the float64 restatement of the fused photometric chain) before a GPU test relies on it:
against the fp32 oracle, against the real reference's recorded losses and gradients, against F.grid_sample in f64,
and the conditions under which the strip-seam sweep's comparisons mean something, for every input of that sweep."""
import os

import numpy as np
import pytest
import torch

from oracle import fsnet_oracle as O
from tests import helpers_photo64 as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_shape_lists_reach_every_seam():
    hs, ws = [h for h, _ in P.SHAPES_B], [w for _, w in P.SHAPES_B]
    assert all(hs.count(h) >= 2 for h in P.HS_B) and all(ws.count(w) >= 2 for w in P.WS_B)
    assert 28 <= len(P.SHAPES_B) <= 32 and set(hs) == set(P.HS_B) and set(ws) == set(P.WS_B)
    # a one-column / one-row last strip: forward 62 x 16, backward 60 x 32
    assert {63, 125} <= {w for w in ws if w % 62 == 1} and {61, 121} <= {w for w in ws if w % 60 == 1}
    assert 17 in hs and 33 in hs and (33, 61) in P.SHAPES_B and (17, 125) in P.SHAPES_B and (33, 125) in P.SHAPES_B
    assert len(set(P.SHAPES_B)) == len(P.SHAPES_B)
    assert all(H % 8 == 0 and W % 8 == 0 for H, W, _ in P.SHAPES_A)
    assert len(set(P.ALL_NAMES)) == len(P.ALL_NAMES)


def _oracle_case(data, depths, Ts):
    return dict(B=data["P2"].shape[0], H=depths[0].shape[2], W=depths[0].shape[3],
                maps=tuple(tuple(d.shape[2:]) for d in depths),
                img0=data[("original_image", 0)].numpy(), src=[data[("original_image", 1)].numpy(), data[("original_image", -1)].numpy()],
                depths=[d.detach().numpy() for d in depths], P2=data["P2"].numpy(), T=[t.detach().numpy() for t in Ts],
                patched_mask=data["patched_mask"].numpy(), motion_mask=None)


def test_fp32_helper_vs_oracle_on_synthetic_batch():
    B, H, W = 2, 32, 64
    data = O.synthetic_batch(B, H, W, seed=8)
    g = torch.Generator().manual_seed(4)
    outputs, leaves = {}, []
    for s in range(4):
        d = (3 + 20 * torch.rand(B, 1, H >> s, W >> s, generator=g)).requires_grad_(True)
        leaves.append(d)
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = O.depth_to_disp(d.detach(), 0.5, 100.0)       # (detached: no smoothness gradient)
    Ts = [data[("relative_pose", 1)], data[("relative_pose", -1)]]
    outputs[("cam_T_cam", 1)], outputs[("cam_T_cam", -1)] = Ts
    total, ld = O.photometric_loss(outputs, data)
    total.backward()
    case = _oracle_case(data, leaves, Ts)
    r = P.photo_chain(case, dtype=torch.float32)
    denom = float(data["patched_mask"].sum()) + 1e-6
    for s in range(4):
        want = float(ld["loss/%d" % s]) - float(ld["smooth_loss/%d" % s])
        got = float(r["loss_sums"][s].sum()) / denom
        print("scale %d: loss %.8f oracle %.8f" % (s, got, want))
        assert abs(got - want) < 1e-6
        for f, fid in enumerate((1, -1)):
            d = (r["pred"][s][f] - outputs[("original_image", fid, s)].detach()).abs().max()
            assert float(d) < 2e-5, (s, f, float(d))
        two = torch.topk(r["cand"][s], 2, dim=1, largest=False)[0]
        differ = (r["argmin"][s] != outputs[("min_idx", s)]) & ((two[:, 1] - two[:, 0]) >= 1e-5)
        assert not bool(differ.any()), s
        rel = float((r["g_depth"][s].float() - leaves[s].grad).norm() / leaves[s].grad.norm())
        print("scale %d: depth gradient rel-L2 %.2e" % (s, rel))
        assert rel < 2e-3, (s, rel)


def test_f64_helper_vs_reference_golden():
    g = np.load(os.path.join(GOLD, "loss_chain.npz"))
    T_ = lambda a: torch.from_numpy(np.asarray(a))
    data = {("original_image", 0): T_(g["img_0"]), ("original_image", 1): T_(g["img_p"]),
            ("original_image", -1): T_(g["img_m"]), "P2": T_(g["P2"]), "patched_mask": T_(g["patched_mask"])}
    depths = [T_(g["depth_%d" % s]) for s in range(4)]
    Ts = [O.transformation_from_parameters(T_(g["aa_" + tag]), T_(g["tr_" + tag]), invert=(f < 0))
          for f, tag in ((1, "p"), (-1, "m"))]
    r = P.photo_chain(_oracle_case(data, depths, Ts))
    denom = float(data["patched_mask"].sum()) + 1e-6
    img0 = data[("original_image", 0)]
    for s in range(4):
        got = float(r["loss_sums"][s].sum()) / denom + float(g["ld_smooth_loss_%d" % s])
        assert abs(got - float(g["ld_loss_%d" % s])) < 1e-6, s
        # the recorded depth gradient includes the smoothness path through the disparity
        d = depths[s].clone().requires_grad_(True)
        disp = O.depth_to_disp(d, 0.5, 100.0)
        color = img0 if s == 0 else torch.nn.functional.adaptive_avg_pool2d(img0, disp.shape[2:])
        sm = O.smooth_loss(disp / (disp.mean(2, True).mean(3, True) + 1e-7), color) * 1e-5 / (2 ** s)
        (sm / 4).backward()
        ref = T_(g["gdepth_%d" % s])
        rel = float((r["g_depth"][s].float() + d.grad - ref).norm() / ref.norm())
        print("scale %d: gdepth rel-L2 %.2e" % (s, rel))
        assert rel < 3e-3, (s, rel)


@pytest.mark.parametrize("name", ["a-40x128-B2", "c-33x61", "c-20x70", "d-32x120-motion_mask"])
def test_sigma_zero_is_grid_sample(name):
    case, opts = P.case_named(name)
    a, b = P.photo_chain(case, **opts), P.photo_chain(case, sampler="grid_sample", **opts)
    S = len(case["maps"])
    for s in range(S):
        for k in ("cand", "pred", "g_depth", "g_up"):
            x, y = a[k][s], b[k][s]
            fin = torch.isfinite(x)
            assert bool((fin == torch.isfinite(y)).all()) and float((x[fin] - y[fin]).abs().max()) <= 1e-12, (s, k)
        assert bool((a["argmin"][s] == b["argmin"][s]).all())
    assert float((a["loss_sums"] - b["loss_sums"]).abs().max()) <= 1e-12 * float(a["loss_sums"].abs().max())
    for f in range(2):
        assert float((a["dT"][f] - b["dT"][f]).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", P.ALL_NAMES)
def test_sweep_inputs_meet_the_conditions(name):
    case, opts = P.case_named(name)
    y = P.yardsticks(case, opts)
    assert P.check_conditions(case, opts, y) == []
    for key in ("img0", "src"):
        for a in ([case[key]] if key == "img0" else case[key]):
            assert a.min() >= 0.0 and a.max() <= 1.0
    assert all(d.min() >= 3.0 and d.max() <= 23.0 for d in case["depths"])
    assert 0.6 < case["patched_mask"].mean() < 0.8 or case["patched_mask"].size < 200
