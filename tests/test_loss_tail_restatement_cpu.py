"""tests/helpers_loss_tail.py held against the oracle (float64, 1e-12), the conditions its smoothness inputs must
meet, and the branch every case of tests/test_loss_tail_gpu.py is meant to take, from the restated host arithmetic.
No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fsnet_oracle as O
from tests import helpers_loss_tail as T

F32, F64 = torch.float32, torch.float64


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------- smoothness
@pytest.mark.parametrize("name", [c[0] for c in T.SMOOTH_CASES])
@pytest.mark.parametrize("gout", [None, 0.37])
def test_smooth_terms_equal_the_oracle(name, gout):
    B, hw, sids, disps, colors, _ = T.smooth_case(name)
    S = len(hw)
    terms = T.smooth_terms(disps, colors, sids, gout)
    for s in range(S):
        d = disps[s].double().requires_grad_(True)
        mean = d.mean(2, True).mean(3, True)
        sm = O.smooth_loss(d / (mean + 1e-7), colors[s].double()) * 1e-5 / (2 ** sids[s])
        (sm * (1.0 if gout is None else gout) / S).backward()
        t = terms[s]
        sm = sm.detach()
        assert abs(float(t["loss"]) - float(sm)) <= 1e-12 * abs(float(sm))
        assert rel(t["d_disp"], d.grad) <= 1e-12
        assert rel(t["disp_sum"], d.detach().sum((1, 2, 3))) <= 1e-12
        h, w = hw[s]
        again = (t["sx_sum"].sum() / (B * h * (w - 1)) + t["sy_sum"].sum() / (B * (h - 1) * w)) * 1e-5 / 2 ** sids[s]
        assert abs(float(again) - float(sm)) <= 1e-12 * abs(float(sm))


def _oracle_chain(disp_only):
    """the batch of test_photometric_chain_vs_oracle_no_mask; disp_only: the depth gradient of the smoothness terms
    alone (depth -> disp -> smooth_loss), else of the whole loss"""
    B, H, W = 2, 32, 64
    data = O.synthetic_batch(B, H, W, seed=8)
    del data["patched_mask"]
    g = torch.Generator().manual_seed(4)
    outputs, leaves = {}, {}
    for s in range(4):
        d = (3 + 20 * torch.rand(B, 1, H >> s, W >> s, generator=g)).requires_grad_(True)
        leaves[s] = d
        outputs[("depth", s, s)] = d
        outputs[("disp", s)] = O.depth_to_disp(d, 0.5, 100.0)
    for f in (1, -1):
        outputs[("cam_T_cam", f)] = data[("relative_pose", f)]
    total, ld = O.photometric_loss(outputs, data)
    if disp_only:
        img, total = data[("original_image", 0)], 0
        for s in range(4):
            disp = outputs[("disp", s)]
            color = img if s == 0 else F.adaptive_avg_pool2d(img, disp.shape[2:])
            total = total + O.smooth_loss(disp / (disp.mean(2, True).mean(3, True) + 1e-7), color) * 1e-5 / 2 ** s / 4
    total.backward()
    return data, outputs, ld, [leaves[s].grad for s in range(4)]


def test_smooth_loss_per_scale_equals_the_oracles_report():
    """smooth_terms(float64) against `smooth_loss/s` of O.photometric_loss, which runs in float32: means of at most
    2 * 32 * 64 products of O(1) numbers, each a handful of float32 roundings -> 2e-6 relative is ample"""
    data, outputs, ld, _ = _oracle_chain(False)
    hw = [(32 >> s, 64 >> s) for s in range(4)]
    colors = T.color_pyramid(data[("original_image", 0)], hw)
    terms = T.smooth_terms([outputs[("disp", s)] for s in range(4)], colors, [0, 1, 2, 3], None)
    for s in range(4):
        want = float(ld["smooth_loss/%d" % s])
        assert abs(float(terms[s]["loss"]) - want) <= 2e-6 * want, s


def test_old_chain_tests_cannot_see_the_smoothness_gradient():
    """the gap as a recorded fact: on the B=2, 32x64 oracle batch the smoothness-only depth gradient is below 1e-3 of
    the full gradient's norm at every scale, while the chain tests bound the relative L2 error of the sum by 2e-3 / 3e-3:
    a smoothness backward that wrote zeros would pass them"""
    _, _, _, full = _oracle_chain(False)
    _, _, _, smooth = _oracle_chain(True)
    shares = [float(smooth[s].norm() / full[s].norm()) for s in range(4)]
    print("smoothness share of the depth gradient per scale:", ["%.2e" % v for v in shares])
    assert all(0 < v < 1e-3 for v in shares), shares


@pytest.mark.parametrize("name", [c[0] for c in T.SMOOTH_CASES] + ["chain"])
def test_smoothness_inputs_meet_their_conditions(name):
    if name == "chain":
        data, _, disps = T.chain_batch()
        B, hw, sids, const_b = 2, [(32 >> s, 64 >> s) for s in range(4)], [0, 1, 2, 3], 1
        colors = T.color_pyramid(data[("original_image", 0)], hw)
    else:
        B, hw, sids, disps, colors, const_b = T.smooth_case(name)
    terms = T.smooth_terms(disps, colors, sids, None)
    for s, d in enumerate(disps):
        assert d.dtype == F32 and colors[s].dtype in (F32, F64)
        gaps = T.neighbour_gaps(d)
        vary = [b for b in range(B) if b != const_b]
        gv = gaps[vary]
        assert float(gv[gv > 0].min()) >= 1e-3, (name, s)
        share = float((gv == 0).double().mean())
        assert 0.10 <= share <= 0.50, (name, s, share)
        # equal in float64 <=> equal float32 inputs: what the kernel's sign sees as 0 is what torch.abs sees as 0
        dx = torch.cat([(d[..., :-1] == d[..., 1:]).flatten(1), (d[:, :, :-1] == d[:, :, 1:]).flatten(1)], 1)
        assert torch.equal(dx, gaps == 0)
        if const_b is not None:
            assert bool((gaps[const_b] == 0).all())
            assert bool((terms[s]["d_disp"][const_b] == 0).all())
            assert all(bool((terms[s]["d_disp"][b] != 0).any()) for b in vary)
    if name in ("c", "d"):                              # the edge weight spans e^-1 .. 1
        c = colors[0].double()
        wx = torch.exp(-(c[..., :-1] - c[..., 1:]).abs().mean(1))
        assert float(wx.min()) < 0.4 and float(wx.max()) == 1.0


def test_smoothness_grid_per_case():
    want = {"a": (1, [(1, 4, 0)]),
            "b": (1, [(1, 15, 0)]),
            # 8 blocks; 18x26 fills two and 9x13 one: six and seven whole blocks without a pixel join the block sums
            "c": (8, [(1, 1961, 0), (1, 468, 6), (1, 117, 7)]),
            # 38 blocks capped to 32: a second round of 1408 of 8192 pixels; 2x300 leaves 29 blocks empty
            "d": (32, [(2, 1408, 0), (1, 600, 29)])}
    for name, B, hw, sids, _ in T.SMOOTH_CASES:
        assert T.smooth_grid(hw) == want[name], name
    assert (96 * 100 + 255) // 256 == 38
    assert T.smooth_grid([(32, 64), (16, 32), (8, 16), (4, 8)])[0] == 8          # the chain batch


# ---------------------------------------------------------------------------------------------- sumsq
def test_sumsq_walk_per_size():
    for n in T.SUMSQ_NS:
        w = T.sumsq_walk(n)
        assert w["two"] + w["one"] + w["tail"] == n, n
    walk = {n: T.sumsq_walk(n) for n in T.SUMSQ_NS}
    for n in (1, 3):                                   # scalar tail only
        assert (walk[n]["two"], walk[n]["one"], walk[n]["tail"]) == (0, 0, n)
    assert (walk[4]["one"], walk[4]["tail"]) == (4, 0)
    assert (walk[5]["one"], walk[5]["tail"]) == (4, 1)
    assert (walk[1023]["two"], walk[1023]["one"], walk[1023]["tail"]) == (0, 1020, 3)
    assert (walk[4101]["two"], walk[4101]["one"], walk[4101]["tail"]) == (0, 4100, 1) and walk[4101]["blocks"] == 6
    for n in T.SUMSQ_NS[:6]:
        assert walk[n]["blocks"] < 512 and walk[n]["two"] == 0        # below the cap the loop cannot run
    # the 512-block cap binds: stride 524288.  524292: exactly one thread has both loads in range
    w = walk[524292]
    assert w["blocks"] == 512 and (w["threads_two"], w["two"], w["one"], w["tail"]) == (1, 8, 524284, 0)
    # 2 * 524288 + 5: every thread once through the two-in-flight loop; thread 0 goes on to the single loop and
    # thread 1 to the tail
    w = walk[2 * 524288 + 5]
    assert w["threads_two"] == w["threads"] == 131072 and (w["two"], w["one"], w["tail"]) == (2 * 524288, 4, 1)
    # 3 * 524288 + 1027: every thread through the two-in-flight loop, the first 256 of them twice; the other 130816
    # once through the single loop, and thread 256 on to a tail of three
    w = walk[3 * 524288 + 1027]
    assert w["threads_two"] == w["threads"] and w["threads_one"] == w["threads"] - 256
    assert (w["two"], w["one"], w["tail"], w["threads_tail"]) == (2 * 524288 + 2048, 524288 - 1024, 3, 1)
    assert max(T.SUMSQ_NS) * 4 < 7 * 2 ** 20


# ---------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("K", T.HEAD_KS)
def test_head_equals_the_oracle(K):
    g = torch.Generator().manual_seed(K)
    n, h, w = T.HEAD_SINGLE
    M = n * h * w
    logits = T.head_logits(g, M, K, K + 4)[:, :K]
    bins = O.depth_bins(T.MIN_D, T.MAX_D, K).float()
    assert bins.shape == (K,)
    gd, gp = torch.randn(M, generator=g).double(), torch.randn(M, generator=g).double()
    lr = logits.double().t().reshape(1, K, M, 1).clone().requires_grad_(True)          # the oracle's [B, K, h, w]
    d = O.gather_activation(lr, bins.double())
    dp = O.depth_to_disp(d, T.MIN_D, T.MAX_D)
    (d.flatten() * gd + dp.flatten() * gp).sum().backward()
    depth, disp, dl = T.head(logits, bins, None, T.MIN_D, T.MAX_D, gd, gp)
    assert rel(depth, d.detach().flatten()) <= 1e-12 and rel(disp, dp.detach().flatten()) <= 1e-12
    assert rel(dl, lr.grad[0, :, :, 0].t()) <= 1e-12
    # the closed interval: +-10 pass the gradient, +-10.5 and +-30 do not
    row = logits[0]
    assert bool((dl[0][(row.abs() == 10)] != 0).all()) and bool((dl[0][row.abs() > 10] == 0).all())
    assert bool((dl[1] != 0).sum() > 0)
    _, _, none = T.head(logits, bins, None, T.MIN_D, T.MAX_D)
    assert bool((none == 0).all())


def test_head_with_the_focal_scale_equals_the_oracles_decoder():
    """O.depth_decoder_forward(..., P2=, base_fx=): its logits into head(), its depth and disp out, in float64"""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in O.init_state(seed=3, with_pose=False).items()}
    pre = "head.depth_decoder."
    g = torch.Generator().manual_seed(2)
    ch = O.num_ch_enc(18)
    B = 3
    feats = [torch.randn(B, c, 32 >> i, 64 >> i, generator=g).double() for i, c in enumerate(ch)]
    P2 = T.head_P2(B).double()
    out = O.depth_decoder_forward(sd, pre, feats, T.MIN_D, T.MAX_D, P2=P2, base_fx=T.HEAD_BASE_FX)
    for s in range(4):
        lg = out[("logits", s)]
        _, K, h, w = lg.shape
        rows = lg.permute(0, 2, 3, 1).reshape(-1, K)
        sc = T.head_scale(P2, T.HEAD_BASE_FX, h * w)
        depth, disp, _ = T.head(rows, sd[pre + "depth_bins"], sc, T.MIN_D, T.MAX_D)
        assert rel(depth, out[("depth", s, s)].flatten()) <= 1e-12
        assert rel(disp, out[("disp", s)].flatten()) <= 1e-12
    assert len(set(float(v) for v in sc)) == 3


def test_head_block_ranges():
    n, h, w = T.HEAD_SINGLE
    assert T.head_blocks([n * h * w]) == [0, 1]
    Ms = [n * h * w for n, h, w in T.HEAD_MULTI]
    assert Ms == [105, 36, 12] and T.head_blocks(Ms) == [0, 1, 2, 3]          # one block per scale, three images each
    assert [M // 3 for M in Ms] == [35, 12, 4] and all(M % 3 == 0 for M in Ms)
    assert any(M % 2 for M in Ms)                                             # the reject: M % nimg != 0 with nimg = 2
    assert T.head_blocks([300, 256, 257]) == [0, 2, 3, 5]


# ---------------------------------------------------------------------------------------------- finalize, pose tail
def test_finalize_restates_the_oracles_bookkeeping():
    """loss/s = photometric mean + smooth_loss/s, total = mean over the scales; and the lane loop of the kernel is
    entered by the cases with B > 64"""
    for i, (B, hw, sids) in enumerate(T.FINALIZE_CASES):
        ls, ms, sm = T.finalize_sums(B, hw, i)
        out = T.finalize(ls, ms, sm, B, [h for h, _ in hw], [w for _, w in hw], sids)
        S = len(hw)
        for s, (h, w) in enumerate(hw):
            smooth = (sm[s, :, 0].sum() / (B * h * (w - 1)) + sm[s, :, 1].sum() / (B * (h - 1) * w)) * 1e-5 / 2 ** sids[s]
            assert abs(out[S + s] - smooth) <= 2.0 ** -22 * smooth
            assert abs(out[s] - (ls[s].sum() / (ms.sum() + 1e-6) + out[S + s])) <= 1e-15 * out[s]
        assert abs(out[2 * S] - out[:S].mean()) <= 1e-15 * out[2 * S]
    assert sorted(B for B, _, _ in T.FINALIZE_CASES) == [1, 3, 64, 65, 130]
    assert any(sids != list(range(len(sids))) for _, _, sids in T.FINALIZE_CASES)


@pytest.mark.parametrize("invert", [False, True])
def test_pose_tail_restatement(invert):
    """frame 1 and the padding channels get no gradient, frame 0's six do; angles are a few 1e-3 and never zero"""
    g = torch.Generator().manual_seed(6)
    x = T.pose_features(g, 3, 65, 16)
    dT = torch.randn(3, 4, 4, generator=g)
    aa, tr, Tm, dx = T.pose_tail(x, 2, invert, 0.01, dT)
    assert Tm.dtype == F64 and dx.dtype == F64
    ang = aa[:, 0].norm(dim=-1)
    assert float(ang.min()) > 1e-3 and float(ang.max()) < 3e-2
    assert bool((dx[:, :, 6:] == 0).all()) and bool((dx[:, :, :6] != 0).all())
    R = Tm[:, :3, :3]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max()) < 1e-6       # (the 1e-7 in the axis)
    m = x.double()[:, :, :12].mean(1) * 0.01
    assert torch.equal(aa[:, 1, 0], m[:, 6:9]) and torch.equal(tr[:, 0, 0], m[:, 3:6])
