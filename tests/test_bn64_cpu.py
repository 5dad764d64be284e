"""tests/helpers_bn64.py held to account without a GPU: the float64 restatement equals torch's batch_norm (+ add, + relu,
+ replicate padding) and its autograd in float64 to 1e-12; the case list of tests/test_bn_paths_gpu.py reaches every
branch of csrc/bn.hip's launch decisions (asserted from launch_paths, so a case removed later fails here); and the
activation handed to the backward kernels keeps the reference's ReLU mask exactly."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_bn64 as B

SMALL = [c for c in B.CASES if not c.large]


def close(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-12 * scale, what


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def torch_chain(c, d):
    """the same case through torch.nn.functional in float64: G module calls in a row; a SyncBN world of two identical
    shards as one batch of both"""
    rep = 2 if c.sync else 1
    G, C = c.G, c.C

    def run_bn(x, p):
        rm, rv = p["running_mean"].clone(), p["running_var"].clone()
        xs, outs, gams, bets = [], [], [], []
        for xg in x.reshape(G, -1, c.H, c.W, C):
            xl = torch.cat([xg] * rep).clone().requires_grad_(True)
            gam, bet = p["gamma"].clone().requires_grad_(True), p["beta"].clone().requires_grad_(True)
            outs.append(nhwc(F.batch_norm(nchw(xl), rm, rv, gam, bet, training=c.train, momentum=B.MOM, eps=B.EPS)))
            xs.append(xl); gams.append(gam); bets.append(bet)
        return dict(x=xs, out=outs, gamma=gams, beta=bets, rm=rm, rv=rv)
    t1 = run_bn(d["x"], d["bn"])
    t2 = None
    pre = t1["out"]
    rs = None
    if c.res == "bn2":
        t2 = run_bn(d["res"], d["bn2"])
        pre = [a + b for a, b in zip(t1["out"], t2["out"])]
    elif c.res == "res":
        rs = [torch.cat([r] * rep).clone().requires_grad_(True) for r in d["res"].reshape(G, -1, c.H, c.W, C)]
        pre = [a + r for a, r in zip(pre, rs)]
    for p_ in pre:
        p_.retain_grad()
    y = [F.relu(p_) if c.relu else p_ for p_ in pre]
    if c.pad:
        y = [nhwc(F.pad(nchw(v), (1, 1, 1, 1), mode="replicate")) for v in y]
    return t1, t2, rs, pre, y


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_restatement_equals_torch_float64(case):
    c = case
    d, fw, bw, bw2 = B.reference(c)
    t1, t2, rs, pre, y = torch_chain(c, d)
    n = c.N // c.G                                            # images of a group (of its first shard)
    close(fw["y"], torch.cat([v[:n] for v in y]).detach(), "y")
    for k, t in ((fw["bn"], t1), (fw["bn2"], t2)):
        if t is None:
            continue
        close(k["running_mean"], t["rm"], "running_mean")
        close(k["running_var"], t["rv"], "running_var")
        assert k["nbt"] == (c.G if c.train else 0)
        if c.train:
            xs = torch.stack([v.detach().reshape(-1, c.C) for v in t["x"]])
            close(k["mean"], xs.mean(1), "save_mean")
            close(k["invstd"], (xs.var(1, unbiased=False) + B.EPS).rsqrt(), "save_invstd")
        # (the affine form the consumers of fs_bn_finalize apply)
        x0 = torch.stack([v.detach()[:n].reshape(-1, c.C) for v in t["x"]])
        close(x0 * k["scale"][:, None] + k["shift"][:, None], torch.stack([v.detach()[:n].reshape(-1, c.C) for v in t["out"]]), "scale/shift")
    if not c.backward:
        return
    douts = d["dout"].reshape((c.G, n) + tuple(d["dout"].shape[1:]))
    for v, g in zip(y, douts):
        v.backward(torch.cat([g] * (2 if c.sync else 1)))
    close(bw["g"], torch.cat([p_.grad[:n] for p_ in pre]), "g_out")
    close(bw["dx"], torch.cat([v.grad[:n] for v in t1["x"]]), "dx")
    world = 2.0 if c.sync else 1.0
    close(bw["sums"][:, 0], torch.stack([v.grad for v in t1["beta"]]) / world, "sum g")
    close(bw["sums"][:, 1], torch.stack([v.grad for v in t1["gamma"]]) / world, "sum g xhat")
    close(bw["dgamma"], d["dgamma0"] + sum(v.grad for v in t1["gamma"]) / world, "dgamma")
    close(bw["dbeta"], d["dbeta0"] + sum(v.grad for v in t1["beta"]) / world, "dbeta")
    if rs is not None:
        close(bw["g"], torch.cat([r.grad[:n] for r in rs]), "residual gradient")
    if t2 is not None:
        # (the second BatchNorm's backward starts from g_out as stored: its reference gradient is that rounded tensor)
        t1b, t2b, _, preb, yb = torch_chain(c, d)
        for p_, g in zip(preb, bw2["gin"].reshape((c.G, n) + tuple(bw2["gin"].shape[1:]))):
            p_.backward(g)
        close(bw2["dx"], torch.cat([v.grad[:n] for v in t2b["x"]]), "dx2")
        close(bw2["dgamma"], sum(v.grad for v in t2b["gamma"]), "dgamma2")
        close(bw2["dbeta"], sum(v.grad for v in t2b["beta"]), "dbeta2")


def test_fold_is_the_adjoint_of_replicate_padding():
    g = torch.Generator().manual_seed(3)
    for H, W in ((2, 2), (7, 2), (2, 5), (4, 6)):
        v = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64, requires_grad=True)
        dp = torch.randn(2, H + 2, W + 2, 3, generator=g, dtype=torch.float64)
        nhwc(F.pad(nchw(v), (1, 1, 1, 1), mode="replicate")).backward(dp)
        close(B.fold_border(dp), v.grad, (H, W))


def test_folded_gradients_are_exact_in_fp32():
    """the precondition of comparing g_out bit for bit: the padded gradients are chosen so that no fp32 addition of the
    fold rounds, whatever its order"""
    for c in B.CASES:
        if c.pad:
            d = B.make_inputs(c)
            assert B.exact_f32(d["dout"]) and bool((B.rnd(d["dout"], "bf16") == d["dout"]).all())
            assert float(d["dout"].abs().max()) * 4 * 32 < 2 ** 24 and bool((d["dout"] * 32 == (d["dout"] * 32).round()).all())


def test_mask_guard():
    """every backward case: rounding the reference activation to the storage type changes the sign of no element (zero stays
    zero, positive stays positive), so the kernels' mask is the reference's and no element is left out of a comparison"""
    n = 0
    for c in B.CASES:
        if not (c.backward and c.relu):
            continue
        d = B.make_inputs(c)
        y = B.forward_reference(c, d)["y"]
        act = B.rnd(y, c.dtype)
        assert bool(((y > 0) == (act > 0)).all()) and bool(((y == 0) == (act == 0)).all()), c.id
        assert bool((y > 0).any()) and bool((y == 0).any()), c.id
        n += 1
    assert n >= 60


# ---------------------------------------------------------------------------------------------------------------------
# coverage of csrc/bn.hip's launch decisions by the case list
# ---------------------------------------------------------------------------------------------------------------------
def paths_where(pred):
    return [(c, p) for c in B.CASES for p in [c.paths()] if pred(c, p)]


def test_launch_paths_reference_points():
    """launch_paths against launches worked out by hand from bn.hip"""
    p = B.launch_paths(64, "bf16", 36 * 96 * 320)            # the stem's width: 8 lanes, 512-block cap
    assert (p["lanes"], p["slabs"], p["ew_grid"], p["cgb"], p["pixel_lanes"], p["red_grid"]) == (8, 1, (512, 1, 1), 8, 32, (1024, 1, 1))
    assert p["fwd_fast"] and p["bwd_fast"] and p["ring"] and not p["half_active"]
    p = B.launch_paths(2048, "bf16", 640)                     # ResNet-50 layer 4: 256 lanes in 8 slabs, grid cap 64
    assert (p["lanes"], p["slabs"], p["ew_grid"], p["fwd_lds"], p["bwd_lds"]) == (256, 8, (64, 8, 1), 2048, 5120)
    assert (p["cgb"], p["red_cap"], p["red_grid"]) == (32, 128, (40, 8, 1))
    p = B.launch_paths(24, "f32", 420, dense_y=False)         # 6 lanes: divisions, CGB 4 with two idle lanes
    assert (p["lanes"], p["pow2"], p["fwd_fast"], p["bwd_fast"], p["cgb"], p["half_active"]) == (6, False, False, False, 4, True)
    assert (p["ew_grid"], p["ew_min"], p["ew_max"], p["red_grid"], p["red_min"], p["red_max"]) == ((10, 1, 1), 0, 1, (4, 2, 1), 1, 2)


def test_cases_reach_every_first_pass_variant():
    bwd = paths_where(lambda c, p: c.backward)
    reach = {(p["cgb"], c.dtype) for c, p in bwd}
    assert reach == {(cgb, dt) for cgb in (2, 4, 8, 32) for dt in ("f32", "bf16")}
    # (the thin decoder and DLA widths: 16 channels bf16 and 8 at either type on <2>, 16 fp32 and 32 bf16 on <4>)
    have = {(c.C, c.dtype, p["cgb"]) for c, p in bwd}
    assert {(16, "bf16", 2), (8, "bf16", 2), (8, "f32", 2), (16, "f32", 4), (32, "bf16", 4)} <= have
    assert {p["cgb"] for c, p in bwd if p["half_active"]} >= {2, 4, 32}
    # bf16 with 3, 6 and 12 lanes; 48 lanes at both types
    assert {p["lanes"] for c, p in bwd if c.dtype == "bf16" and not p["pow2"]} >= {3, 6, 48}
    assert {(c.dtype, p["lanes"]) for c, p in bwd} >= {("bf16", 12), ("f32", 48), ("bf16", 48)}


@pytest.mark.parametrize("path", ["fwd_fast", "bwd_fast", "ring"])
def test_cases_reach_every_per_thread_count(path):
    lo, hi = ("red_min", "red_max") if path == "ring" else ("ew_min", "ew_max")
    ragged = "red_ragged" if path == "ring" else "ew_ragged"
    on = paths_where(lambda c, p: p[path] and (c.backward or path == "fwd_fast"))
    counts = set()
    for c, p in on:
        counts |= set(range(p[lo], p[hi] + 1))
    assert {0, 1, 2, 3} <= counts and max(counts) >= 4, counts
    # four rounds or more with a part-filled last one: some threads walk one round fewer
    assert any(p[hi] >= 4 and p[ragged] and p[lo] == p[hi] - 1 for c, p in on)
    # the 2 x 3 map of layer 4 at 64 x 96: threads of the ring with one row and with none
    if path == "ring":
        assert any((c.N, c.H, c.W) == (1, 2, 3) and (p[lo], p[hi]) == (0, 1) for c, p in on)


def test_cases_reach_the_generic_loops_and_slabs():
    fwd = paths_where(lambda c, p: not p["fwd_fast"])
    bwd = paths_where(lambda c, p: c.backward and not p["bwd_fast"])
    for group in (fwd, bwd):
        for dt in ("f32", "bf16"):
            lanes = {p["lanes"] for c, p in group if c.dtype == dt and not p["pow2"]}
            assert any(l > 32 for l in lanes) and any(l < 32 for l in lanes), (dt, lanes)
            assert all(p["slabs"] == 1 for c, p in group if not p["pow2"])
            # power-of-two lanes behind strides: padded and plainly strided
            assert any(p["pow2"] and c.pad for c, p in group if c.dtype == dt)
            assert any(p["pow2"] and c.strided for c, p in group if c.dtype == dt)
    slabs = {(p["slabs"], c.res == "bn2", c.train) for c, p in paths_where(lambda c, p: p["slabs"] > 1)}
    assert {(2, True, True), (2, True, False)} <= slabs and any(s >= 4 and b for s, b, _ in slabs)
    assert any(p["slabs"] >= 4 and c.backward for c, p in paths_where(lambda c, p: True))


def test_cases_cover_the_flag_combinations():
    ids = {c.id for c in B.CASES}
    assert len(ids) == len(B.CASES)
    for dt in ("f32", "bf16"):
        sel = [c for c in B.CASES if c.dtype == dt]
        assert any(c.pad and c.G > 1 for c in sel) and any(c.pad and c.res for c in sel)
        assert any(c.G == 2 and not c.pad and c.start and c.g_out for c in sel) and any(c.G == 3 and not c.pad for c in sel)
        assert any(not c.train and c.res == "bn2" for c in sel) and any(not c.train and c.res == "res" for c in sel)
        assert any(c.strided for c in sel)
    assert any(c.sync for c in B.CASES)
    large = [c for c in B.CASES if c.large]
    assert len(large) == 3 and all(c.M * c.C <= 6.5e6 for c in large)
    assert all(c.M * c.C < 100000 for c in B.CASES if not c.large)
