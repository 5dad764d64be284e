"""is_unscaled_distill on the device: the kernels against the float64 restatement (tests/helpers_distill_unscaled.py),
determinism, bounds, exactness, and the decoder / DistillWPoseMeta against the golden vectors of the REAL reference
(tests/golden/distill_unscaled.npz).

Measured on an MI355X, err / e with e = max(|fp32 restatement - float64|_max, 2^-23 max |float64|), bound 4 — the largest
over all cases, with and without uncertainty, gout in {NULL, 1.7}: loss 0.523, d_pred 1.206, d_uncertain 1.361
(DESIGN §29)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers_distill_unscaled as HU

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "distill_unscaled.npz")
GUARD = 64
MARGIN = 4.0


def _chunk():
    from fsnet_amd.hip import ops
    return ops.distill_unscaled_chunk()


def _case(name):
    return HU.case(name, _chunk() if name == "three_blocks" else None)


def _refs(name, with_unc, gout):
    return HU.references(name, _chunk() if name == "three_blocks" else None, with_unc, gout)


class _Raw:
    """the entry points on buffers of this test's own: every tensor sits `offset` floats into a NaN-filled buffer with
    GUARD elements behind it, so unwritten cells and writes past the end show"""

    def __init__(self, preds, teachers, uncs, dev, offset=0):
        from fsnet_amd.hip.binding import FsDistillUnscaledArgs
        from fsnet_amd.hip import lib
        self.S, self.dev, self.offset = len(preds), dev, offset
        self.shapes = [tuple(p.shape) for p in preds]
        self.numels = [p.numel() for p in preds]
        self.a = a = FsDistillUnscaledArgs()
        self.bufs = {}
        for key, src in (("pred", preds), ("teacher", teachers), ("uncertain", uncs), ("d_pred", preds),
                         ("d_uncertain", uncs)):
            if src is None:
                continue
            self.bufs[key] = []
            for s in range(self.S):
                buf = torch.full((offset + self.numels[s] + GUARD,), float("nan"), dtype=torch.float32, device=dev)
                if not key.startswith("d_"):
                    buf[offset:offset + self.numels[s]] = src[s].to(dev).flatten()
                self.bufs[key].append(buf)
                getattr(a, key)[s] = buf.data_ptr() + 4 * offset
        for s in range(self.S):
            a.n[s] = preds[s].shape[2] * preds[s].shape[3]
        a.planes, a.S = preds[0].shape[0] * preds[0].shape[1], self.S
        nbytes = int(lib.fs_distill_unscaled_workspace_bytes(a.planes, C.addressof(a.n), a.S))
        assert nbytes > 0
        self.ws = torch.full((nbytes // 8 + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        self.loss = torch.full((self.S + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        a.workspace, a.loss_out = self.ws.data_ptr(), self.loss.data_ptr()
        self.ws_cells = nbytes // 8

    def run(self, gout=None):
        from fsnet_amd.hip import lib
        from fsnet_amd.hip.binding import stream_ptr
        self.gout = None if gout is None else torch.full((self.S,), gout, dtype=torch.float64, device=self.dev)
        self.a.gout = None if gout is None else self.gout.data_ptr()
        assert lib.fs_distill_unscaled_fwd(C.byref(self.a), stream_ptr()) == 0
        assert lib.fs_distill_unscaled_bwd(C.byref(self.a), stream_ptr()) == 0
        torch.cuda.synchronize()
        return self

    def out(self, key, s):
        o = self.offset
        return self.bufs[key][s][o:o + self.numels[s]].view(self.shapes[s])

    def check_guards(self):
        o = self.offset
        for key, bufs in self.bufs.items():
            for s, buf in enumerate(bufs):
                assert bool(torch.isnan(buf[:o]).all()) and bool(torch.isnan(buf[o + self.numels[s]:]).all()), (key, s)
                if key.startswith("d_"):
                    assert not bool(torch.isnan(buf[o:o + self.numels[s]]).any()), (key, s, "unwritten cells")
        assert bool(torch.isnan(self.ws[self.ws_cells:]).all()) and not bool(torch.isnan(self.ws[:self.ws_cells]).any())
        assert bool(torch.isnan(self.loss[self.S:]).all()) and not bool(torch.isnan(self.loss[:self.S]).any())


def _raw(name, with_unc, dev, offset=0, scales=None):
    c = _case(name)
    idx = range(len(c["pred"])) if scales is None else scales
    return _Raw([c["pred"][s] for s in idx], [c["teacher"][s] for s in idx],
                [c["uncertain"][s] for s in idx] if with_unc else None, dev, offset)


# ---- the kernels against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gout", [None, 1.7])
@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("name", HU.ALL)
def test_kernels_against_float64(dev, name, with_unc, gout):
    r = _raw(name, with_unc, dev).run(gout)
    r.check_guards()
    refs = _refs(name, with_unc, 1.0 if gout is None else gout)
    for s, ref in enumerate(refs):
        (l32, dp32, du32), (l64, dp64, du64) = ref["f32"], ref["f64"]
        got = [("loss", r.loss[s].cpu(), l32, l64), ("d_pred", r.out("d_pred", s).cpu(), dp32, dp64)]
        if with_unc:
            got.append(("d_uncertain", r.out("d_uncertain", s).cpu(), du32, du64))
        ratios = {}
        for what, g, f32, f64 in got:
            e = HU.yardstick(f32, f64)
            ratios[what] = float((g.double() - f64).abs().max()) / e
        print("RATIO %-12s scale %d unc %d gout %-4s  " % (name, s, with_unc, gout) +
              "  ".join("%s %.3f" % kv for kv in ratios.items()))
        for what, v in ratios.items():
            assert v <= MARGIN, (name, s, what, v)


def test_ops_wrappers_equal_the_raw_entry_points(dev):
    from fsnet_amd.hip import ops
    c = _case("four_scales")
    r = _raw("four_scales", True, dev).run(1.7)
    mv = lambda xs: [x.to(dev) for x in xs]
    losses, ctx = ops.distill_unscaled_fwd(mv(c["pred"]), mv(c["teacher"]), mv(c["uncertain"]))
    dp, du = ops.distill_unscaled_bwd(ctx, torch.full((4,), 1.7, dtype=torch.float64, device=dev))
    assert losses.dtype == torch.float64 and torch.equal(losses, r.loss[:4])
    for s in range(4):
        assert torch.equal(dp[s], r.out("d_pred", s)) and torch.equal(du[s], r.out("d_uncertain", s))
    dp1, du1 = ops.distill_unscaled_bwd(ctx)                    # gouts None: ones
    r.run(None)
    assert all(torch.equal(dp1[s], r.out("d_pred", s)) for s in range(4))


@pytest.mark.parametrize("with_unc", [False, True])
def test_four_scales_in_one_launch_equal_four_launches(dev, with_unc):
    four = _raw("four_scales", with_unc, dev).run(1.7)
    for s in range(4):
        one = _raw("four_scales", with_unc, dev, scales=[s]).run(1.7)
        assert torch.equal(one.loss[:1], four.loss[s:s + 1])
        assert torch.equal(one.out("d_pred", 0), four.out("d_pred", s))
        if with_unc:
            assert torch.equal(one.out("d_uncertain", 0), four.out("d_uncertain", s))


@pytest.mark.parametrize("with_unc", [False, True])
def test_two_runs_are_bit_identical(dev, with_unc):
    a = _raw("three_blocks", with_unc, dev).run(1.7)
    b = _raw("three_blocks", with_unc, dev).run(1.7)
    assert torch.equal(a.loss[:1], b.loss[:1]) and torch.equal(a.out("d_pred", 0), b.out("d_pred", 0))
    assert torch.equal(a.ws[:a.ws_cells], b.ws[:b.ws_cells])
    if with_unc:
        assert torch.equal(a.out("d_uncertain", 0), b.out("d_uncertain", 0))


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["odd", "three_blocks", "below_wave"])
def test_unaligned_tensors_fill_their_cells_and_nothing_else(dev, name, offset):
    """every tensor starts 4, 8 or 12 bytes past a 16-byte boundary: all cells written, the guards on both sides intact,
    and the same bits as the aligned run (a thread owns the same elements on both load paths)"""
    base = _raw(name, True, dev).run(1.7)
    r = _raw(name, True, dev, offset=offset).run(1.7)
    r.check_guards()
    assert torch.equal(r.loss[:1], base.loss[:1])
    assert torch.equal(r.out("d_pred", 0), base.out("d_pred", 0))
    assert torch.equal(r.out("d_uncertain", 0), base.out("d_uncertain", 0))


# ---- exactness -----------------------------------------------------------------------------------------------------
def test_zero_prediction_gives_zero_loss_and_zero_gradient(dev):
    c = _case("odd")
    r = _Raw([torch.zeros_like(c["pred"][0])], c["teacher"], None, dev).run(1.7)
    assert float(r.loss[0]) == 0.0
    assert float(r.out("d_pred", 0).abs().max()) == 0.0


def test_a_scaled_teacher_is_matched_where_the_plain_term_is_not(dev):
    """pred = 3 teacher: ratio = 3 (1 - mean 1e-5 / (t + 1e-5)), so e_i <= 3 t_i 1e-5 / min t and the loss stays below
    1e-4 mean(pred); the plain term on the same input is mean |t - 3 t| = 2 mean(teacher)"""
    from fsnet_amd.hip import ops
    c = _case("sibling")
    t = c["teacher"][0]
    p = 3 * t
    r = _Raw([p], [t], None, dev).run()
    assert 0 <= float(r.loss[0]) < 1e-4 * float(p.double().mean())
    plain = float(ops.distill_fwd(p.to(dev), t.to(dev), None))
    assert abs(plain - 2 * float(t.double().mean())) < 1e-5 * plain


def test_invalid_arguments_launch_nothing(dev):
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import stream_ptr
    r = _raw("below_wave", True, dev)

    def refused():
        assert lib.fs_distill_unscaled_fwd(C.byref(r.a), stream_ptr()) == 1
        assert lib.fs_distill_unscaled_bwd(C.byref(r.a), stream_ptr()) == 1

    for field, bad in (("S", 0), ("S", 5), ("planes", 0)):
        keep = getattr(r.a, field)
        setattr(r.a, field, bad)
        refused()
        setattr(r.a, field, keep)
    keep, r.a.n[0] = r.a.n[0], 0
    refused()
    r.a.n[0] = keep
    for field in ("pred", "teacher", "uncertain"):
        keep = getattr(r.a, field)[0]
        getattr(r.a, field)[0] = None
        if field == "uncertain":                       # all NULL with d_uncertain set: the backward refuses
            assert lib.fs_distill_unscaled_bwd(C.byref(r.a), stream_ptr()) == 1
        else:
            refused()
        getattr(r.a, field)[0] = keep
    keep, r.a.workspace = r.a.workspace, None
    refused()
    r.a.workspace = keep
    torch.cuda.synchronize()
    for key in ("d_pred", "d_uncertain"):
        assert bool(torch.isnan(r.bufs[key][0]).all())
    assert bool(torch.isnan(r.ws).all()) and bool(torch.isnan(r.loss).all())
    r.run()                                            # the restored set is a valid one
    r.check_guards()


# ---- decoder level -------------------------------------------------------------------------------------------------
def _decoder(**flags):
    from fsnet_amd.monodepth.networks.models.heads import monodepth2_decoder as M
    dec = M.MonoDepth2Decoder.__new__(M.MonoDepth2Decoder)
    torch.nn.Module.__init__(dec)
    dec.frame_ids = [0, 1, -1]
    for k, v in flags.items():
        setattr(dec, k, v)
    return dec


@pytest.mark.parametrize("with_unc", [False, True])
def test_compute_distill_loss_returns_the_reference_values(dev, with_unc):
    g = np.load(GOLD)
    dec = _decoder(is_unscaled_distill=True, is_uncertain_distill=with_unc)
    for r, (name, s) in enumerate(HU.golden_rows()):
        c = HU.case(name)
        ref = HU.references(name, None, with_unc)[s]
        p = c["pred"][s].to(dev).requires_grad_(True)
        u = c["uncertain"][s].to(dev).requires_grad_(True)
        od = {("depth", 7, 7): p, ("teacher_depth", 7, 7): c["teacher"][s].to(dev), ("uncertain_z", 7): u}
        loss = dec.compute_distill_loss(od, {}, 7)
        assert loss.dim() == 0
        loss.backward()
        want = float(g["k_loss"][r, int(with_unc)])
        assert abs(float(loss.detach()) - want) <= MARGIN * HU.yardstick(ref["f32"][0], ref["f64"][0]) + HU.ULP * abs(want), (name, s)
        grads = [(p.grad, ref["f32"][1], ref["f64"][1])] + ([(u.grad, ref["f32"][2], ref["f64"][2])] if with_unc else [])
        assert with_unc or u.grad is None
        for k, (got, f32, f64) in enumerate(grads):
            stored = g["k_grad"][r, int(with_unc), k].astype(np.float64)
            bound = HU.digest_tolerance(got.numel(), MARGIN * HU.yardstick(f32, f64)) + HU.ULP * np.abs(stored)
            assert (np.abs(HU.digest(got.cpu()) - stored) <= bound).all(), (name, s, k)


# ---- model level ---------------------------------------------------------------------------------------------------
def _model_cfg(H, W, teacher_path=None, with_unc=True):
    from tests.test_distill_gpu import _cfg
    cfg = _cfg(H, W, teacher_path)
    cfg.head_cfg.is_unscaled_distill = True
    cfg.head_cfg.is_uncertain_distill = with_unc
    return cfg


@pytest.mark.parametrize("with_unc", [True, False])
def test_fp32_step_matches_the_reference_golden(dev, tmp_path, with_unc):
    """bounds of tests/test_distill_gpu.py for the same quantities: 3e-4 relative on the losses, 2e-2 on the gradient
    norms above 1e-3 of the largest"""
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import distill_oracle as D
    from oracle import fsnet_oracle as O
    RT.set_compute_dtype(torch.float32)
    tie, RT.tie_noise = RT.tie_noise, False
    try:
        g = np.load(GOLD)
        M = HU.MODEL
        sd = D.init_states(seed=M["seed"], teacher_seed=M["teacher_seed"])
        tpath = str(tmp_path / "teacher.pth")
        torch.save({k[len("teacher_net."):]: v.clone() for k, v in sd.items() if k.startswith("teacher_net.")}, tpath)
        m = build(**_model_cfg(M["H"], M["W"], tpath, with_unc))
        m.load_state_dict({k: v.clone() for k, v in sd.items() if not k.startswith("teacher_net.")}, strict=False)
        m = m.to(dev).train()
        data = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v)
                for k, v in O.synthetic_batch(M["B"], M["H"], M["W"], seed=M["batch_seed"]).items()}
        out = m(data, dict(is_training=True))
        out["loss"].backward()
        torch.cuda.synchronize()
        want = g["m_loss"][int(with_unc)].astype(np.float64)
        loss = float(out["loss"].detach())
        assert abs(loss - want[0]) < 3e-4 * abs(want[0]), (loss, want[0])
        for s in range(4):
            got = float(out["loss_dict"]["distilation/%d" % s])
            assert abs(got - want[1 + s]) < 3e-4 * want[1 + s], (s, got, want[1 + s])
        params = [(k, p) for k, p in m.named_parameters() if not k.startswith("teacher_net.")]
        gn = np.array([float(p.grad.norm()) if p.grad is not None else 0.0 for _, p in params])
        ref = g["m_gradnorm"][int(with_unc)].astype(np.float64)
        big = ref > 1e-3 * ref.max()
        assert np.abs(gn - ref)[big].max() / ref[big].max() < 2e-2, float(np.abs(gn - ref)[big].max() / ref[big].max())
        assert all(p.grad is None or float(p.grad.abs().max()) == 0 for p in m.teacher_net.parameters())
    finally:
        RT.tie_noise = tie


def _hook_run(dev, dtype, graph_warmup, steps=5, lr=1e-4):
    from fsnet_amd.configs import training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    from oracle import distill_oracle as D
    from oracle import fsnet_oracle as O
    RT.set_compute_dtype(dtype)
    m = build(**_model_cfg(64, 128))
    m.load_state_dict(D.init_states(seed=5, teacher_seed=6), strict=True)
    m = m.to(dev).train()
    t0 = torch.cat([p.detach().flatten().clone() for p in m.teacher_net.parameters()])
    tc = training_cfg(lr=lr)
    opt = build_optimizer(m, **tc.optimizer)
    hook = build(**dict(tc.training_hook, graph_warmup=graph_warmup))
    losses = []
    for it in range(steps):
        out = hook(dict(O.synthetic_batch(2, 64, 128, seed=9)), m, opt)
        losses.append(float(out["loss"].detach()))
    torch.cuda.synchronize()
    t1 = torch.cat([p.detach().flatten() for p in m.teacher_net.parameters()])
    assert float((t0 - t1).abs().max()) == 0.0                  # the teacher is unchanged
    return losses, hook


def test_bf16_training_steps_through_the_hook(dev):
    from fsnet_amd.engine.runtime import RT
    try:
        losses, hook = _hook_run(dev, torch.bfloat16, 2)
    finally:
        RT.set_compute_dtype(torch.float32)
    assert all(np.isfinite(l) and abs(l) < 1e4 for l in losses) and losses[-1] < losses[0], losses
    assert hook.graph_captures == 1 and hook.graph_replays == 2


def test_replayed_fp32_steps_equal_eager_ones(dev):
    """five hook steps on one batch with a learning rate of zero: the weights stay, so every step computes the same loss
    and the eager steps (the first two) stand beside the replayed ones (the last two) — 2e-5 relative, the bound of the
    fisheye step test.  (With a learning rate the steps differ, and two runs drift apart by the training dynamics, not
    by the capture: 3e-8 relative after one update grows to 1e-3 after four.)"""
    from fsnet_amd.engine.runtime import RT
    tie, RT.tie_noise = RT.tie_noise, False
    try:
        losses, hook = _hook_run(dev, torch.float32, 2, lr=0.0)
    finally:
        RT.tie_noise = tie
    print("eager / captured / replayed losses", losses)
    assert hook.graph_captures == 1 and hook.graph_replays == 2
    assert all(np.isfinite(l) for l in losses)
    for replayed in losses[3:]:
        for eager in losses[:2]:
            assert abs(eager - replayed) <= 2e-5 * abs(eager), losses
