"""is_unscaled_distill without a GPU: the helper's float32 restatement against the golden vectors of the REAL
compute_distill_loss (tests/golden/distill_unscaled.npz), the cases' distance from the kink of |x|, the option check,
and the new entry points' declarations, exports, argument checks and register use."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import helpers_distill_unscaled as HU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "distill_unscaled.npz")
SYMBOLS = ("fs_distill_unscaled_fwd", "fs_distill_unscaled_bwd", "fs_distill_unscaled_workspace_bytes",
           "fs_distill_unscaled_chunk")


def _chunk():
    from fsnet_amd.hip import lib
    return int(lib.fs_distill_unscaled_chunk())


@pytest.mark.parametrize("with_unc", [False, True])
def test_fp32_restatement_reproduces_the_reference_golden(with_unc):
    """tolerance per quantity: 4 x max(|fp32 restatement - float64|, 2^-23 max |float64|) — the restatement's own
    distance from float64; the golden digests are stored in float32, which costs the sums one more rounding"""
    g = np.load(GOLD)
    assert [HU.case(n)["seed"] for n in HU.SMALL] == list(g["k_seed"])
    for r, (name, s) in enumerate(HU.golden_rows()):
        ref = HU.references(name, None, with_unc)[s]
        (l32, dp32, du32), (l64, dp64, du64) = ref["f32"], ref["f64"]
        n = dp32.numel()
        tol = 4 * HU.yardstick(l32, l64)
        assert abs(float(l32) - float(g["k_loss"][r, int(with_unc)])) <= tol, (name, s)
        for k, (a32, a64) in enumerate(((dp32, dp64), (du32, du64))):
            want = g["k_grad"][r, int(with_unc), k].astype(np.float64)
            if a32 is None:
                assert not want.any()
                continue
            bound = HU.digest_tolerance(n, 4 * HU.yardstick(a32, a64)) + HU.ULP * np.abs(want)
            err = np.abs(HU.digest(a32) - want)
            assert (err <= bound).all(), (name, s, k, err / bound)


def test_every_case_stays_clear_of_the_kink():
    chunk = _chunk()
    for name in HU.ALL:
        c = HU.case(name, chunk if name == "three_blocks" else None)
        worst = min(HU.min_abs_x(p, t) for p, t in zip(c["pred"], c["teacher"]))
        print("case %-12s seed %d  shapes %s  min |x| %.3e" % (name, c["seed"], [tuple(p.shape) for p in c["pred"]], worst))
        assert worst >= HU.MIN_ABS_X, (name, worst)
        for p, t, u in zip(c["pred"], c["teacher"], c["uncertain"]):
            assert p.dtype == t.dtype == u.dtype == torch.float32
            assert 1 <= float(p.min()) and float(p.max()) < 51 and 1 <= float(t.min()) and float(t.max()) < 51
            assert 0.05 <= float(u.min()) and float(u.max()) < 0.95
    c = HU.case("three_blocks", chunk)
    n = c["pred"][0].shape[2] * c["pred"][0].shape[3]
    assert n == 2 * chunk + 5 and c["pred"][0].shape[0] == 2
    assert HU.case("odd")["pred"][0][0].numel() % 4 != 0          # the second plane is not 16-byte aligned


def test_the_rejected_seeds_the_issue_names_are_rejected():
    for shape in ((3, 1, 24, 40), (2, 1, 33, 127)):
        p, t, _ = HU._draw([shape], 5)[0]
        assert HU.min_abs_x(p, t) < HU.MIN_ABS_X, shape


def _decoder(cls="MonoDepth2Decoder", fids=(0, 1, -1), **flags):
    from fsnet_amd.monodepth.networks.models.heads import monodepth2_decoder as M
    dec = getattr(M, cls).__new__(getattr(M, cls))
    torch.nn.Module.__init__(dec)
    dec.frame_ids = list(fids)
    for k, v in flags.items():
        setattr(dec, k, v)
    return dec


@pytest.mark.parametrize("with_unc", [False, True])
def test_check_options_accepts_unscaled_distill(with_unc):
    _decoder(distillation_loss_weight=0.3, is_unscaled_distill=True, is_uncertain_distill=with_unc)._check_options({})


def test_pinned_refusals_still_raise():
    for cls, fids, word in (("MonoDepth2Decoder", [0, "s"], "stereo"), ("MonoDepth2Decoder", [0, 1, 1], "once"),
                            ("MonoDepth2Decoder", [0, 1, 0], "differ"),
                            ("MonoDepth2Decoder", [0, -3, -2, -1, 1, 2], "at most"), ("FishEyeDecoder", [0, -1], "two")):
        with pytest.raises(NotImplementedError) as e:
            _decoder(cls, fids, distillation_loss_weight=0.3, is_unscaled_distill=True)._check_options({})
        assert word in str(e.value)
    for flag in ("is_residual_flow", "is_light_compensate", "learnable_photometric_uncertain", "is_ssim_weight"):
        with pytest.raises(NotImplementedError):
            _decoder(is_unscaled_distill=True, **{flag: True})._check_options({})


def test_symbols_are_declared_exported_and_the_abi_stays_15():
    from fsnet_amd.hip import binding, lib
    from fsnet_amd.hip.signatures import SIGNATURES
    header = open(os.path.join(ROOT, "include", "fsnet_hip.h")).read()
    for name in SYMBOLS:
        assert name in SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(lib, name) is not None
    assert "typedef struct FsDistillUnscaledArgs" in header and hasattr(binding, "FsDistillUnscaledArgs")
    assert int(lib.fs_abi_version()) == binding.ABI_VERSION == 15
    assert re.search(r"#define FS_ABI_VERSION 15\b", header)
    chunk = _chunk()
    assert chunk >= 256 and chunk % 256 == 0
    n = (C.c_int64 * 4)(chunk, chunk + 1, 1, 3 * chunk)
    assert lib.fs_distill_unscaled_workspace_bytes(5, n, 4) == 3 * 8 * 5 * (1 + 2 + 1 + 3)
    assert lib.fs_distill_unscaled_workspace_bytes(5, n, 1) == 3 * 8 * 5
    assert lib.fs_distill_unscaled_workspace_bytes(0, n, 1) == -1 and lib.fs_distill_unscaled_workspace_bytes(1, n, 5) == -1
    n[2] = 0
    assert lib.fs_distill_unscaled_workspace_bytes(1, n, 3) == -1 and lib.fs_distill_unscaled_workspace_bytes(1, n, 2) > 0


def test_invalid_arguments_are_rejected_before_any_launch():
    """none of these reaches the device: the checks run first, and this test runs without one.  (Addresses are
    placeholders that nothing dereferences.)"""
    from fsnet_amd.hip import lib
    from fsnet_amd.hip.binding import FsDistillUnscaledArgs

    def good(S=2, unc=True):
        a = FsDistillUnscaledArgs()
        for s in range(S):
            a.pred[s], a.teacher[s], a.d_pred[s], a.n[s] = 0x1000, 0x2000, 0x3000, 15
            if unc:
                a.uncertain[s], a.d_uncertain[s] = 0x4000, 0x5000
        a.workspace, a.loss_out, a.planes, a.S = 0x6000, 0x7000, 2, S
        return a

    def both(a):
        return lib.fs_distill_unscaled_fwd(C.byref(a), None), lib.fs_distill_unscaled_bwd(C.byref(a), None)

    assert (lib.fs_distill_unscaled_fwd(None, None), lib.fs_distill_unscaled_bwd(None, None)) == (1, 1)
    for field, value in (("S", 0), ("S", 5), ("planes", 0), ("workspace", None)):
        a = good()
        setattr(a, field, value)
        assert both(a) == (1, 1), field
    for field in ("pred", "teacher"):
        a = good()
        getattr(a, field)[1] = None
        assert both(a) == (1, 1), field
    a = good()
    a.n[1] = 0
    assert both(a) == (1, 1)
    a = good()
    a.uncertain[1] = None                       # half-set uncertain
    assert both(a) == (1, 1)
    a = good()
    a.loss_out = None
    assert lib.fs_distill_unscaled_fwd(C.byref(a), None) == 1
    a = good()
    a.d_pred[0] = None
    assert lib.fs_distill_unscaled_bwd(C.byref(a), None) == 1
    a = good()
    a.d_uncertain[0] = None                     # half-set d_uncertain
    assert lib.fs_distill_unscaled_bwd(C.byref(a), None) == 1
    a = good(unc=False)
    a.d_uncertain[0] = a.d_uncertain[1] = 0x5000        # d_uncertain without uncertain
    assert lib.fs_distill_unscaled_bwd(C.byref(a), None) == 1


def test_new_kernels_use_no_scratch():
    from fsnet_amd.csrc import build as B
    src = os.path.join(os.path.dirname(B.__file__), "distill_unscaled.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"] + B.extra_flags(src)
        r = subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        txt = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M)
    vspill = [int(x) for x in re.findall(r"^\s*\.vgpr_spill_count:\s*(\d+)", txt, re.M)]
    sspill = [int(x) for x in re.findall(r"^\s*\.sgpr_spill_count:\s*(\d+)", txt, re.M)]
    scratch = [int(x) for x in re.findall(r"^; ScratchSize: (\d+)", txt, re.M)]
    assert len(kernels) == 6 and len(vspill) == len(sspill) == len(scratch) == 6, kernels
    assert not any(vspill) and not any(sspill) and not any(scratch), (vspill, sspill, scratch)
    assert "-ffp-contract=off" in flags
    assert not re.search(r"global_atomic_\w*f(32|64)|flat_atomic_\w*f(32|64)", txt)      # no floating-point atomics


def test_oracle_step_reproduces_the_real_model_losses():
    """the model-level restatement (oracle pieces + the new term) against the REAL DistillWPoseMeta with the flag;
    3e-4 relative, the bound the GPU step is held to (the two run the same torch operators: they agree far closer)"""
    from oracle import distill_oracle as D
    from oracle import fsnet_oracle as O
    g = np.load(GOLD)
    M = HU.MODEL
    sd = D.init_states(seed=M["seed"], teacher_seed=M["teacher_seed"])
    with torch.no_grad():
        tot, losses, _ = HU.forward_train_unscaled(sd, O.synthetic_batch(M["B"], M["H"], M["W"], seed=M["batch_seed"]))
    want = g["m_loss"][1]
    assert abs(float(tot) - want[0]) < 3e-4 * want[0]
    for s in range(4):
        assert abs(float(losses["distilation/%d" % s]) - want[1 + s]) < 3e-4 * want[1 + s], s
