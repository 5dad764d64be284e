"""CPU side of the fisheye (Mei) loss chain over one to four source frames: the entry points exist and refuse what they
must, FishEyeDecoder takes the frame lists, the inputs of tests/test_fisheye_n_gpu.py meet the conditions of
tests/helpers_fisheye_n.py on the oracle alone, and the oracle reproduces the REAL FishEyeDecoder.loss
(tests/golden/fisheye_nsrc.npz, tools/gen_golden.py::gen_fisheye_nsrc)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers_fisheye_n as Q

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FRAME_LISTS = [[0, -1], [0, -2, -1, 1], [0, -2, -1, 1, 2]]


def _args(N=3, B=2, H=8, W=8, S=1):
    """a complete FsPhotoMeiMultiArgs with dummy (never dereferenced) addresses"""
    from fsnet_amd.hip.binding import FsPhotoMeiMultiArgs
    a = FsPhotoMeiMultiArgs()
    p = 0x1000
    a.img0 = a.geo = a.ident = a.sel = a.loss_sums = a.mask_sum = a.dP = a.lut_ptrs = a.mei = a.warp_mask = p
    for f in range(N):
        a.img_src[f] = p
    for s in range(S):
        a.depth[s] = a.d_depth[s] = p
        a.dh[s], a.dw[s] = max(H >> s, 1), max(W >> s, 1)
    a.B, a.H, a.W, a.S, a.nsrc = B, H, W, S, N
    a.noise_seed = -1
    return a


def test_entry_points_exist_and_reject_invalid_arguments_without_a_gpu():
    from fsnet_amd.hip import binding, lib
    from fsnet_amd.hip.signatures import SIGNATURES
    for name in ("fs_photo_mei_multi_setup", "fs_photo_mei_multi_fwd", "fs_photo_mei_multi_bwd"):
        assert name in SIGNATURES and getattr(lib, name) is not None
    assert int(lib.fs_abi_version()) == binding.ABI_VERSION == 15
    M, A = binding.FsPhotoMultiArgs, binding.FsPhotoMeiMultiArgs
    # FsPhotoMultiArgs field for field, then the ray-table fields: a pointer to it serves fs_photo_multi_identity
    assert A._fields_[:len(M._fields_)] == M._fields_
    assert [n for n, _ in A._fields_[len(M._fields_):]] == ["lut_ptrs", "mei", "warp_mask"]
    assert all(getattr(A, n).offset == getattr(M, n).offset for n, _ in M._fields_)
    fwd, bwd = lib.fs_photo_mei_multi_fwd, lib.fs_photo_mei_multi_bwd
    assert fwd(None, None) == 1 and bwd(None, None) == 1
    for fn in (fwd, bwd):
        def bad(**kw):
            a = _args()
            for k, v in kw.items():
                setattr(a, k, v)
            return fn(C.byref(a), None) == 1
        assert bad(lut_ptrs=None) and bad(mei=None) and bad(lut_ptrs=None, mei=None)
        assert bad(nsrc=0) and bad(nsrc=5) and bad(S=0) and bad(S=5) and bad(B=0) and bad(H=1) and bad(W=1)
        assert bad(img0=None) and bad(geo=None) and bad(sel=None)
        assert bad(H=32768, W=10923)                                  # 3 H W >= 2^30
        a = _args()
        a.img_src[2] = None
        assert fn(C.byref(a), None) == 1
        a = _args()
        a.depth[0] = None
        assert fn(C.byref(a), None) == 1
    a = _args()
    a.ident = None                                                    # forward: identity planes or a motion mask
    assert fwd(C.byref(a), None) == 1
    a = _args()
    a.loss_sums = None
    assert fwd(C.byref(a), None) == 1
    a = _args()
    a.pred = 0x1000                                                   # pred without ov
    assert fwd(C.byref(a), None) == 1
    for k in ("dP", "mask_sum"):
        a = _args()
        setattr(a, k, None)
        assert bwd(C.byref(a), None) == 1
    a = _args()
    a.d_depth[0] = None
    assert bwd(C.byref(a), None) == 1
    Tp = (C.c_void_p * 4)(0x1000, 0x1000, 0x1000, None)
    setup = lib.fs_photo_mei_multi_setup
    assert setup(None, 3, 0x1000, 2, None, None) == 1 and setup(Tp, 3, None, 2, None, None) == 1
    assert setup(Tp, 0, 0x1000, 2, None, None) == 1 and setup(Tp, 5, 0x1000, 2, None, None) == 1
    assert setup(Tp, 4, 0x1000, 2, None, None) == 1                   # the fourth transform is missing
    assert setup(Tp, 3, 0x1000, 0, None, None) == 1


def _decoder(fids, **flags):
    from fsnet_amd.monodepth.networks.models.heads import monodepth2_decoder as M
    dec = M.FishEyeDecoder.__new__(M.FishEyeDecoder)
    torch.nn.Module.__init__(dec)
    dec.frame_ids = list(fids)
    for k, v in flags.items():
        setattr(dec, k, v)
    return dec


@pytest.mark.parametrize("fids", FRAME_LISTS + [[0, 1, -1]])
def test_fisheye_model_constructs(fids):
    from fsnet_amd.configs import meta_arch_cfg
    from fsnet_amd.monodepth.networks.models.heads.monodepth2_decoder import FishEyeDecoder
    from fsnet_amd.vision_base.utils.builder import build
    m = build(**meta_arch_cfg(64, 64, with_pose=False, num_output_channels=64, max_depth=150.0, fisheye=True,
                              frame_ids=fids))
    assert isinstance(m.head, FishEyeDecoder) and list(m.head.frame_ids) == fids
    assert bool(m.head.n_frame_kernels) == (len(fids) != 3)
    m.head._check_frame_ids()
    m.head._check_options({})


def test_check_frame_ids_accepts_and_refuses():
    """with the head option n_frame_kernels every list the base class admits passes; the base class's refusals stay;
    without the option a list other than [0, a, b] is refused as before (pinned in tests/test_photo64n_cpu.py), and the
    message names the option"""
    for fids in FRAME_LISTS + [[0, 1, -1]]:
        _decoder(fids, n_frame_kernels=True)._check_frame_ids()
        _decoder(fids, n_frame_kernels=True)._check_options({})
    _decoder([0, 1, -1])._check_options({})
    for fids, word in (([0, "s"], "stereo"), ([0, 1, "s"], "stereo"), ([0, 1, 1], "once"), ([0, 1, 0], "differ"),
                       ([0, -3, -2, -1, 1, 2], "at most"), ([0], "at least one"), ([1, 0], "target")):
        with pytest.raises(NotImplementedError) as e:
            _decoder(fids, n_frame_kernels=True)._check_frame_ids()
        assert word in str(e.value) and repr(fids) in str(e.value)
    for fids in FRAME_LISTS:
        with pytest.raises(NotImplementedError) as e:
            _decoder(fids)._check_frame_ids()
        assert "two" in str(e.value) and "n_frame_kernels" in str(e.value) and repr(fids) in str(e.value)


def test_photo_mei_multi_kernels_do_not_spill(tmp_path):
    """photo_mei_multi.hip compiled to assembly with the library's flags: the two resource-summary numbers of its three
    kernels, as tests/test_photo64n_cpu.py reads them for photo_multi.hip"""
    import re
    import subprocess
    from fsnet_amd.csrc import build as Bd
    src = os.path.join(Bd.HERE, "photo_mei_multi.hip")
    out = str(tmp_path / "photo_mei_multi.s")
    r = subprocess.run([Bd.HIPCC] + Bd.FLAGS + Bd.extra_flags(src) + ["--cuda-device-only", "-S", src, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)]
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", asm)]
    assert len(spills) == 3 and len(scratch) == 3, (spills, scratch)
    assert all(v == 0 for v in spills), spills
    assert all(v <= 128 for v in scratch), scratch
    assert "photo_mei_multi_bwd_kernel" in asm and "photo_mei_multi_fwd_kernel" in asm


def test_photometric_loss_engine_takes_the_ray_tables_on_the_n_frame_backend():
    """ops.PhotometricLoss: nsrc != 2 (or force_multi) starts on fs_photo_multi_*; what stage_fisheye() does to it is on
    the GPU side — here: the backend table"""
    from fsnet_amd.hip import binding, lib, ops
    be = ops._photo_backend(True, fisheye=True)
    assert be.args is binding.FsPhotoMeiMultiArgs and be.name == "photo_mei_multi"
    assert be.fwd is lib.fs_photo_mei_multi_fwd and be.bwd is lib.fs_photo_mei_multi_bwd
    assert be.identity is lib.fs_photo_multi_identity and be.bwd_tiles is lib.fs_photo_multi_bwd_tiles
    assert be.geo_floats(3) == 18 + 12 * 3
    two = ops._photo_backend(False)
    assert two.args is binding.FsPhotoArgs and two.fwd is lib.fs_photo_fused_fwd


@pytest.mark.parametrize("name", Q.case_names())
def test_inputs_meet_the_conditions(name):
    case = Q.make_case(name)
    m = Q.measure(case)
    print("CONDITIONS %-10s seed %d wins %s ties %.5f fragile %.5f noise shift %.2e" % (
        name, case["seed"], " ".join("%.3f" % w for w in m["wins"]), m["ties"], m["fragile"], m["noise_shift"]))
    assert Q.check_conditions(case, m) == []
    # the regions lie inside the ray-table mask
    _, _, lm = Q.sample_coords(torch.ones(Q.B, 1, case["H"], case["W"]), torch.eye(4).repeat(Q.B, 1, 1),
                               case["data"]["P2"], case["data"]["calib_meta"])
    for _, _, y0, y1, x0, x1 in Q.cells(case["H"], case["W"], case["N"]):
        assert bool((lm[:, y0:y1, x0:x1] == 1).all())
    # and what the selection test excuses stays small
    res = Q.oracle_chain(case)
    assert float((Q.gap(Q.candidates(case, res)) < Q.NOISE_GAP).double().mean()) < 0.02


@pytest.mark.parametrize("name", [n for n in Q.case_names() if Q.SEEDS[n] > 1])
def test_the_seed_is_the_first_that_meets_them(name):
    assert Q.find_seed(name, limit=Q.SEEDS[name]) == Q.SEEDS[name]


def test_existing_two_source_inputs_near_ties_and_fragile_samples():
    """the inputs of tests/golden/fisheye.npz, which the N = 2 equivalence test runs: conditions 2 and 3 measured (1 is
    not theirs to meet: the file predates it)"""
    from tests.test_oracle_golden import fisheye_chain_inputs
    g = np.load(os.path.join(GOLD, "fisheye.npz"))
    case = case_from_fisheye_golden(g, fisheye_chain_inputs(g))
    res = Q.oracle_chain(case)
    ties = float((Q.gap(Q.candidates(case, res)) < 1e-6).double().mean())
    frag = float(Q.fragile(case).double().mean())
    print("CONDITIONS n2 (fisheye.npz) ties %.5f fragile %.5f" % (ties, frag))
    assert ties <= Q.MAX_TIES


def case_from_fisheye_golden(g, data):
    """tests/golden/fisheye.npz as a case of helpers_fisheye_n (frame_ids [0, 1, -1])"""
    H, W = int(g["H"]), int(g["W"])
    return dict(name="n2", N=2, fids=(0, 1, -1), H=H, W=W, data=data,
                depths=[torch.from_numpy(g["depth_%d" % s]) for s in range(4)],
                aa={1: torch.from_numpy(g["aa_p"]), -1: torch.from_numpy(g["aa_m"])},
                tr={1: torch.from_numpy(g["tr_p"]), -1: torch.from_numpy(g["tr_m"])}, seed=int(g["seed"]))


@pytest.mark.parametrize("N", [1, 3, 4])
def test_oracle_reproduces_the_reference_golden(N):
    """FO.photometric_loss on the inputs of the golden against the REAL FishEyeDecoder.loss: the deviations
    tools/gen_golden.py::gen_fisheye prints for N = 2, held to the bounds tests/test_oracle_golden.py holds that file to"""
    g = np.load(os.path.join(GOLD, "fisheye_nsrc.npz"))
    tag = "n%d_" % N
    case = Q.make_case("golden-n%d" % N)
    fids = list(case["fids"])
    # the golden's inputs are the helper's
    assert list(g[tag + "frame_ids"]) == fids and int(g[tag + "seed"]) == case["seed"]
    for f in fids:
        assert np.array_equal(g[tag + "img8_%d" % f], case["u8"][f])
    for s in range(4):
        assert np.array_equal(g[tag + "depth_%d" % s], case["depths"][s].numpy())
    for f in fids[1:]:
        assert np.array_equal(g[tag + "aa_%d" % f], case["aa"][f].numpy()) and np.array_equal(g[tag + "tr_%d" % f], case["tr"][f].numpy())
    assert np.array_equal(g[tag + "P2"], case["data"]["P2"].numpy())
    assert np.array_equal(g[tag + "patched_mask"], case["data"]["patched_mask"].numpy().astype(np.uint8))
    o = Q.oracle_chain(case, grads=True)
    dev = lambda a, b: float((a.double() - torch.as_tensor(b).double()).abs().max())
    d_tot = abs(float(o["total"]) - float(g[tag + "total_loss"]))
    d_s = [abs(float(o["ld"]["loss/%d" % s]) - float(g[tag + "ld_loss_%d" % s])) for s in range(4)]
    d_g = [float((o["depths"][s].grad - torch.from_numpy(g[tag + "gdepth_%d" % s])).norm()
                 / torch.from_numpy(g[tag + "gdepth_%d" % s]).norm()) for s in range(4)]
    d_w = max(dev(o["outputs"][("original_image", f, 0)][:, :, ::2, ::2], g[tag + "warp0_%d" % f]) for f in fids[1:])
    ov = min(float((o["outputs"][("overlapped_mask", f, 0)].numpy() == g[tag + "ovmask0_%d" % f]).mean()) for f in fids[1:])
    print("DEVIATION N=%d total %.2e per scale %s gdepth rel %s warp %.2e ov agreement %.5f" % (
        N, d_tot, " ".join("%.2e" % v for v in d_s), " ".join("%.2e" % v for v in d_g), d_w, ov))
    assert o["total"].dtype == torch.float64
    assert d_tot < 2e-7 and max(d_s) < 5e-7 and max(d_g) < 2e-3 and d_w < 1e-5 and ov > 0.9999
    for (aa, tr), f in zip(o["poses"], fids[1:]):
        for got, key in ((aa.grad, "gaa_%d" % f), (tr.grad, "gtr_%d" % f)):
            ref = torch.from_numpy(g[tag + key])
            assert dev(got, ref) < 5e-3 * float(ref.abs().max()) + 1e-9, key
    # under the reference's noise the oracle's selection is the golden's
    noisy = Q.oracle_chain(case, noise=Q.reference_noise(case))
    for s in range(4):
        assert np.array_equal(noisy["outputs"][("min_idx", s)].numpy().astype(np.uint8), g[tag + "minidx_%d" % s])
    assert abs(float(noisy["total"]) - float(g[tag + "total_loss"])) < 2e-7
