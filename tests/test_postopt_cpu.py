"""CPU checks of the sparse-VO post-optimisation: the torch restatement (tests/helpers_postopt.py) against the golden
vectors of the real reference (tests/golden/postopt.npz, tools/gen_golden.py gen_postopt), the C ABI's argument checks
without a GPU, and the kernels' register budget (no scratch, like test_no_spills_cpu.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from fsnet_amd.csrc import build as B
from tests import helpers_postopt as HP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postopt.npz")


def golden_case(g, tag):
    H, W, hs, ws, it, l0, l1, l2, mp = g["%s_params" % tag]
    params = dict(h_seg=int(hs), w_seg=int(ws), iter_num=int(it), lambda0=float(l0), lambda1=float(l1),
                  lambda2=float(l2), max_points=int(mp), lab_dist_weight=1, depth_dist_weight=1, image_dist_weight=1)
    return g["%s_image" % tag], g["%s_depth" % tag], g["%s_vo" % tag], params


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_reference(tag):
    g = np.load(GOLD)
    image, depth, vo, params = golden_case(g, tag)
    if tag == "a":
        assert int(((vo > 3) & (vo < 80)).sum()) > params["max_points"]        # the top-k branch
    else:
        assert int(((vo > 3) & (vo < 80)).sum()) < params["max_points"]
    out, seg, centres, _, _ = HP.post_optimize(image, depth, vo, details=True, **params)
    labels = g["%s_labels" % tag]
    assert (seg.numpy() == labels).mean() >= 0.999
    assert int(seg.max()) + 1 == int(labels.max()) + 1 == g["%s_centres" % tag].shape[0]
    rel = np.abs(out.numpy() / g["%s_refined" % tag] - 1)
    assert (rel <= 1e-5).mean() >= 0.999, rel.max()
    np.testing.assert_allclose(centres.numpy(), g["%s_centres" % tag], rtol=1e-5, atol=1e-4)


def test_restatement_early_stop_and_empty_segments():
    image, _, pred, vo = HP.synthetic_scene(64, 200, 3)
    _, _, _, nempty, its = HP.post_optimize(image, pred, vo, **dict(HP.HOOK_DEFAULTS, h_seg=16, w_seg=32,
                                                                      iter_num=40), details=True)
    assert nempty > 0 and its < 40


def _lib():
    path = B.build(verbose=False)
    from fsnet_amd.hip import lib
    assert os.path.exists(path)
    return lib


def test_invalid_arguments_are_rejected_without_a_gpu():
    from fsnet_amd.hip.binding import FsPostOptArgs
    lib = _lib()
    assert lib.fs_postopt(None, None) == 1
    assert lib.fs_postopt_workspace_bytes(1, 192, 640, 180) > 0
    assert lib.fs_postopt_workspace_bytes(1, 192, 640, 1025) == -1
    assert lib.fs_postopt_workspace_bytes(1, 65536, 32768, 180) == -1          # H*W = 2^31
    buf = (C.c_float * 16)()
    a = FsPostOptArgs()
    a.image = a.depth = a.vo = a.centres = a.out = a.workspace = C.addressof(buf)
    a.workspace_bytes = 1 << 40
    a.B, a.H, a.W, a.K, a.iter_num, a.max_points = 1, 8, 8, 2000, 3, 800
    a.lambda0, a.lambda1, a.lambda2 = 0.003, 1.0, 0.4
    assert lib.fs_postopt(C.byref(a), None) == 1                               # K out of range
    for field, bad in (("K", 0), ("iter_num", 0), ("max_points", 0), ("lambda2", 0.0), ("lambda0", -1.0)):
        a.K = 180
        old = getattr(a, field)
        setattr(a, field, bad)
        assert lib.fs_postopt(C.byref(a), None) == 1, field
        setattr(a, field, old)
    a.workspace_bytes = 16
    assert lib.fs_postopt(C.byref(a), None) == 1                               # workspace too small


@pytest.mark.skipif(shutil.which(B.HIPCC) is None and not os.path.exists(B.HIPCC), reason="hipcc not available")
def test_postopt_kernels_do_not_spill():
    src = os.path.join(os.path.dirname(B.__file__), "postopt.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        flags = [f for f in B.FLAGS if f != "-fPIC"] + B.extra_flags(src)
        subprocess.run([B.HIPCC] + flags + ["-S", "--cuda-device-only", src, "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        txt = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M)
    names = {"prepare", "centres_init", "assign", "vo_select", "segment_stats", "solve", "apply"}
    assert names == {n for n in names if any("postopt_" + n in k for k in kernels)}
    vspill = [int(x) for x in re.findall(r"^\s*\.vgpr_spill_count:\s*(\d+)", txt, re.M)]
    scratch = [int(x) for x in re.findall(r"^; ScratchSize: (\d+)", txt, re.M)]
    assert kernels and len(vspill) >= len(kernels) and len(scratch) >= len(kernels)
    assert max(vspill) == 0 and max(scratch) == 0, (vspill, scratch)
    assert not re.search(r"^\s*(scratch_(load|store)|buffer_(load|store)\S* .*\boffen\b.*s\[0:3\])", txt, re.M)
