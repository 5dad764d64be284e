"""Times of the loss prologue's kernels alone (device events, no profiler): the identity terms as tile kernel
(fs_photo_identity) and as row-walking kernel (fs_photo_identity_rows), the colour pyramid as one launch per level and
as fs_color_pyramid_multi.   python tools/bench_photo_prologue.py [--iters 300]
Each kernel is timed twice: on ONE input set (the 53 MB of frames stay in the 256 MiB Infinity Cache between calls) and
rotating over six sets (390 MB: every call reads from HBM, as in the training step, where a whole step's traffic passes
between two calls).  FSNET_HIP_LIB selects another build of the library (e.g. one with another strip height ID_RS in
photometric.hip)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsnet_amd.hip import lib  # noqa: E402
from fsnet_amd.hip.binding import FsPhotoArgs, check, stream_ptr  # noqa: E402

NSETS = 6


def timed(fn, iters, nsets):
    for i in range(20):
        fn(i % nsets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % nsets)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"strip_rows": int(lib.fs_photo_identity_strip_rows()), "lib": os.environ.get("FSNET_HIP_LIB", "in-tree")}
    for B, H, W in ((12, 192, 640), (16, 384, 384)):
        g = torch.Generator(device=dev).manual_seed(B * H + W)
        sets = [[torch.rand(B, 3, H, W, device=dev, generator=g) for _ in range(3)] for _ in range(NSETS)]
        ident = torch.empty(B, 2, H, W, device=dev)
        msum = torch.zeros(B, dtype=torch.float64, device=dev)
        geo = torch.zeros(B, 48, device=dev)
        pas = []
        for t, s0, s1 in sets:
            pa = FsPhotoArgs()
            pa.img0, pa.img_src[0], pa.img_src[1] = t.data_ptr(), s0.data_ptr(), s1.data_ptr()
            pa.ident, pa.mask_sum, pa.geo = ident.data_ptr(), msum.data_ptr(), geo.data_ptr()
            pa.B, pa.H, pa.W, pa.S = B, H, W, 1
            pas.append(pa)
        hw = [(H >> s, W >> s) for s in (1, 2, 3)]
        pyr = [torch.empty(B, 3, h, w, device=dev) for h, w in hw]
        ptrs = (C.c_void_p * 3)(*[p.data_ptr() for p in pyr])
        hs, ws = (C.c_int32 * 3)(*[h for h, _ in hw]), (C.c_int32 * 3)(*[w for _, w in hw])
        st = stream_ptr()

        def ident_tile(i):
            check(lib.fs_photo_identity(C.byref(pas[i]), st), "identity")

        def ident_rows(i):
            check(lib.fs_photo_identity_rows(C.byref(pas[i]), st), "identity_rows")

        def pyr_levels(i):
            for p, (h, w) in zip(pyr, hw):
                check(lib.fs_color_pyramid(sets[i][0].data_ptr(), p.data_ptr(), B, H, W, h, w, st), "pyramid")

        def pyr_multi(i):
            check(lib.fs_color_pyramid_multi(sets[i][0].data_ptr(), ptrs, hs, ws, 3, B, H, W, st), "pyramid_multi")

        ident_bytes = 11 * B * H * W * 4            # nine planes read, two written
        pyr_bytes = int(B * 3 * H * W * 4 * (1 + 1 / 4 + 1 / 16 + 1 / 64))
        r = {}
        for name, fn, nbytes in (("identity_tile", ident_tile, ident_bytes), ("identity_rows", ident_rows, ident_bytes),
                                 ("pyramid_per_level", pyr_levels, pyr_bytes), ("pyramid_multi", pyr_multi, pyr_bytes)):
            for mode, nsets in (("one_set", 1), ("six_sets", NSETS)):
                us = min(timed(fn, a.iters, nsets) for _ in range(3))
                r["%s/%s" % (name, mode)] = {"us": round(us, 2), "GB_per_s": round(nbytes / us / 1e3, 1)}
        out["%dx%dx%d" % (B, H, W)] = r
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
