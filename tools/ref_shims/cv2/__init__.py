"""Import shim for tools/gen_golden.py ONLY (never on the product path, never on the GPU box).

OpenCV is not installed in this image.  The reference's augmentation module imports cv2 at module level and calls
two of its functions on the training path (warpAffine, cvtColor) and resize on the validation path.  This stand-in lets the module import and
routes those two calls to oracle/augment_oracle.py's restatement of OpenCV's algorithms — so golden vectors that
pass through them pin the reference's OWN arithmetic around the calls (draw order, P2 bookkeeping, mirror, colour
ops, Normalize) but NOT OpenCV itself: the oracle header and DESIGN.md mark warpAffine / cvtColor "parity unpinned".
"""
INTER_NEAREST, INTER_LINEAR = 0, 1
BORDER_CONSTANT = 0
COLOR_RGB2HSV, COLOR_HSV2RGB = 41, 55


def warpAffine(src, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT):
    from oracle import augment_oracle as A
    assert borderMode == BORDER_CONSTANT
    w, h = dsize
    if flags == INTER_NEAREST:
        return A.warp_affine_nearest(src, M, w, h)
    assert flags == INTER_LINEAR
    return A.warp_affine_linear(src, M, w, h)


def cvtColor(src, code):
    from oracle import augment_oracle as A
    if code == COLOR_RGB2HSV:
        return A.rgb2hsv(src)
    assert code == COLOR_HSV2RGB
    return A.hsv2rgb(src)


def resize(src, dsize, interpolation=INTER_LINEAR):
    from oracle import augment_oracle as A
    if interpolation == INTER_NEAREST:
        return A.resize_nearest(src, dsize[0], dsize[1])
    assert interpolation == INTER_LINEAR and src.dtype.name == "float32"
    return A.resize_linear(src, dsize[0], dsize[1])


# the motion-mask precompute hooks (monodepth/pipeline_hooks/precomputing_hooks/base_precompute_hooks.py) and the
# dataset's readers of their files: routed to tests/helpers_optflow.py's restatement of optflowgf.cpp (parity with
# OpenCV unpinned, like warpAffine) and to PIL / the project's 16-bit PNG reader
COLOR_BGR2GRAY = 6
IMREAD_UNCHANGED = -1
OPTFLOW_FARNEBACK_GAUSSIAN = 256


def _cvt_gray(src):
    import numpy as np
    from tests import helpers_optflow as HO
    assert src.dtype == np.uint8 and src.ndim == 3
    return HO.gray(src).astype(np.uint8)


_cvt_colour = cvtColor


def cvtColor(src, code):   # noqa: F811
    if code == COLOR_BGR2GRAY:
        return _cvt_gray(src)
    return _cvt_colour(src, code)


def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    from tests import helpers_optflow as HO
    assert flow is None
    return HO.farneback(prev, next, pyr_scale=pyr_scale, levels=levels, winsize=winsize, iterations=iterations,
                        poly_n=poly_n, poly_sigma=poly_sigma, flags=flags)


def imwrite(path, img):
    import numpy as np
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img)).save(path)
    return True


def imread(path, flags=1):
    import numpy as np
    from PIL import Image
    assert flags == IMREAD_UNCHANGED
    with open(path, "rb") as f:
        head = f.read(26)
    if head[24] == 16:                                     # 16-bit: cv2 returns BGR, or [H, W] for greyscale
        from fsnet_amd.monodepth.data.datasets.utils import read_png16
        img = read_png16(path)
        return img[:, :, ::-1].copy() if img.ndim == 3 else img
    return np.array(Image.open(path))
