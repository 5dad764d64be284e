"""rgb2lab stand-in for tools/gen_golden.py: skimage.color.rgb2lab restated from its published constants (sRGB
companding, the sRGB -> XYZ matrix, the D65 / 2-degree white, the CIE Lab f(t)), in float64.  Golden vectors that
pass through it pin the reference's own SLIC / solve arithmetic, NOT scikit-image: parity unpinned."""
import numpy as np

_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
_WHITE = (0.95047, 1.0, 1.08883)


def rgb2lab(rgb):
    c = np.asarray(rgb).astype(np.float64)
    if np.asarray(rgb).dtype == np.uint8:
        c = c / 255.0
    c = np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)
    xyz = [(c[..., 0] * _M[i, 0] + c[..., 1] * _M[i, 1] + c[..., 2] * _M[i, 2]) / _WHITE[i] for i in range(3)]
    fx, fy, fz = [np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0) for t in xyz]
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=-1)
