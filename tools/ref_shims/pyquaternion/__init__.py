"""Dev-only stand-in for `pyquaternion` (absent in this image) so that tools/gen_golden.py can run the reference's
nuScenes evaluator.  This is this project's reading of the package — construction from four numbers (w, x, y, z) and
the rotation_matrix property: normalise unless already unit within 1e-14, then the lower-right 3x3 block of
Q(q) @ Qbar(q)^T — and is not pinned against the real one.  Never imported on the product path or the GPU box."""
import numpy as np


class Quaternion(object):
    def __init__(self, *args):
        vals = args[0] if len(args) == 1 else args
        self.q = np.array(vals, dtype=float).reshape(4)

    def _sum_of_squares(self):
        return np.dot(self.q, self.q)

    @property
    def norm(self):
        return np.sqrt(self._sum_of_squares())

    def is_unit(self, tolerance=1e-14):
        return abs(1.0 - self._sum_of_squares()) < tolerance

    def _normalise(self):
        if not self.is_unit():
            n = self.norm
            if n > 0:
                self.q = self.q / n

    def _q_matrix(self):
        w, x, y, z = self.q
        return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])

    def _q_bar_matrix(self):
        w, x, y, z = self.q
        return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])

    @property
    def rotation_matrix(self):
        self._normalise()
        product_matrix = np.dot(self._q_matrix(), self._q_bar_matrix().conj().transpose())
        return product_matrix[1:][:, 1:]
