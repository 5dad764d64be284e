"""The perspective half of the tiny KITTI-360 tree: tests/helpers_kitti360.make_tree plus calibration/perspective.txt
(P_rect_00 / P_rect_01 and rectifying rotations that are not identity) and rectified frames of both pinhole cameras
under image_00 / image_01 / data_rect, at a small non-square size — shared by tools/gen_golden.py::gen_kitti360_persp
(which runs the REAL KITTI360MonoDataset and Kitti360Evaluator over it) and the tests.  The scans are made dense enough
(NPTS points) that every evaluation frame has more than a thousand pixels hit twice or more and at least one merged
edge pair — points on (r, W-1) and on (r+1, 0), which share the export's index (monodepth_utils.sub2ind)."""
import os

import numpy as np

from tests import helpers_kitti360 as HK

SEQ = HK.SEQ
H, W = 94, 310
NFRAMES = HK.NFRAMES
EVAL_FRAMES = HK.EVAL_FRAMES
NPTS = 60000
SEED = 11
GOLDEN_DRAW_SEED = 3          # np.random.seed before the golden's use_right_image samples are drawn


def perspective():
    """(P_rect_00, P_rect_01 [3, 4], R_rect_00, R_rect_01 [3, 3]) of the two pinhole cameras at H x W"""
    f = 151.25
    P0 = np.array([[f, 0, 155.3, 0], [0, f, 47.1, 0], [0, 0, 1, 0]])
    g = 150.5                  # (the two cameras differ so that a sample's P2 tells which one it came from)
    P1 = np.array([[g, 0, 156.1, -g * 0.594], [0, g, 46.8, 0], [0, 0, 1, 0]])
    R0 = HK._rot("x", 0.006) @ HK._rot("y", -0.004) @ HK._rot("z", 0.003)
    R1 = HK._rot("x", -0.005) @ HK._rot("y", 0.007) @ HK._rot("z", -0.002)
    return P0, P1, R0, R1


def make_tree(root, seed=SEED, npts=NPTS):
    """-> (raw path, training split, evaluation split)"""
    from PIL import Image
    raw, train, val, _ = HK.make_tree(root, seed=seed, npts=npts)
    P0, P1, R0, R1 = perspective()
    with open(os.path.join(raw, "calibration", "perspective.txt"), "w") as f:
        for k, (P, R) in (("00", (P0, R0)), ("01", (P1, R1))):
            f.write("S_rect_%s: %r %r\n" % (k, float(W), float(H)))
            f.write("R_rect_%s: %s\n" % (k, " ".join(repr(float(v)) for v in R.reshape(-1))))
            f.write("P_rect_%s: %s\n" % (k, " ".join(repr(float(v)) for v in P.reshape(-1))))
    rng = np.random.RandomState(seed + 1000)
    for cam in ("image_00", "image_01"):
        d = os.path.join(raw, "data_2d_raw", SEQ, cam, "data_rect")
        os.makedirs(d, exist_ok=True)
        for i in range(NFRAMES):
            Image.fromarray(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(os.path.join(d, "%010d.png" % i))
    return raw, train, val


dataset_cfg = HK.dataset_cfg


def scan(raw, i):
    return np.fromfile(os.path.join(raw, "data_3d_raw", SEQ, "velodyne_points/data", "%010d.bin" % i),
                       dtype=np.float32).reshape(-1, 4)


def velo_to_image(raw):
    """P_velo2img = P0 @ R0 @ inv(T_cam2velo), from the values written (kitti_unsupervised_eval.py:190)"""
    P0, _, R0, _ = perspective()
    R = np.eye(4)
    R[:3, :3] = R0
    return P0 @ R @ np.linalg.inv(HK.extrinsics()[4])


def pixel_points(velo, P):
    """per point with x >= 0, in scan order: (u, v) f64 before rounding, (row, col) after np.round(.) - 1 (f64) and
    the value (float32 x) — the reference's arithmetic with the same numpy matrix product"""
    v4 = velo[velo[:, 0] >= 0, :].copy()
    v4[:, 3] = 1.0
    p = np.dot(P, v4.T).T
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    col, row = np.round(u) - 1, np.round(v) - 1
    return u, v, row, col, v4[:, 0]


def fixture_counts(velo, P, H=H, W=W):
    """(pixels hit by two or more points, merged edge pairs: rows r with points on (r, W-1) and on (r+1, 0))"""
    _, _, row, col, _ = pixel_points(velo, P)
    ok = (col >= 0) & (row >= 0) & (col < W) & (row < H)
    hits = np.bincount((row[ok] * W + col[ok]).astype(np.int64), minlength=H * W).reshape(H, W)
    pairs = int(((hits[:-1, W - 1] > 0) & (hits[1:, 0] > 0)).sum())
    return int((hits >= 2).sum()), pairs


def sparse(depth):
    idx, val, _ = HK.sparse(depth, np.zeros(depth.shape, bool))
    return idx, val


def dense(idx, val, H=H, W=W):
    return HK.dense(idx, val, np.zeros(0, np.int32), H, W)[0]
