"""A tiny KITTI-360 tree on disk (one sequence, both fisheye cameras, PNG frames, Mei calibration YAMLs, camera /
velodyne extrinsics, data_poses, velodyne scans, a fisheye mask and a comma-separated split) generated from a seed —
shared by tools/gen_golden.py::gen_kitti360_fisheye (which runs the REAL KITTI360FisheyeDataset and
Kitti360FisheyeEvaluator over it) and the tests.  Also a vectorised numpy restatement of the reference's fisheye
ground truth (kitti360_fisheye_eval.py:97-145; the last point written to a pixel wins)."""
import os

import numpy as np

SEQ = "2013_05_28_drive_0000_sync"
H, W = 350, 350
NFRAMES = 12
MASK_HW = (700, 700)          # the mask file is larger than the frames: the reader resizes it (INTER_NEAREST)
EVAL_FRAMES = (2, 4, 6, 9)    # frames with a velodyne scan: the evaluation split


def mei_calib(variant):
    """(P [3,4] f32, calib dict) of synthetic_mei_calib at H x W: left (0) / right (1) camera"""
    from fsnet_amd.vision_base.data.datasets.synthetic import synthetic_mei_calib
    return synthetic_mei_calib(H, W, variant)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _line(T):
    return " ".join(repr(float(v)) for v in T[:3, :].reshape(-1))


def extrinsics():
    """camera -> vehicle pose frame (x forward, y left, z up) of image_00 (forward) and the fisheyes image_02 (looking
    left) / image_03 (looking right), and camera 00 -> velodyne"""
    # camera axes: x right, y down, z optical axis
    fwd = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])        # columns: camera x, y, z in the pose frame
    left = np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]])
    right = np.array([[-1.0, 0, 0], [0, 0, -1], [0, -1, 0]])
    T00 = _T(fwd @ _rot("x", 0.004) @ _rot("y", -0.003), [1.50, 0.02, 1.56])
    T01 = _T(fwd @ _rot("z", 0.002), [1.52, -0.58, 1.55])
    T02 = _T(left @ _rot("x", 0.02) @ _rot("y", -0.015) @ _rot("z", 0.01), [0.72, 1.03, 1.48])
    T03 = _T(right @ _rot("x", -0.018) @ _rot("y", 0.012) @ _rot("z", -0.008), [0.73, -1.01, 1.47])
    velo = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])        # velodyne axes as the pose frame's, 0.3 m higher
    T_cam2velo = _T(velo @ _rot("x", 0.003) @ _rot("z", -0.002), [0.78, -0.29, -0.31])
    return T00, T01, T02, T03, T_cam2velo


def _write_yaml(path, P, calib, name):
    with open(path, "w") as f:
        f.write("%YAML:1.0\n")                          # not YAML for PyYAML: the reader skips the first line
        f.write("---\nmodel_type: MEI\ncamera_name: %s\nimage_width: %d\nimage_height: %d\n" % (name, W, H))
        f.write("mirror_parameters:\n   xi: %r\n" % float(calib["mirror_parameters"]["xi"]))
        f.write("distortion_parameters:\n   k1: %r\n   k2: %r\n   p1: 0.0\n   p2: 0.0\n" % (
            float(calib["distortion_parameters"]["k1"]), float(calib["distortion_parameters"]["k2"])))
        f.write("projection_parameters:\n   gamma1: %r\n   gamma2: %r\n   u0: %r\n   v0: %r\n" % (
            float(P[0, 0]), float(P[1, 1]), float(P[0, 2]), float(P[1, 2])))


def scene(rng, n=20000):
    """velodyne frame (x forward, y left, z up; ground 1.73 m below): ground, building walls on both sides, boxes
    and poles; float32 [n, 4] with a reflectance column.  About half lies to the right, behind the left camera."""
    parts = []
    ng = n * 2 // 5
    r, a = rng.uniform(2.0, 30.0, ng), rng.uniform(-np.pi, np.pi, ng)
    parts.append(np.stack([r * np.cos(a), r * np.sin(a), -1.73 + rng.normal(0, 0.02, ng)], 1))
    nw = n * 3 // 10
    side = np.where(rng.rand(nw) < 0.5, 1.0, -1.0)
    parts.append(np.stack([rng.uniform(-25, 25, nw), side * (7.5 + rng.uniform(0, 0.3, nw)),
                           rng.uniform(-1.73, 6.0, nw)], 1))
    no = n - ng - nw
    centres = np.stack([rng.uniform(-12, 12, 8), rng.uniform(-6, 6, 8), np.full(8, -0.9)], 1)
    k = rng.randint(0, 8, no)
    parts.append(centres[k] + rng.uniform(-0.9, 0.9, (no, 3)) * np.array([1.0, 0.8, 0.9]))
    pts = np.concatenate(parts)[rng.permutation(n)]
    out = np.empty((n, 4), np.float32)
    out[:, :3] = pts
    out[:, 3] = rng.uniform(0, 1, n)
    return out


def make_tree(root, seed=11, npts=20000):
    """-> (raw path, training split, evaluation split, fisheye mask path)"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    raw = os.path.join(root, "KITTI-360")
    calib_dir = os.path.join(raw, "calibration")
    os.makedirs(calib_dir, exist_ok=True)
    for cam, variant in (("image_02", 0), ("image_03", 1)):
        P, calib = mei_calib(variant)
        _write_yaml(os.path.join(calib_dir, cam + ".yaml"), P, calib, cam)
    T00, T01, T02, T03, T_cam2velo = extrinsics()
    with open(os.path.join(calib_dir, "calib_cam_to_pose.txt"), "w") as f:
        for name, T in (("image_00", T00), ("image_01", T01), ("image_02", T02), ("image_03", T03)):
            f.write("%s: %s\n" % (name, _line(T)))
    with open(os.path.join(calib_dir, "calib_cam_to_velo.txt"), "w") as f:
        f.write(_line(T_cam2velo) + "\n")
    # poses: steady drive along x with a slight turn; rows 6-7 stand still, row 10 jumps 4 m (both filtered out)
    pose_dir = os.path.join(raw, "data_poses", SEQ)
    os.makedirs(pose_dir, exist_ok=True)
    x, yaw = 0.0, 0.0
    with open(os.path.join(pose_dir, "poses.txt"), "w") as f:
        for i in range(NFRAMES + 2):
            x += {6: 0.0, 7: 0.0, 10: 4.0}.get(i, 0.9)
            yaw += 0.01
            T = _T(_rot("z", yaw) @ _rot("x", rng.uniform(-0.01, 0.01)), [x, 0.05 * i, 0.1 + 0.01 * i])
            f.write("%d %s\n" % (100 + i, _line(T)))
    for cam in ("image_02", "image_03"):
        d = os.path.join(raw, "data_2d_raw", SEQ, cam, "data_rgb")
        os.makedirs(d, exist_ok=True)
        for i in range(NFRAMES):
            Image.fromarray(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).save(os.path.join(d, "%010d.png" % i))
    vd = os.path.join(raw, "data_3d_raw", SEQ, "velodyne_points", "data")
    os.makedirs(vd, exist_ok=True)
    for i in EVAL_FRAMES:
        scene(rng, npts).tofile(os.path.join(vd, "%010d.bin" % i))
    yy, xx = np.mgrid[0:MASK_HW[0], 0:MASK_HW[1]]
    mask = (((yy - MASK_HW[0] / 2.0) ** 2 + (xx - MASK_HW[1] / 2.0) ** 2) < (0.47 * MASK_HW[0]) ** 2).astype(np.uint8)
    mask_path = os.path.join(root, "fisheye_mask.png")
    Image.fromarray(mask).save(mask_path)
    # split lines: sequence, pose index, image index, former, latter (pose rows index poses.txt's line order)
    train = os.path.join(root, "kitti360_train.txt")
    with open(train, "w") as f:
        for i in range(1, NFRAMES - 1):
            f.write("%s,%d,%d,%d,%d\n" % (SEQ, i, i, i - 1, i + 1))
    val = os.path.join(root, "kitti360_val.txt")
    with open(val, "w") as f:
        for i in EVAL_FRAMES:
            f.write("%s,%d,%d,%d,%d\n" % (SEQ, i, i, i - 1, i + 1))
    return raw, train, val, mask_path


def dataset_cfg(raw, split, prefix, **kw):
    """ConvertToFloat + Normalize + ConvertToTensor only (no cv2 pixel calls: the reference class runs with the
    import shim)"""
    aug = prefix + 'vision_base.data.augmentations.augmentations'
    frame_ids = [0, -1, 1]
    keys = [('image', i) for i in frame_ids]
    cfg = dict(raw_path=raw, split_file=split, frame_ids=frame_ids,
               augmentation=dict(name=prefix + 'vision_base.utils.builder.Sequential', cfg_list=[
                   dict(name=aug + '.ConvertToFloat'),
                   dict(name=aug + '.Normalize', mean=np.array([0.485, 0.456, 0.406]),
                        stds=np.array([0.229, 0.224, 0.225])),
                   dict(name=aug + '.ConvertToTensor')],
                   image_keys=keys, calib_keys=['P2'], gt_image_keys=['patched_mask']))
    cfg.update(kw)
    return cfg


def velo_to_cam02(calib_dir):
    """T_velo2cam02 composed like kitti360_fisheye_eval.py:106-108"""
    from fsnet_amd.monodepth.data.datasets.fisheye_dataset import (read_cam2velo_from_sequence,
                                                                   read_extrinsic_from_sequence)
    T = read_extrinsic_from_sequence(os.path.join(calib_dir, "calib_cam_to_pose.txt"))
    T_cam2velo = read_cam2velo_from_sequence(os.path.join(calib_dir, "calib_cam_to_velo.txt"))
    return np.linalg.inv(T["T_image2"]) @ T["T_image0"] @ np.linalg.inv(T_cam2velo)


def mei_project(cam, P, calib):
    """_cam2image's pixel coordinates (mei_fisheye_utils.py:23-51) in numpy f64, its operation order, and the norm"""
    eps = 1e-6
    norm = np.linalg.norm(cam, axis=-1)
    xs = cam[:, 0] / (norm + eps)
    ys = cam[:, 1] / (norm + eps)
    zs = cam[:, 2] / (norm + eps)
    xi = calib["mirror_parameters"]["xi"]
    xs /= zs + xi + eps
    ys /= zs + xi + eps
    k1, k2 = calib["distortion_parameters"]["k1"], calib["distortion_parameters"]["k2"]
    r2 = xs * xs + ys * ys
    xs = xs * (1 + k1 * r2 + k2 * r2 * r2)
    ys = ys * (1 + k1 * r2 + k2 * r2 * r2)
    return P[0, 0] * xs + P[0, 2], P[1, 1] * ys + P[1, 2], norm


def gt_points(velo, T, P, calib):
    """per point with camera z > 0, in scan order: (u, v, z, norm) f64 — the reference's arithmetic (the same numpy
    matrix product for the transform)"""
    cam = (T @ np.concatenate([velo[:, 0:3], np.ones([velo.shape[0], 1])], axis=1).T).T[:, 0:3]
    cam = cam[cam[:, 2] > 0]
    u, v, norm = mei_project(cam, P, calib)
    return u, v, cam[:, 2], norm


def ground_truth(velo, T, P, calib, H=H, W=W):
    """(depth float32 [H, W], close mask bool [H, W]) of one scan: int32 truncation of the pixel coordinates, the last
    point written to a pixel wins (numpy's fancy assignment in the reference's _projection); points outside the image
    are dropped (none are in this tree)"""
    u, v, z, norm = gt_points(velo, T, P, calib)
    keep = (u > -1) & (u < W) & (v > -1) & (v < H)
    iy, ix = v[keep].astype(np.int32), u[keep].astype(np.int32)
    depth = np.zeros((H, W))
    depth[iy, ix] = z[keep]
    gt_norm = np.zeros((H, W))
    gt_norm[iy, ix] = norm[keep]
    return depth.astype(np.float32), (gt_norm > 0) & (gt_norm < 8)


def float_sub2ind_unique(velo, T, P, calib, H=H):
    """the reference's duplicate search (sub2ind on untruncated coordinates, monodepth_utils.py:291-295) finds no
    duplicate: every point's row * (W - 1) + col - 1 differs"""
    u, v, _, _ = gt_points(velo, T, P, calib)
    inds = v * (W - 1) + u - 1
    return len(np.unique(inds)) == len(inds)


def sparse(depth, mask):
    """compact golden form: flat indices + values of the depth map, flat indices of the close mask"""
    d = depth.reshape(-1)
    idx = np.flatnonzero(d).astype(np.int32)
    return idx, d[idx].astype(np.float32), np.flatnonzero(mask.reshape(-1)).astype(np.int32)


def dense(idx, val, midx, H=H, W=W):
    depth = np.zeros(H * W, np.float32)
    depth[idx] = val
    mask = np.zeros(H * W, bool)
    mask[midx] = True
    return depth.reshape(H, W), mask.reshape(H, W)


def single_loss(pred, gt, close_mask):
    """the fisheye _single_loss (kitti360_fisheye_eval.py:43-72) in numpy on a prediction already at the ground
    truth's size: 0.3 < gt < 60 (float32 comparisons) and the close mask, median scaling, clamp [1e-3, 80], the seven
    errors for the scaled and the unscaled prediction"""
    from oracle import eval_oracle as EO
    mask = (gt > np.float32(0.3)) & (gt < np.float32(60.0)) & close_mask
    p, g = pred[mask].astype(np.float32), gt[mask].astype(np.float32)
    if len(p) == 0:
        raise ValueError
    ratio = np.median(g) / np.median(p)
    scaled = np.clip(p * ratio, np.float32(1e-3), np.float32(80.0))
    err = EO.compute_errors(g, scaled)
    abs_err = EO.compute_errors(g, np.clip(p, np.float32(1e-3), np.float32(80.0)))
    return dict(ratio=ratio, error=err, abs_error=abs_err)


# ---- shared by tests/test_kitti360_fisheye_gpu.py and tests/test_kitti360_persp_gpu.py

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
AUG = 'fsnet_amd.vision_base.data.augmentations.augmentations'


def check_metric(got, want, n_valid):
    """the tolerances of tests/test_eval_gpu.py::test_depth_eval_matches_oracle"""
    assert abs(float(got["ratio"]) - float(want["ratio"])) <= 1e-5 * abs(float(want["ratio"]))
    for key in ("error", "abs_error"):
        a, b = np.array(got[key], np.float64), np.array(want[key], np.float64)
        print(key, np.abs(a - b).max())
        assert np.abs(a[:4] - b[:4]).max() <= 2e-5 * max(1.0, np.abs(b[:4]).max()), (key, a, b)
        assert np.abs(a[4:] - b[4:]).max() <= 3.0 / max(1, n_valid // 4), (key, a, b)


def run_captured(op, fills):
    """a staged LiDAR op run once, then captured into a graph on a side stream and replayed; `fills` (output buffer
    name -> value) overwrites the outputs before the capture and before the replay, so what they hold afterwards is
    what the replay wrote"""
    import torch

    def overwrite():
        for name, value in fills.items():
            getattr(op, name).fill_(value)
    op.run()
    torch.cuda.synchronize()
    overwrite()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            op.run()
    torch.cuda.current_stream().wait_stream(s)
    overwrite()
    graph.replay()
    torch.cuda.synchronize()


def val_augmentation(h, w):
    """the validation chain of the KITTI-360 configs: ConvertToFloat, Resize without aspect ratio, Normalize,
    ConvertToTensor"""
    return dict(name='fsnet_amd.vision_base.utils.builder.Sequential', cfg_list=[
        dict(name=AUG + '.ConvertToFloat'),
        dict(name=AUG + '.Resize', size=(h, w), preserve_aspect_ratio=False),
        dict(name=AUG + '.Normalize', mean=MEAN, stds=STD),
        dict(name=AUG + '.ConvertToTensor')],
        image_keys=[('image', 0)], calib_keys=['P2'])


def train_augmentation(h, w, origs_in_image_keys):
    """the training chain; the perspective one lists the ('original_image', f) among its image_keys, the fisheye one
    does not"""
    fids = [0, -1, 1]
    imgs, origs = [('image', i) for i in fids], [('original_image', i) for i in fids]
    return dict(name='fsnet_amd.vision_base.utils.builder.Sequential', cfg_list=[
        dict(name=AUG + '.ConvertToFloat'),
        dict(name=AUG + '.Resize', size=(h, w), preserve_aspect_ratio=False),
        dict(name=AUG + '.Normalize', mean=MEAN, stds=STD, image_keys=imgs),
        dict(name=AUG + '.Normalize', mean=np.zeros(3), stds=np.ones(3), image_keys=origs),
        dict(name=AUG + '.ConvertToTensor')],
        image_keys=imgs + origs if origs_in_image_keys else imgs, calib_keys=['P2'], gt_image_keys=['patched_mask'])


def direct_batch(samples, h, w, dev, fisheye=False):
    """the same samples collated on the host: numpy restatement of the resize and of Normalize.  `fisheye`: P2 is
    stacked as the tensors the samples hold, and the batch carries the samples' calib_meta"""
    import torch
    from oracle import augment_oracle as A
    direct = {}
    mean, std = MEAN.astype(np.float32), STD.astype(np.float32)
    for f in (0, -1, 1):
        res = [A.resize_linear(s[('image', f)].astype(np.float32), w, h) for s in samples]
        direct[('image', f)] = torch.from_numpy(np.stack([((r / np.float32(255.0) - mean) / std).transpose(2, 0, 1)
                                                          for r in res]).astype(np.float32))
        direct[('original_image', f)] = torch.from_numpy(np.stack([(r / np.float32(255.0)).transpose(2, 0, 1)
                                                                   for r in res]).astype(np.float32))
    for f in (-1, 1):
        direct[('relative_pose', f)] = torch.from_numpy(np.stack([s[('relative_pose', f)] for s in samples]))
    if fisheye:
        direct['P2'] = torch.stack([s['P2'] for s in samples])
        direct['calib_meta'] = [s['calib_meta'] for s in samples]
    else:
        direct['P2'] = torch.stack([torch.as_tensor(s['P2']) for s in samples])
    direct['patched_mask'] = torch.ones(len(samples), h, w, dtype=torch.float64)
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in direct.items()}


def step_losses(batches, make_model):
    """the loss of one training step per batch, each from a fresh `make_model()` in training mode"""
    import torch
    from fsnet_amd.configs import training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    losses = []
    for b in batches:
        m = make_model().train()
        tc = training_cfg()
        opt = build_optimizer(m, **tc.optimizer)
        hook = build(use_graph=False, **tc.training_hook)
        out = hook(dict(b), m, opt)
        torch.cuda.synchronize()
        losses.append(float(out["loss"].detach()))
    RT.set_compute_dtype(torch.bfloat16)
    return losses
