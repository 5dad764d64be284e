"""Seeded weights and inputs of the matching-encoder tests, shared by tools/gen_golden_matching.py (which feeds them
to the reference class) and the tests (which feed them to fsnet_amd's): no npz carries a ResNet's weights."""
import math

import numpy as np
import torch

# (h, w, D, C, B, F, binning, zero pose (sample, frame) or None, nearest bin): the op-level cases.  (Case b's 96 inverse
# bins start further out: from 0.5 m every pixel has a bin that leaves the image and no pixel is confident.)
OP_CASES = {
    "a": (16, 24, 8, 64, 2, 2, "linear", (1, 1), 0.5),
    "b": (16, 26, 96, 64, 1, 1, "inverse", None, 2.5),
    "c": (16, 24, 8, 256, 1, 2, "linear", None, 0.5),
}
MIN_BIN, MAX_BIN = 0.5, 20.0
MODULE = dict(depth=18, H=64, W=96, D=8, B=2, F=2)


def thin(a, limit):
    """every k-th element of the flattened array, at most ~limit of them (the same rule on both sides of a comparison)"""
    a = np.asarray(a).reshape(-1)
    return a[::max(1, int(math.ceil(a.size / float(limit))))]


def init_state(state_dict, seed):
    """seeded values for every entry of a state_dict (keys and shapes are the module's own)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in state_dict.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros(shape, dtype=v.dtype)
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            out[k] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3]
            out[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan)
        elif k.endswith("weight"):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        else:
            out[k] = 0.1 * torch.randn(shape, generator=g)
    return out


def pose(ry, tx, ty, tz):
    T = np.eye(4)
    c, s = math.cos(ry), math.sin(ry)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[0, 3], T[1, 3], T[2, 3] = tx, ty, tz
    return T


_POSES = [(0.013, 0.31, 0.0, -0.83), (-0.021, -0.27, 0.02, 0.91), (0.017, 0.22, -0.01, -0.64), (-0.011, -0.35, 0.0, 0.77)]


def poses_and_P2(B, F, h, w, zero=None):
    """generic poses (never the identity: it puts samples exactly on the edge thresholds) and intrinsics derived from the
    matching resolution h x w"""
    T = np.zeros((B, F, 4, 4))
    for b in range(B):
        for f in range(F):
            ry, tx, ty, tz = _POSES[(b * F + f) % len(_POSES)]
            T[b, f] = pose(ry * (1.0 + 0.1 * b), tx, ty, tz)
    if zero is not None:
        T[zero[0], zero[1]] = 0.0
    P2 = np.zeros((B, 3, 4))
    P2[:, 0, 0], P2[:, 1, 1], P2[:, 0, 2], P2[:, 1, 2], P2[:, 2, 2] = 0.58 * w, 1.92 * h, 0.5 * w, 0.5 * h, 1.0
    return torch.from_numpy(T).float(), torch.from_numpy(P2).float()


def _smooth(shape, g, k=5):
    t = torch.rand(shape, generator=g)
    return torch.nn.functional.avg_pool2d(t, k, 1, k // 2)


def op_inputs(name):
    """-> dict(cur [B,C,h,w], look [B,F,C,h,w], poses [B,F,4,4], P2 [B,3,4]): smooth non-negative features, the lookup
    frames shifted crops of the same field plus a little noise, so that the costs have a structure over the bins"""
    h, w, D, C, B, F, binning, zero, _ = OP_CASES[name]
    g = torch.Generator().manual_seed(1000 + ord(name))
    field = _smooth((B, C, h + 8, w + 8), g) * 2.0
    cur = field[:, :, 4:4 + h, 4:4 + w].contiguous()
    shifts = [(4, 2), (5, 7), (3, 5)]
    look = torch.stack([field[:, :, sy:sy + h, sx:sx + w] for sy, sx in (shifts[f % 3] for f in range(F))], 1)
    look = (look + 0.02 * torch.rand(look.shape, generator=g)).contiguous()
    poses, P2 = poses_and_P2(B, F, h, w, zero)
    return dict(cur=cur, look=look, poses=poses, P2=P2)


def module_inputs():
    """-> (current [B,3,H,W], lookup [B,F,3,H,W], poses, P2): smooth images so that the features correlate"""
    m = MODULE
    B, F, H, W = m["B"], m["F"], m["H"], m["W"]
    g = torch.Generator().manual_seed(3)
    base = _smooth((B, 3, H + 16, W + 16), g)
    cur = base[:, :, 8:8 + H, 8:8 + W].contiguous()
    look = torch.stack([base[:, :, 8:8 + H, 6:6 + W], base[:, :, 9:9 + H, 11:11 + W]], 1).contiguous()
    poses, P2 = poses_and_P2(B, F, H // 4, W // 4, zero=(1, 1))
    return cur, look, poses, P2
