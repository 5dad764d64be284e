"""File readers of the KITTI raw layout with the reference's names (monodepth/data/datasets/utils.py:22-54):
PNG decode through PIL exactly like the reference's read_image, 16-bit ground-truth depth / 256, the MATLAB-devkit
pose file, velodyne scans, and the camera-frame relative poses."""
import numpy as np
import scipy.io as sio
from PIL import Image


def read_image(path):
    """[H, W, 3] uint8 RGB (reference :22-30)"""
    return np.array(Image.open(path, 'r'))


def read_depth(path):
    """16-bit PNG / 256 -> float32 metres (reference :32-40 reads it with cv2.imread(path, -1))"""
    return np.array(np.asarray(Image.open(path, 'r'), dtype=np.float64) / 256.0, dtype=np.float32)


def read_pose_mat(path):
    """[N, 4, 4] imu-to-world poses written by the MATLAB devkit (reference :42-50)"""
    return sio.loadmat(path)['pose_mat']


def read_pc_from_bin(bin_path):
    """velodyne scan: float32 [N, 4] = x, y, z, reflectance (reference :8-11)"""
    return np.fromfile(bin_path, dtype=np.float32).reshape(-1, 4)


def cam_relative_pose_nusc(T_imu2world_0, T_imu2world_1, T_imu2cam):
    """pose of camera frame 0 expressed in camera frame 1 from imu-to-world poses and one imu-to-camera transform
    (reference :56-57; the KITTI-360 fisheye reader passes inv(T_cam2pose))"""
    return T_imu2cam @ np.linalg.inv(T_imu2world_1) @ T_imu2world_0 @ np.linalg.inv(T_imu2cam)


def cam_relative_pose(T_imu2world_0, T_imu2world_1, T_imu2vel, T_vel2cam):
    """pose of camera frame 0 expressed in camera frame 1 (reference :53-54)"""
    return T_vel2cam @ T_imu2vel @ np.linalg.inv(T_imu2world_1) @ T_imu2world_0 @ np.linalg.inv(T_imu2vel) \
        @ np.linalg.inv(T_vel2cam)


def get_transformation_matrix(translation, rotation):
    """T [4, 4] from a translation [x, y, z] and a quaternion [w, x, y, z] (reference :59-67)"""
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[0:3, 0:3] = Rotation.from_quat([rotation[1], rotation[2], rotation[3], rotation[0]]).as_matrix()
    T[0:3, 3] = translation
    return T


def read_vo_depth(path):
    """sparse visual-odometry depth, 16-bit PNG -> float64 metres: / 65535 * 120, values < 3 or > 80 set to 120 (the
    reference's marker for "no point"; postopt_utils.py:50-53 reads it with cv2.imread(path, -1))"""
    d = np.asarray(Image.open(path, 'r'), dtype=np.float64) / 65535.0 * 120
    d[d < 3] = 120
    d[d > 80] = 120
    return d


def read_motion_mask(path):
    """[H, W] uint8 as written by the precompute hooks (reference mono_dataset.py:241-244 reads it with
    cv2.imread(path, IMREAD_UNCHANGED))"""
    return np.array(Image.open(path, 'r'))


def read_png16(path):
    """16-bit truecolour PNG (colour type 2, bit depth 16, not interlaced) -> uint16 [H, W, 3] in file channel order;
    16-bit greyscale (colour type 0: KITTI depth maps) -> uint16 [H, W].
    PIL opens the truecolour files as 8-bit RGB, so this decodes them with zlib: IHDR, the IDAT stream, filters 0-4.
    Filters None, Sub and Up are vectorised per row (a 375x1242 file in ~20 ms); Average and Paeth rows step one pixel at a
    time in numpy (seconds for a 375x1242 file made only of them).  write_png16 writes filter 0."""
    import struct
    import zlib
    with open(path, 'rb') as f:
        blob = f.read()
    if blob[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError("%s is not a PNG file" % path)
    pos, idat, hdr = 8, [], None
    while pos < len(blob):
        n, kind = struct.unpack('>I4s', blob[pos:pos + 8])
        body = blob[pos + 8:pos + 8 + n]
        if kind == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            break
        pos += 12 + n
    W, H, depth, ctype, _, _, interlace = hdr
    if depth != 16 or ctype not in (0, 2) or interlace != 0:
        raise ValueError("%s: only 16-bit RGB or greyscale non-interlaced PNGs are read here (bit depth %d, colour "
                         "type %d)" % (path, depth, ctype))
    bpp = 6 if ctype == 2 else 2
    stride = W * bpp
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8).reshape(H, stride + 1)
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(H):
        ft, line = raw[y, 0], raw[y, 1:].astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 1:        # Sub: a running sum along each of the bpp byte lanes
            cur = np.cumsum(line.reshape(W, bpp), axis=0).reshape(-1) & 255
        elif ft == 2:        # Up
            cur = (line + prev) & 255
        elif ft in (3, 4):   # Average / Paeth: sequential along the row, one pixel (bpp lanes) per step
            cur = np.zeros(stride, np.int64)
            a = np.zeros(bpp, np.int64)
            c = np.zeros(bpp, np.int64)
            for x in range(0, stride, bpp):
                b = prev[x:x + bpp]
                if ft == 3:
                    pr = (a + b) >> 1
                else:
                    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
                    pr = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
                a = (line[x:x + bpp] + pr) & 255
                cur[x:x + bpp] = a
                c = b
        else:
            raise ValueError("%s: PNG filter type %d" % (path, ft))
        out[y] = cur
        prev = cur
    img = out.reshape(H, W, bpp // 2, 2).astype(np.uint16) @ np.array([256, 1], np.uint16)
    return img if ctype == 2 else img[:, :, 0]


def write_png16(path, img):
    """uint16 [H, W, 3] -> 16-bit truecolour PNG, uint16 [H, W] -> 16-bit greyscale PNG (filter 0): the formats
    read_png16 reads"""
    import struct
    import zlib
    img = np.ascontiguousarray(np.asarray(img, '>u2'))
    H, W = img.shape[:2]
    ctype = 0 if img.ndim == 2 else 2
    raw = b''.join(b'\x00' + img[y].tobytes() for y in range(H))

    def chunk(kind, body):
        return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 16, ctype, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw)) + chunk(b'IEND', b''))


def read_flow_png(path):
    """precomputed flow (reference mono_dataset.py:246-250): cv2.imread(path, IMREAD_UNCHANGED)[:, :, 0:2] is BGR,
    i.e. the file's channels (2, 1); (v - 2^15) / 64 in fp32 -> [H, W, 2]"""
    v = read_png16(path)[:, :, [2, 1]]
    return (v.astype(np.float32) - 2 ** 15) / 64.0
