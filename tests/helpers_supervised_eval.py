"""Oracle and inputs of the supervised KITTI depth metrics: a vectorised float64 numpy restatement of the reference's
compute_errors (monodepth/evaluation/kitti_supervised_eval.py:7-81, a per-pixel double loop), pinned to the REAL function
by tests/golden/supervised_eval.npz (tests/test_supervised_eval_cpu.py), and the seeded uint16 pairs both are run on —
shared by tools/gen_golden.py::gen_supervised_eval and the tests."""
import numpy as np

NAMES = ["mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log", "abs relative",
         "squared relative"]
GOLDEN_SHAPES = ((7, 9), (37, 123))


def u16_pair(H, W, seed, valid=0.25):
    """(gt, pred) uint16 [H, W]: predictions >= 256 (1 m and more); ground truth about `valid` non-zero, of which a few
    are 1 or 2 (<= 0.01 after / 256: not counted), the rest 2 .. 80 m with the prediction within a factor ~1.5"""
    rng = np.random.RandomState(seed)
    gt = rng.randint(512, 80 * 256, size=(H, W))
    pred = np.clip(gt * np.exp(rng.uniform(-0.4, 0.4, size=(H, W))), 256, 65535).astype(np.uint16)
    gt[rng.rand(H, W) > valid] = 0
    tiny = rng.rand(H, W) < 0.03
    gt[tiny] = rng.randint(1, 3, size=int(tiny.sum()))
    return gt.astype(np.uint16), pred


def sums(image_gt, image_pred):
    """float64 images -> (the nine normalised / finalised errors, n_valid, the radicand of slot 6)"""
    gt = np.asarray(image_gt, np.float64)
    pred = np.asarray(image_pred, np.float64)
    m = gt > 0.01
    g, p = gt[m], pred[m]
    n = float(g.size)
    d = np.abs(p - g)
    d2 = d ** 2
    di = np.abs(1.0 / g - 1.0 / p)
    dl = np.abs(np.log(p) - np.log(g))
    log_sum = np.sum(np.log(g) - np.log(p))
    e = np.zeros(9)
    with np.errstate(invalid="ignore", divide="ignore"):
        e[0] = np.sum(d) / n
        e[1] = np.sqrt(np.sum(d2) / n)
        e[2] = np.sum(di) / n
        e[3] = np.sqrt(np.sum(di ** 2) / n)
        e[4] = np.sum(dl) / n
        nsl = np.sum(dl ** 2) / n
        e[5] = np.sqrt(nsl)
        radicand = nsl - (log_sum ** 2 / (n ** 2))
        e[6] = np.sqrt(radicand)
        e[7] = np.sum(d / g) / n
        e[8] = np.sum(d2 / (g ** 2)) / n
    return e, int(n), radicand, nsl


def compute_errors(image_gt, image_pred):
    return sums(image_gt, image_pred)[0]
