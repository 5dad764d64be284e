"""BatchNorm (+ residual, + second BatchNorm, + ReLU, + replicated border) forward and backward restated in float64, the
a-priori error bounds of the HIP kernels' fp32 arithmetic against that restatement, the host-side launch geometry of
csrc/bn.hip, and the case list that tests/test_bn64_cpu.py (coverage) and tests/test_bn_paths_gpu.py (the sweep) share.
No GPU and no import of the extension: torch on the CPU only.

Error bounds (u = 2^-24, the unit roundoff of fp32; every bound is multiplied by SECOND = 1 + 2^-10 for the products of
two roundings, which are below 2^-20 of the first-order terms).  The kernels' operation order is the one in
csrc/bn_coeffs.h and csrc/bn.hip; a contraction of a multiply and an add into one fused operation only removes a
rounding, so each count is an upper limit.  The f64 steps (slot sums, moments, 1/sqrt, the atomics of the first
backward pass) round at 2^-53 and are covered by F64 = 2^-44 relative, far below u.

  coefficients (bn_coeffs.h: bn_coeffs)
    mean_f   = (float)m                          1 rounding                          u |m|
    invstd_f = (float)(1/sqrt(v + eps))          1 rounding                          u invstd
    scale_f  = gamma * invstd_f                  invstd_f (1) + product (1)          2u |scale|
    shift_f  = beta - mean_f * scale_f           mean_f (1) + scale_f (2) + product (1) = 4 on |mean scale|,
                                                 the subtraction 1 on |beta| + |mean scale|
                                                                                     u (|beta| + 5 |mean scale|)
  forward element  v = x * scale_f + shift_f  (bn.hip: bn_apply_kernel, both loops)
    x scale: scale_f (2) + product (1) + add (1) = 4;  mean scale: shift_f (5) + add (1) = 6;  beta: shift_f (1) + add (1) = 2
                                                 E_bn = u (4 |x scale| + 6 |mean scale| + 2 |beta|)
    + res: one more addition                     E = E_bn + u (|bn| + |res|)
    + bn2(res): the second BatchNorm's E_bn2 and the addition
                                                 E = E_bn + E_bn2 + u (|bn| + |bn2|)
    ReLU moves no error (|max(a,0) - max(b,0)| <= |a - b|).
    bf16 output: one round-to-nearest-even of the computed value; bf16 has 8 significand bits, so the unit roundoff
    is UB = 2^-8 (half the 2^-7 spacing of [1, 2)):                                E + UB (|y| + E)
  running statistics, one step per group  r' = (1 - mom) * r + mom * b   (bn_coeffs.h: bn_momentum, bn_running_update)
    (1 - mom) r: the fp32 difference 1 - mom (1) + product (1) + add (1) = 3
    mom b: b is mean_f (1) or (float)(var_b_f * count / (count - 1)) (2), product (1), add (1) = at most 4
    an earlier step's error is multiplied by (1 - mom) < 1:   sum over the groups of u (3 |(1 - mom) r| + 4 |mom b|)
  first backward pass (bn.hip: bn_bwd_reduce_kernel, reduce_tail)
    a thread adds its rows in fp32, the block folds its 256 / CGB pixel lanes through LDS in fp32, then f64 atomics.  A term
    passes through at most n = (rows of the thread) + (pixel lanes) fp32 additions (two rows per iteration add g0 + g1
    first and the pair second: never more than one addition per row).
    sum g:       g is exact (a masked input; a folded gradient is required to be exact in fp32, see `exact_f32`)
                                                 (n + 2) u sum|g|
    sum g xhat:  the term g * (x - mean_f) * invstd_f: the subtraction (1), invstd_f (1), two products (2) = 4 on |g xhat|;
                 and mean_f's own rounding, which the subtraction does not scale down: u |mean| invstd |g| per term
                                                 (n + 4) u sum|g xhat| + u |mean| invstd sum|g|
  parameter gradients  dgamma += (float)S  (bn.hip: bn_bwd_coeffs; G groups add with atomics, in any order)
    E_S per group, (float)S (1), and one rounding per addition on at most |start| + sum_g |S_g|
                                                 sum_g (E_Sg + u |S_g|) + G u (|start| + sum_g |S_g|)
  dx element  k * (g - a - xh * b),  xh = (x - mean_f) * invstd_f, a = (float)(S1 / count), b = (float)(S2 / count),
  k = gamma * invstd_f  (bn.hip: bn_dx)
    a: E_S1 / count + u |a|;  b: E_S2 / count + u |b|;  xh: u |mean| invstd + 3u |xh|;  k: 2u
    g:     g - a (1), the second subtraction (1), k (2) and the last product (1)               = 5
    a:     its own rounding (1) and the same four steps                                       = 6
    xh b:  b (1), xh (3), the product (1), the second subtraction (1), k and the last product (3)  = 9
                 E_dx = |k| (E_S1 / count + |xh| E_S2 / count + u |b| |mean| invstd + u (5 |g| + 6 |a| + 9 |xh b|))
    bf16 output:                                 E_dx + UB (|dx| + E_dx)
  g_out and the ReLU mask are exact: g_out is the masked gradient rounded once to the storage type.
"""
import zlib

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
SECOND = 1.0 + 2.0 ** -10
F64 = 2.0 ** -44
SLOTS = 8                                  # FS_STAT_SLOTS (include/fsnet_hip.h)
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # BN_EPS / BN_MOMENTUM as the float fields of the argument
MOM = float(torch.tensor(0.1, dtype=torch.float32))           # structs hold them
SENTINEL = 1024.0                          # fill of every output buffer: exact in bf16, far from every result

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def rnd(t, dtype):
    """f64 -> the storage type and back: the value the device tensor holds"""
    return t.to(DT[dtype] if isinstance(dtype, str) else dtype).double()


def exact_f32(t):
    return bool((t.float().double() == t).all())


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def slot_stats(x, G):
    """x f64 [N,H,W,C] -> (sum, sumsq) per statistics group as the conv epilogue leaves them: [G][SLOTS][2][C], the rows of a
    group dealt round-robin to the slots"""
    C = x.shape[-1]
    r = x.reshape(G, -1, C)
    out = torch.zeros(G, SLOTS, 2, C, dtype=torch.float64)
    for k in range(SLOTS):
        out[:, k, 0] = r[:, k::SLOTS].sum(1)
        out[:, k, 1] = (r[:, k::SLOTS] ** 2).sum(1)
    return out


def bn64_coeffs(stats, count, gamma, beta, rmean, rvar, G=1, eps=EPS, momentum=MOM):
    """one BatchNorm's per-(group, channel) coefficients and state updates, with their bounds"""
    train = stats is not None
    if train:
        s = stats.sum(1)                                   # [G][2][C]
        m = s[:, 0] / count
        v = (s[:, 1] / count - m * m).clamp_min(0.0)
    else:
        assert G == 1
        m, v = rmean[None].clone(), rvar[None].clone()
    invstd = 1.0 / torch.sqrt(v + eps)
    scale = gamma[None] * invstd
    shift = beta[None] - m * scale
    o = dict(mean=m, invstd=invstd, scale=scale, shift=shift, var=v)
    o["mean_b"] = SECOND * (U + F64) * m.abs()
    o["invstd_b"] = SECOND * (U + F64) * invstd
    o["scale_b"] = SECOND * (2 * U + F64) * scale.abs()
    o["shift_b"] = SECOND * (U + F64) * (beta[None].abs() + 5 * (m * scale).abs())
    rm, rv = rmean.clone(), rvar.clone()
    rm_b, rv_b = torch.zeros_like(rm), torch.zeros_like(rv)
    if train:
        for g in range(G):
            unb = v[g] * count / (count - 1.0) if count > 1.0 else v[g]
            rm_b += SECOND * U * (3 * ((1 - momentum) * rm).abs() + 4 * (momentum * m[g]).abs())
            rv_b += SECOND * U * (3 * ((1 - momentum) * rv).abs() + 4 * (momentum * unb).abs())
            rm = (1 - momentum) * rm + momentum * m[g]
            rv = (1 - momentum) * rv + momentum * unb
    o.update(running_mean=rm, running_var=rv, running_mean_b=rm_b, running_var_b=rv_b, nbt=G if train else 0)
    return o


def _affine(x, k, G):
    """x [N,H,W,C], k: bn64_coeffs -> (scale x + shift, E_bn) in x's shape"""
    C = x.shape[-1]
    r = x.reshape(G, -1, C)
    sc, sh, m, be = k["scale"][:, None], k["shift"][:, None], k["mean"][:, None], k["beta"][None, None]
    v = r * sc + sh
    e = U * (4 * (r * sc).abs() + 6 * (m * sc).abs() + 2 * be.abs()).expand_as(r)
    return v.reshape(x.shape), e.reshape(x.shape)


def _pad_replicate(t):
    """[N,H,W,C] -> [N,H+2,W+2,C] with a replicated border (index copies: exact)"""
    t = torch.cat([t[:, :1], t, t[:, -1:]], 1)
    return torch.cat([t[:, :, :1], t, t[:, :, -1:]], 2)


def bn64(x, stats, count, gamma, beta, running_mean, running_var, res=None, stats2=None, gamma2=None, beta2=None,
         running_mean2=None, running_var2=None, relu=True, bn2=False, pad_out=False, groups=1, train=True, eps=EPS, momentum=MOM,
         out_dtype="f32"):
    """Forward.  Operands are f64 tensors that hold storage-type values, NHWC; stats [G][SLOTS][2][C] f64 (ignored in eval
    mode: train=False normalises with the running statistics and updates nothing).  -> dict: y (padded when pad_out),
    y_b (its bound), pre (before the ReLU), bn / bn2 (per-BatchNorm dicts of bn64_coeffs: mean, invstd, scale, shift,
    running_mean, running_var, nbt, each with <name>_b)."""
    G = max(groups, 1)
    k1 = bn64_coeffs(stats if train else None, count, gamma, beta, running_mean, running_var, G, eps, momentum)
    k1["beta"] = beta
    v, e = _affine(x, k1, G)
    out = dict(bn=k1, bn2=None)
    if bn2:
        assert res is not None
        k2 = bn64_coeffs(stats2 if train else None, count, gamma2, beta2, running_mean2, running_var2, G, eps, momentum)
        k2["beta"] = beta2
        v2, e2 = _affine(res, k2, G)
        e = e + e2 + U * (v.abs() + v2.abs())
        v = v + v2
        out["bn2"] = k2
    elif res is not None:
        e = e + U * (v.abs() + res.abs())
        v = v + res
    y = v.clamp_min(0.0) if relu else v
    e32 = e = SECOND * e
    if out_dtype == "bf16":
        e = e + UB * (y.abs() + e)
    if pad_out:
        y, e, e32 = _pad_replicate(y), _pad_replicate(e), _pad_replicate(e32)
    out.update(y=y, y_b=e, y_b32=e32, pre=v)
    return out


def fold_border(dp):
    """gradient on the replicate-padded grid [N,H+2,W+2,C] -> on the map [N,H,W,C]: every border copy adds onto its edge
    pixel (H, W >= 2)"""
    assert dp.shape[1] >= 4 and dp.shape[2] >= 4
    g = dp[:, 1:-1, 1:-1].clone()
    g[:, 0] += dp[:, 0, 1:-1]
    g[:, -1] += dp[:, -1, 1:-1]
    g[:, :, 0] += dp[:, 1:-1, 0]
    g[:, :, -1] += dp[:, 1:-1, -1]
    g[:, 0, 0] += dp[:, 0, 0]
    g[:, 0, -1] += dp[:, 0, -1]
    g[:, -1, 0] += dp[:, -1, 0]
    g[:, -1, -1] += dp[:, -1, -1]
    return g


def bn64_backward(x, dout, act, k, gamma, count, chain, relu=True, fold=False, groups=1, dgamma0=None, dbeta0=None,
                  exchange=None, out_dtype="f32"):
    """Backward of one BatchNorm.  dout: the gradient w.r.t. the block output, [N,H,W,C] or (fold) on the padded grid;
    act: the activation whose sign is the ReLU mask (None without relu); k: the forward's coefficient dict (mean, invstd
    per group); chain: the longest fp32 addition chain of the first pass (launch_paths()["chain"]); exchange: f(sums) -> the
    sums after the data-parallel exchange (dx from those, the parameter gradients from the local ones).
    -> dict: g (= g_out), sums [G][2][C] with sums_b, dx with dx_b, dgamma / dbeta with their bounds."""
    G = max(groups, 1)
    C = x.shape[-1]
    g = fold_border(dout) if fold else dout.clone()
    if relu:
        g = torch.where(act > 0, g, torch.zeros_like(g))
    m, istd = k["mean"][:, None], k["invstd"][:, None]                # [G][1][C]
    xr, gr = x.reshape(G, -1, C), g.reshape(G, -1, C)
    xh = (xr - m) * istd
    S1, S2 = gr.sum(1), (gr * xh).sum(1)                               # [G][C]
    A1, A2 = gr.abs().sum(1), (gr * xh).abs().sum(1)
    S1_b = SECOND * ((chain + 2) * U + F64) * A1
    S2_b = SECOND * (((chain + 4) * U + F64) * A2 + U * k["mean"].abs() * k["invstd"] * A1)
    sums = torch.stack([S1, S2], 1)
    E1, E2 = S1_b, S2_b
    X1, X2 = S1, S2
    if exchange is not None:
        ex = exchange(sums)
        X1, X2 = ex[:, 0], ex[:, 1]
        E1, E2 = exchange(torch.stack([S1_b, S2_b], 1)).unbind(1)
    a, b = (X1 / count)[:, None], (X2 / count)[:, None]
    kk = (gamma[None] * k["invstd"])[:, None]
    dx = kk * (gr - a - xh * b)
    e = kk.abs() * (E1[:, None] / count + xh.abs() * E2[:, None] / count + U * b.abs() * m.abs() * istd
                    + U * (5 * gr.abs() + 6 * a.abs() + 9 * (xh * b).abs()))
    e32 = e = SECOND * e
    if out_dtype == "bf16":
        e = e + UB * (dx.abs() + e)
    dg0 = dgamma0 if dgamma0 is not None else torch.zeros(C, dtype=torch.float64)
    db0 = dbeta0 if dbeta0 is not None else torch.zeros(C, dtype=torch.float64)
    dgamma, dbeta = dg0 + S2.sum(0), db0 + S1.sum(0)
    dgamma_b = SECOND * ((S2_b + U * S2.abs()).sum(0) + G * U * (dg0.abs() + S2.abs().sum(0)))
    dbeta_b = SECOND * ((S1_b + U * S1.abs()).sum(0) + G * U * (db0.abs() + S1.abs().sum(0)))
    return dict(g=g, sums=sums, sums_b=torch.stack([S1_b, S2_b], 1), dx=dx.reshape(x.shape), dx_b=e.reshape(x.shape), dx_b32=e32.reshape(x.shape),
                dgamma=dgamma, dbeta=dbeta, dgamma_b=dgamma_b, dbeta_b=dbeta_b)


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry: arithmetic copied from fsnet_amd/csrc/bn.hip (line numbers of that file)
#   bn_slabs :862, grid_for :867-880, dtype_lanes :982
#   fs_bn_apply2 (grid, LDS) :1023-1025; bn_apply_kernel: slab decode :109-111, fast-path condition :158-168
#   fs_bn_bwd_apply2 (grid, LDS) :1064-1074; bn_bwd_apply_kernel: slab decode :759-761, fast-path condition :790-795
#   fs_bn_bwd_reduce2 (CGB, rows per block, cap) :1049-1053; launch_reduce (grid) :993-996;
#   bn_bwd_reduce_kernel: lanes, `act`, row walk :645-647, :691-696, the bf16 ring :705-725; reduce_tail (LDS fold) :467-471
# ---------------------------------------------------------------------------------------------------------------------
def bn_slabs(CG):
    return CG // 32 if (CG > 32 and (CG & (CG - 1)) == 0) else 1


def grid_for(items):
    return int(max(1, min((items + 255) // 256, 512)))


def _counts(total, stride):
    """items per thread of a grid-stride walk: (min, max) over the threads i0 = 0 .. stride - 1"""
    per = lambda i0: 0 if i0 >= total else -(-(total - i0) // stride)
    return per(stride - 1), per(0)


def launch_paths(C, dtype, M, G=1, dense_y=True, dense_grad=True, has2=False):
    vec = 8 if dtype == "bf16" else 4
    assert C % 8 == 0 and M % G == 0
    CG = C // vec
    pow2 = (CG & (CG - 1)) == 0
    nslab = bn_slabs(CG)
    Mg = M // G
    # the two element-wise passes share their grid
    items = Mg * CG
    gx = min(grid_for(items // nslab), max(32, grid_for(1 << 40) // nslab))
    SCG = 32 if nslab > 1 else CG
    shift_ok = nslab > 1 or pow2
    total, stride = Mg * SCG, gx * 256
    ew_min, ew_max = _counts(total, stride)
    p = dict(lanes=CG, pow2=pow2, slabs=nslab, vec=vec, rows=Mg,
             ew_grid=(gx, nslab, G), ew_total=total, ew_stride=stride, ew_min=ew_min, ew_max=ew_max,
             ew_ragged=total % stride != 0,
             fwd_fast=dense_y and shift_ok, bwd_fast=dense_grad and shift_ok,
             fwd_lds=(4 if has2 else 2) * (C // nslab) * 4, bwd_lds=5 * (C // nslab) * 4)
    # first backward pass
    if CG >= 32:
        CGB, rpb, cap = 32, 16, max(32, min(512, 1024 // (((CG + 31) // 32) * G)))
    elif CG >= 8:
        CGB, rpb, cap = 8, 64, 1024
    elif CG >= 4:
        CGB, rpb, cap = 4, 128, 1024
    else:
        CGB, rpb, cap = 2, 256, 1024
    PL = 256 // CGB
    rgx = min((Mg + rpb - 1) // rpb, cap)
    rgy = (CG + CGB - 1) // CGB
    r_min, r_max = _counts(Mg, rgx * PL)
    p.update(cgb=CGB, pixel_lanes=PL, red_grid=(rgx, rgy, G), red_cap=cap, red_stride=rgx * PL, red_min=r_min, red_max=r_max,
             red_ragged=Mg % (rgx * PL) != 0, ring=dtype == "bf16" and dense_grad, half_active=CG % CGB != 0,
             chain=r_max + PL)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """one BatchNorm launch set: forward, and (train mode) both backward passes.
    res: None | "res" | "bn2";  pad: padded output + folded gradient;  strided: y and dout are interior views of larger
    buffers;  sync: count = 2 M with doubled sums and an exchange that doubles;  start: dgamma / dbeta start non-zero"""

    def __init__(self, C, dtype, N, H, W, res=None, relu=True, pad=False, strided=False, G=1, train=True, g_out=False, sync=False,
                 start=False, large=False):
        self.C, self.dtype, self.N, self.H, self.W = C, dtype, N, H, W
        self.res, self.relu, self.pad, self.strided, self.G, self.train = res, relu, pad, strided, G, train
        self.g_out = g_out or res is not None
        self.sync, self.start, self.large = sync, start, large
        self.M = N * H * W
        flags = [res or "plain"] + [n for n, f in (("norelu", not relu), ("pad", pad), ("strided", strided), ("G%d" % G, G > 1),
                                                   ("eval", not train), ("gout", g_out), ("sync", sync), ("start", start)) if f]
        self.id = "%d-%s-%dx%dx%d-%s" % (C, dtype, N, H, W, "-".join(flags))

    @property
    def backward(self):
        return self.train

    def paths(self):
        dense = not (self.pad or self.strided)
        return launch_paths(self.C, self.dtype, self.M, self.G, dense_y=dense, dense_grad=dense, has2=self.res == "bn2")


def _cases():
    cs = []
    both = ("f32", "bf16")
    for dt in both:
        # narrowest lanes: launch_reduce<2> (and <4> at 16 channels fp32); one row per thread or none on the 2x3 map
        for C in (8, 16):
            for shape in ((1, 2, 3), (2, 6, 10)):
                cs.append(Case(C, dt, *shape))
                cs.append(Case(C, dt, *shape, res="res"))
        # CGB 4 / 2 with a half-active last block (24 channels bf16: 3 lanes; 24 fp32 / 48 bf16: 6 lanes), 12 lanes for <8>
        for C in (16, 24, 32, 48) + ((96,) if dt == "bf16" else ()):
            cs.append(Case(C, dt, 3, 5, 7))
            cs.append(Case(C, dt, 3, 5, 7, g_out=True))
        # padded output, folded gradient
        for C in (16, 24, 64):
            for shape in ((2, 2, 2), (3, 10, 14), (2, 7, 2)):
                cs.append(Case(C, dt, *shape, pad=True))
                cs.append(Case(C, dt, *shape, pad=True, G=2 if shape[0] % 2 == 0 else 3))
                cs.append(Case(C, dt, *shape, pad=True, res="res"))
        # strided, not padded
        cs.append(Case(32, dt, 2, 6, 10, strided=True))
        cs.append(Case(32, dt, 2, 6, 10, strided=True, res="res"))
        # statistics groups outside POOL mode
        for C in (16, 64):
            cs.append(Case(C, dt, 4, 6, 10, G=2, g_out=True, start=True))
            cs.append(Case(C, dt, 6, 3, 5, G=3, g_out=True, start=True))
        # eval mode
        for C in (24, 64):
            cs.append(Case(C, dt, 2, 6, 10, res="res", train=False))
            cs.append(Case(C, dt, 2, 6, 10, res="bn2", train=False))
    # 48 lanes: launch_reduce<32> with a half-active second block, the generic loop with the whole row's coefficients in LDS
    cs.append(Case(192, "f32", 2, 3, 5, res="res"))
    cs.append(Case(384, "bf16", 2, 3, 5, res="res"))
    # channel slabs with the second BatchNorm: 2 slabs (64 lanes) and 4 (128 lanes)
    for C, dt in ((512, "bf16"), (256, "f32"), (1024, "bf16"), (512, "f32")):
        cs.append(Case(C, dt, 2, 4, 6, res="bn2"))
        cs.append(Case(C, dt, 2, 4, 6, res="bn2", train=False))
    # SyncBN: the count of two shards, the exchanged sums
    cs.append(Case(32, "f32", 2, 6, 10, sync=True))
    # rings with four rounds and a ragged last one (sized from launch_paths: see test_bn64_cpu.py), and a walk of 2-3 rounds
    cs.append(Case(16, "bf16", 4, 256, 385, large=True))
    cs.append(Case(512, "bf16", 2, 64, 97, res="bn2", large=True))
    cs.append(Case(64, "f32", 4, 50, 100, res="res", large=True))
    return cs


CASES = _cases()
FINALIZE_CASES = [(C, G, train) for C in (16, 64) for G in (1, 2) for train in (True, False) if train or G == 1]


def make_inputs(case):
    """every operand of a case as f64 tensors holding storage-type values (deterministic per case id)"""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    N, H, W, C, G = c.N, c.H, c.W, c.C, c.G
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().double()

    def params():
        return dict(gamma=f32(1 + 0.2 * rn(C)), beta=f32(0.1 * rn(C)), running_mean=f32(0.3 * rn(C)),
                    running_var=f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64)))
    world = 2.0 if c.sync else 1.0
    d = dict(x=rnd(rn(N, H, W, C) * 2 + 0.5, c.dtype), bn=params(), count=world * (c.M // G))
    d["stats"] = slot_stats(d["x"], G) * world
    if c.res is not None:
        d["res"] = rnd(rn(N, H, W, C), c.dtype)
    if c.res == "bn2":
        d["bn2"] = params()
        d["stats2"] = slot_stats(d["res"], G) * world
    if c.backward:
        if c.pad:
            # multiples of 1/32 below 4: exact in bf16, and every sum of four of them is exact in fp32 — the folded
            # gradient is then the same number in the kernel and here
            d["dout"] = torch.randint(-127, 128, (N, H + 2, W + 2, C), generator=g).double() / 32
        else:
            d["dout"] = rnd(rn(N, H, W, C), c.dtype)
        d["dgamma0"] = f32(rn(C)) if c.start else torch.zeros(C, dtype=torch.float64)
        d["dbeta0"] = f32(rn(C)) if c.start else torch.zeros(C, dtype=torch.float64)
    return d


def forward_reference(case, d):
    c = case
    kw = {}
    if c.res is not None:
        kw["res"] = d["res"]
    if c.res == "bn2":
        kw.update(bn2=True, stats2=d["stats2"], gamma2=d["bn2"]["gamma"], beta2=d["bn2"]["beta"],
                  running_mean2=d["bn2"]["running_mean"], running_var2=d["bn2"]["running_var"])
    fw = bn64(d["x"], d["stats"], d["count"], d["bn"]["gamma"], d["bn"]["beta"], d["bn"]["running_mean"], d["bn"]["running_var"],
              relu=c.relu, pad_out=c.pad, groups=c.G, train=c.train, out_dtype=c.dtype, **kw)
    return fw


def reference(case, d=None):
    """-> (inputs, forward dict, backward dict or None, second BatchNorm's backward dict or None)"""
    c = case
    d = d if d is not None else make_inputs(c)
    fw = forward_reference(c, d)
    if not c.backward:
        return d, fw, None, None
    act = rnd(fw["y"], c.dtype)
    act_int = act[:, 1:-1, 1:-1] if c.pad else act
    ex = (lambda s: 2.0 * s) if c.sync else None
    chain = c.paths()["chain"]
    bw = bn64_backward(d["x"], d["dout"], act_int, fw["bn"], d["bn"]["gamma"], d["count"], chain, relu=c.relu, fold=c.pad, groups=c.G,
                       dgamma0=d["dgamma0"], dbeta0=d["dbeta0"], exchange=ex, out_dtype=c.dtype)
    bw["act"] = act
    bw2 = None
    if c.res == "bn2":
        # the downsample branch's BatchNorm: its gradient is g_out as stored, no ReLU of its own
        gin = rnd(bw["g"], c.dtype)
        bw2 = bn64_backward(d["res"], gin, None, fw["bn2"], d["bn2"]["gamma"], d["count"], chain, relu=False, groups=c.G,
                            out_dtype=c.dtype)
        bw2["gin"] = gin
    return d, fw, bw, bw2
