"""csrc/bn.hip on every launch path against the float64 restatement of tests/helpers_bn64.py, element for element, under
bounds derived from the kernels' operation count (that module's docstring) — not against torch's fp32 batch_norm and
not under max-normalised tolerances.  tests/test_bn64_cpu.py checks the restatement itself and that this case list takes
every branch.  Each comparison prints its worst error / bound ratio (DESIGN.md "BatchNorm against float64").

One bound differs from the figure this sweep was planned with: a bf16 result was to be allowed 2^-9 |ref| for its one
rounding to storage.  bf16 has 8 significand bits; round-to-nearest errs by up to half a spacing, 2^-8 relative (1 + 2^-8
lies halfway between the neighbours 1 and 1 + 2^-7), so 2^-9 is below what a correctly rounded store can meet and the
bound here is 2^-8 (helpers_bn64.UB).  The ratio against the 2^-9 form is printed beside it (`vs 2^-9`): measured on the
MI355X it is 1.47 to 1.99 for `y` and `dx` of every bf16 case, as the format dictates."""
import numpy as np
import pytest
import torch

from tests import helpers_bn64 as B

pytestmark = pytest.mark.gpu


def to_dev(t, dtype, dev):
    return t.to(B.DT[dtype]).to(dev)


def framed(c, dev, fill=None):
    """-> (buffer filled with the sentinel, the view the kernel is handed): the padded grid, the interior of a larger
    buffer (strided, not padded), or a dense tensor"""
    N, H, W, C = c.N, c.H, c.W, c.C
    dt = B.DT[c.dtype]
    if c.pad:
        buf = torch.full((N, H + 2, W + 2, C), B.SENTINEL, dtype=dt, device=dev)
        view = buf
    elif c.strided:
        buf = torch.full((N, H + 2, W + 3, C), B.SENTINEL, dtype=dt, device=dev)
        view = buf[:, 1:1 + H, 2:2 + W]
    else:
        buf = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev)
        view = buf
    if fill is not None:
        view.copy_(to_dev(fill, c.dtype, dev))
    return buf, view


class Ledger:
    """element-by-element comparisons of one case; every quantity is looked at before the first failure is raised"""

    def __init__(self, case_id, dtype):
        self.id, self.dtype, self.bad = case_id, dtype, []

    def check(self, name, got, ref, bound, alt=None):
        got = got.detach().double().cpu().reshape(ref.shape)
        err = (got - ref).abs()
        bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
        ok = err <= bound
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
        extra = ""
        if alt is not None:
            extra = "  vs 2^-9 %.3f" % float((err / alt.clamp_min(1e-300)).max())
        print("bn64 %-44s %-5s %-14s err/bound %.3f%s" % (self.id, self.dtype, name, ratio, extra))
        if not bool(ok.all()):
            i = int((~ok).reshape(-1).nonzero()[0])
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
            self.bad.append("%s: %d of %d elements out of bound, first at %s: got %r ref %r bound %.3g" % (
                name, int((~ok).sum()), ok.numel(), idx, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                float(bound.reshape(-1)[i])))

    def same(self, name, got, ref):
        self.check(name, got, ref, 0.0)

    def done(self):
        assert not self.bad, "%s\n  " % self.id + "\n  ".join(self.bad)


def bn_tensors(p, dev, nbt=5):
    f = lambda t: t.float().to(dev)
    return {"weight": f(p["gamma"]), "bias": f(p["beta"]), "running_mean": f(p["running_mean"]),
            "running_var": f(p["running_var"]), "num_batches_tracked": torch.full((), nbt, dtype=torch.long, device=dev)}


def new_state(ops, C, dev, G, affine=False):
    st = ops.BnState(C, dev, groups=G, affine=affine)
    for t in (st.mean, st.invstd, st.scale, st.shift):
        if t is not None:
            t.fill_(B.SENTINEL)
    return st


def check_state(L, tag, k, st, bn, train, nbt0=5):
    L.check("save_mean" + tag, st.mean, k["mean"], k["mean_b"])
    L.check("save_invstd" + tag, st.invstd, k["invstd"], k["invstd_b"])
    if train:
        L.check("running_mean" + tag, bn["running_mean"], k["running_mean"], k["running_mean_b"])
        L.check("running_var" + tag, bn["running_var"], k["running_var"], k["running_var_b"])
    else:
        L.same("running_mean" + tag, bn["running_mean"], k["running_mean"])
        L.same("running_var" + tag, bn["running_var"], k["running_var"])
    assert int(bn["num_batches_tracked"]) == nbt0 + k["nbt"]


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_bn_launch_path_against_float64(dev, case):
    from fsnet_amd.hip import ops
    c = case
    d, fw, bw, bw2 = B.reference(c)
    N, H, W, C, G = c.N, c.H, c.W, c.C, c.G
    L = Ledger(c.id, c.dtype)
    x = to_dev(d["x"], c.dtype, dev)
    bn = bn_tensors(d["bn"], dev)
    st = new_state(ops, C, dev, G)
    stats = d["stats"].reshape(G * B.SLOTS, 2, C).to(dev) if c.train else None
    kw, bn2, st2, res = {}, None, None, None
    if c.res is not None:
        res = kw["res"] = to_dev(d["res"], c.dtype, dev)
    if c.res == "bn2":
        bn2, st2 = bn_tensors(d["bn2"], dev), new_state(ops, C, dev, G)
        kw.update(bn2=bn2, st2=st2, stats2=d["stats2"].reshape(G * B.SLOTS, 2, C).to(dev) if c.train else None)
    ybuf, yview = framed(c, dev)
    ops.bn_apply(x, stats, bn, st, yview, H, W, d["count"], relu=c.relu, pad_out=c.pad, groups=G, **kw)
    torch.cuda.synchronize()
    # forward: y with every border element of a padded output; the frame around a strided view keeps its sentinel
    alt = fw["y_b32"] + 2.0 ** -9 * (fw["y"].abs() + fw["y_b32"]) if c.dtype == "bf16" else None
    L.check("y", yview, fw["y"], fw["y_b"], alt)
    if c.strided:
        frame = ybuf.clone()
        frame[:, 1:1 + H, 2:2 + W] = B.SENTINEL
        assert bool((frame == B.SENTINEL).all()), "bn_apply wrote outside the strided view"
    check_state(L, "", fw["bn"], st, bn, c.train)
    if bn2 is not None:
        check_state(L, "2", fw["bn2"], st2, bn2, c.train)
    if c.backward:
        # backward: the mask is the reference activation rounded to storage (test_bn64_cpu.py::test_mask_guard)
        _, act = framed(c, dev, fill=bw["act"])
        if c.pad:
            act = act[:, 1:-1, 1:-1]
            dout = to_dev(d["dout"], c.dtype, dev)
        else:
            _, dout = framed(c, dev, fill=d["dout"])
        dt = B.DT[c.dtype]
        dx = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev)
        gout = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev) if c.g_out else None
        dgam, dbet = d["dgamma0"].float().to(dev), d["dbeta0"].float().to(dev)
        sums = torch.zeros(G * B.SLOTS, 2, C, dtype=torch.float64, device=dev)
        ops.bn_backward(dout, act, x, bn["weight"], st, dx, dgam, dbet, H, W, relu=c.relu, fold=c.pad, g_out=gout, sums=sums,
                        allreduce=(lambda s_, out: torch.mul(s_, 2.0, out=out)) if c.sync else None)
        torch.cuda.synchronize()
        L.check("sums", sums.reshape(G, B.SLOTS, 2, C).sum(1), bw["sums"], bw["sums_b"])
        alt = bw["dx_b32"] + 2.0 ** -9 * (bw["dx"].abs() + bw["dx_b32"]) if c.dtype == "bf16" else None
        L.check("dx", dx, bw["dx"], bw["dx_b"], alt)
        L.check("dgamma", dgam, bw["dgamma"], bw["dgamma_b"])
        L.check("dbeta", dbet, bw["dbeta"], bw["dbeta_b"])
        if gout is not None:
            L.same("g_out", gout, B.rnd(bw["g"], c.dtype))
        if bw2 is not None:
            # the downsample branch's BatchNorm takes g_out as its gradient: no mask, no activation
            dx2 = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev)
            dg2, db2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            sums2 = torch.zeros(G * B.SLOTS, 2, C, dtype=torch.float64, device=dev)
            ops.bn_backward(gout, None, res, bn2["weight"], st2, dx2, dg2, db2, H, W, relu=False, sums=sums2)
            torch.cuda.synchronize()
            L.check("sums2", sums2.reshape(G, B.SLOTS, 2, C).sum(1), bw2["sums"], bw2["sums_b"])
            L.check("dx2", dx2, bw2["dx"], bw2["dx_b"])
            L.check("dgamma2", dg2, bw2["dgamma"], bw2["dgamma_b"])
            L.check("dbeta2", db2, bw2["dbeta"], bw2["dbeta_b"])
    L.done()


@pytest.mark.parametrize("C,G,train", B.FINALIZE_CASES)
def test_bn_finalize_against_float64(dev, C, G, train):
    """fs_bn_finalize: the coefficients alone — save_mean / save_invstd, scale / shift per (group, channel), the running
    statistics after G steps"""
    from fsnet_amd.hip import ops
    g = torch.Generator().manual_seed(100 + C + G)
    x = torch.randn(2 * G, 3, 5, C, generator=g, dtype=torch.float64) * 2 + 0.5
    f32 = lambda t: t.float().double()
    p = dict(gamma=f32(1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)), beta=f32(0.1 * torch.randn(C, generator=g, dtype=torch.float64)),
             running_mean=f32(0.3 * torch.randn(C, generator=g, dtype=torch.float64)),
             running_var=f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64)))
    stats = B.slot_stats(x, G) if train else None
    count = float(x.numel() // C // G)
    k = B.bn64_coeffs(stats, count, p["gamma"], p["beta"], p["running_mean"], p["running_var"], G)
    bn = bn_tensors(p, dev)
    st = new_state(ops, C, dev, G, affine=True)
    ops.bn_finalize(stats.reshape(G * B.SLOTS, 2, C).to(dev) if train else None, bn, st, C, count, groups=G)
    torch.cuda.synchronize()
    L = Ledger("finalize-%d-G%d-%s" % (C, G, "train" if train else "eval"), "f32")
    check_state(L, "", k, st, bn, train)
    L.check("scale", st.scale, k["scale"], k["scale_b"])
    L.check("shift", st.shift, k["shift"], k["shift_b"])
    L.done()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H,W", [(1, 5), (5, 1), (1, 1)])
def test_single_row_or_column_map_is_refused_with_padding(dev, dtype, H, W):
    """pad_out (forward) and fold (both backward passes) on a map with H < 2 or W < 2 would leave a border line unwritten or
    unfolded (bn.hip: for_pad_sites): FS_EINVAL, and nothing is launched — every output keeps its sentinel"""
    from fsnet_amd.hip import ops
    from fsnet_amd.hip.binding import FsError
    N, C = 2, 16
    dt = B.DT[dtype]
    g = torch.Generator().manual_seed(7)
    x64 = B.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype)
    x = to_dev(x64, dtype, dev)
    p = dict(gamma=torch.ones(C), beta=torch.zeros(C), running_mean=torch.zeros(C), running_var=torch.ones(C))
    bn = bn_tensors(p, dev)
    st = new_state(ops, C, dev, 1)
    y = torch.full((N, H + 2, W + 2, C), B.SENTINEL, dtype=dt, device=dev)
    stats = B.slot_stats(x64, 1).reshape(B.SLOTS, 2, C).to(dev)
    with pytest.raises(FsError):
        ops.bn_apply(x, stats, bn, st, y, H, W, N * H * W, relu=True, pad_out=True)
    torch.cuda.synchronize()
    assert bool((y == B.SENTINEL).all()) and bool((st.mean == B.SENTINEL).all()) and bool((st.invstd == B.SENTINEL).all())
    assert bool((bn["running_mean"] == 0).all()) and bool((bn["running_var"] == 1).all()) and int(bn["num_batches_tracked"]) == 5
    # the same map without the border is served
    yd = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev)
    ops.bn_apply(x, stats, bn, st, yd, H, W, N * H * W, relu=True)
    torch.cuda.synchronize()
    assert not bool((yd == B.SENTINEL).any())
    for phase in ("all", "apply"):
        dx = torch.full((N, H, W, C), B.SENTINEL, dtype=dt, device=dev)
        dg, db = torch.full((C,), 3.0, device=dev), torch.full((C,), 4.0, device=dev)
        sums = torch.zeros(B.SLOTS, 2, C, dtype=torch.float64, device=dev)
        dout = torch.ones(N, H + 2, W + 2, C, dtype=dt, device=dev)
        with pytest.raises(FsError):
            ops.bn_backward(dout, y[:, 1:-1, 1:-1], x, bn["weight"], st, dx, dg, db, H, W, relu=True, fold=True, sums=sums, phase=phase)
        torch.cuda.synchronize()
        assert bool((dx == B.SENTINEL).all()) and bool((sums == 0).all()) and bool((dg == 3).all()) and bool((db == 4).all())
