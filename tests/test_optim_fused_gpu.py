"""The fused SGD / AdamW / Adam-L2 launch against torch.optim on CPU fp32 tensors (the objects the reference's
build_optimizer hands out): arithmetic over the sizes at which the loop shape changes, the run table (nothing outside a
run is touched), the step count read from device memory under graph replay, the training hook's captured step for
`sgd` and `adamw`, frozen weights under weight decay, and checkpoints moving between the fused classes and torch's."""
import functools

import pytest
import torch

from oracle import fsnet_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-6            # max |dp| on N(0,1) parameters, as test_ops_gpu.py::test_adam_and_clip
# 7: less than one 16-byte unit; 259: one block and a tail; 100003: test_adam_and_clip's; 4096*256 + 259: one element
# past a single pass of the capped grid at one element per thread; 4096*256*4 + 259: the same at the four elements per
# thread the kernel actually takes
SIZES = [7, 259, 100003, 4096 * 256 + 259, 4096 * 256 * 4 + 259]

SGD = [dict(momentum=m, dampening=d, nesterov=n, weight_decay=wd)
       for m, d, n in [(0.0, 0.0, False), (0.0, 0.5, False), (0.9, 0.0, False), (0.9, 0.0, True), (0.9, 0.5, False)]
       for wd in (0.0, 1e-4)]
CASES = ([("sgd", dict(lr=1e-2, **kw)) for kw in SGD]
         + [("adamw", dict(lr=1e-3, weight_decay=wd)) for wd in (0.0, 1e-2)]
         + [("adam", dict(lr=1e-3, weight_decay=1e-5))])
TORCH = {"sgd": torch.optim.SGD, "adamw": torch.optim.AdamW, "adam": torch.optim.Adam}


# The one case that cannot meet TOL against torch fp32, and why: Adam's L2 decay adds wd * p to the clipped gradient, and
# among 4M elements a few dozen land within ~1e-7 of zero, where the update lr * g / (|g| + eps) turns on g's last digits.
# torch's clip coefficient comes from an fp32 norm that is 1e-4 off at this size (the kernel's sum is f64), which moves
# exactly those elements: max |dp| against torch fp32 is 3.7e-5 at step 1.  For this case both sides are measured
# against torch in f64 (norm, clip and Adam in f64) and the kernel is allowed twice torch fp32's own error; the figures
# are printed by the test and recorded in docs/LAB_r07.md.
F64_YARDSTICK = {("adam", True, 4096 * 256 * 4 + 259)}


def _id(case):
    name, kw = case
    return name + "-" + "-".join("%s=%g" % (k[:4], float(v)) for k, v in kw.items() if k != "lr")


@functools.lru_cache(maxsize=None)
def _data(n):
    """N(0,1) parameters and three gradients (3 * N(0,1): a joint norm far above the clip threshold); shared, read-only"""
    g = torch.Generator().manual_seed(6 + n % 1000)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * 3 for _ in range(3)]


def _state_close(got, want, ulps):
    """a state array against torch's, in units of 2^-23 of its largest magnitude.  A buffer is a handful of fp32
    operations per step, each of which torch may round differently (fused multiply-add or not): 8 such units over three
    steps.  Not under the clip at large n: torch's fp32 gradient norm is itself 1e-4 off at 4M elements (measured
    against f64; the kernel's sum is f64), which scales every buffer entry; at n = 100003 it is 4e-7 off, under 4 units."""
    return float((got.cpu() - want).abs().max()) <= ulps * 2.0 ** -23 * float(want.abs().max())


def _kernel_step(ops, name, kw, pd, gd, state, step, max_norm=None, ss=None, **extra):
    if max_norm:
        ss.zero_()
        ops.sumsq(gd, ss)
        extra.update(max_norm=max_norm, sumsq_buf=ss)
    if name == "sgd":
        ops.sgd_step(pd, gd, state[0] if kw["momentum"] else None, kw["lr"], kw["momentum"], kw["dampening"],
                     kw["nesterov"], kw["weight_decay"], step, **extra)
    else:
        ops.adamw_step(pd, gd, state[0], state[1], kw["lr"], 0.9, 0.999, 1e-8, kw["weight_decay"], step,
                       decoupled=name == "adamw", **extra)


@pytest.mark.parametrize("clip", [None, 35.0], ids=["noclip", "clip35"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_matches_torch_optim(dev, case, clip):
    from fsnet_amd.hip import ops
    name, kw = case
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    for n in SIZES:
        p0, grads = _data(n)
        p = p0.clone().requires_grad_(True)
        opt = TORCH[name]([p], **kw)
        pd = p0.to(dev)
        state = [torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        f64 = (name, bool(clip), n) in F64_YARDSTICK
        if f64:
            p64 = p0.double().requires_grad_(True)
            opt64 = TORCH[name]([p64], **kw)
        for step, g in enumerate(grads, 1):
            p.grad = g.clone()
            if clip:
                torch.nn.utils.clip_grad_norm_([p], clip)
            opt.step()
            _kernel_step(ops, name, kw, pd, g.to(dev), state, step, clip, ss)
            err = float((pd.cpu() - p.detach()).abs().max())
            print("%s n=%d step %d: max |dp| %.3g" % (_id(case), n, step, err))
            if not f64:
                assert err < TOL, (n, step, err)
                continue
            p64.grad = g.double()
            torch.nn.utils.clip_grad_norm_([p64], clip)
            opt64.step()
            e_torch = float((p.detach().double() - p64.detach()).abs().max())
            e_kernel = float((pd.cpu().double() - p64.detach()).abs().max())
            print("    against torch f64: torch fp32 %.3g, kernel %.3g" % (e_torch, e_kernel))
            assert e_kernel <= 2 * e_torch, (n, step, e_kernel, e_torch)
        if name == "sgd" and not kw["momentum"]:
            assert not state[0].any()                      # no buffer was handed over, none written
        elif name == "sgd" and not clip:
            assert _state_close(state[0], opt.state[p]["momentum_buffer"], 8)


@pytest.mark.parametrize("case", [("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-4)),
                                  ("adamw", dict(lr=1e-3, weight_decay=1e-2)),
                                  ("adam", dict(lr=1e-3, weight_decay=1e-5))], ids=_id)
def test_run_table_touches_nothing_outside_its_runs(dev, case):
    from fsnet_amd.hip import ops
    from fsnet_amd.hip.binding import FsError
    name, kw = case
    n = 100003
    runs = [(4, 8), (256, 515), (n - 4, n)]
    inside = torch.zeros(n, dtype=torch.bool)
    for lo, hi in runs:
        inside[lo:hi] = True
    p0, grads = _data(n)
    g = grads[0]                                                # non-zero everywhere
    coef = min(35.0 / (float(g.norm()) + 1e-6), 1.0)
    p = p0[inside].clone().requires_grad_(True)                 # torch sees the trainable elements only
    opt = TORCH[name]([p], **kw)
    p.grad = g[inside] * coef
    opt.step()
    sentinel = 0.25
    state0 = torch.where(inside, torch.zeros(n), torch.full((n,), sentinel))
    pd, gd = p0.to(dev), g.to(dev)
    state = [state0.to(dev), state0.to(dev)]
    table = torch.tensor(runs, dtype=torch.int64, device=dev)
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    _kernel_step(ops, name, kw, pd, gd, state, 1, 35.0, ss, runs=table)
    torch.cuda.synchronize()
    got = pd.cpu()
    assert float((got[inside] - p.detach()).abs().max()) < TOL
    assert float((got[inside] - p0[inside]).abs().min()) > 0                        # every element of a run moved
    assert torch.equal(got[~inside], p0[~inside])
    for s in state:
        assert torch.equal(s.cpu()[~inside], state0[~inside])
    if name == "sgd":
        assert _state_close(state[0][inside], opt.state[p]["momentum_buffer"], 8)
        assert torch.equal(state[1].cpu(), state0)
    else:
        assert _state_close(state[0][inside], opt.state[p]["exp_avg"], 8)
    # a malformed table is refused before anything is launched
    before = [pd.clone(), state[0].clone(), state[1].clone()]
    for bad in ([(8, 4)], [(4, 8), (0, n + 1)], [(-4, 8)]):
        with pytest.raises(FsError):
            _kernel_step(ops, name, kw, pd, gd, state, 2, runs=torch.tensor(bad, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(pd, before[0]) and torch.equal(state[0], before[1]) and torch.equal(state[1], before[2])


def test_sgd_first_step_is_read_from_the_device_step_count(dev):
    """dampening != 0: torch's first step stores the gradient undamped, every later one damps it.  The launch is
    captured once (the host passes step 1, as the optimizer does) and replayed three times with the device counter
    running 1, 2, 3: a first step baked into the capture would fail steps 2 and 3"""
    from fsnet_amd.hip import ops
    from fsnet_amd.vision_base.pipeline_hooks.train_val_hooks import base_training_hooks
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.5, nesterov=False, weight_decay=1e-4)
    n = 100003
    p0, grads = _data(n)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([p], **kw)
    pd, gd, buf = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step_buf = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.counter_incr(step_buf)
        _kernel_step(ops, "sgd", kw, pd, gd, [buf], 1, step_buf=step_buf)
    base_training_hooks._PARKED.append(graph)           # (graphs are parked, not destroyed: see there)
    for step, g in enumerate(grads, 1):
        p.grad = g.clone()
        opt.step()
        gd.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert int(step_buf.item()) == step
        assert float((pd.cpu() - p.detach()).abs().max()) < TOL, step
        assert _state_close(buf, opt.state[p]["momentum_buffer"], 8), step


# ------------------------------------------------------------------------------------------------ the training hook
HOOK_OPT = {"sgd": dict(name="sgd", lr=1e-3, momentum=0.9, weight_decay=1e-4),
            "adamw": dict(name="adamw", lr=1e-4, weight_decay=1e-2),
            "adam": dict(name="adam", lr=1e-4, weight_decay=1e-2)}


def _run_hook(dev, optimizer, use_graph, steps, frozen_stages=-1):
    """64x128, batch 2, with_pose=True, fp32, as test_graph_gpu.py::_run"""
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    try:
        B, H, W = 2, 64, 128
        cfg = meta_arch_cfg(H, W, with_pose=True)
        cfg.depth_backbone_cfg.update(frozen_stages=frozen_stages)
        cfg.pose_backbone_cfg.update(frozen_stages=frozen_stages)
        m = build(**cfg)
        m.load_state_dict(O.init_state(seed=3, with_pose=True), strict=True)
        m = m.to(dev).train()
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        opt = build_optimizer(m, **dict(optimizer))
        hook = build(use_graph=use_graph, graph_warmup=2, **training_cfg().training_hook)
        for it in range(steps):
            hook(dict(O.synthetic_batch(B, H, W, seed=50 + it)), m, opt)
        torch.cuda.synchronize()
    finally:
        RT.set_compute_dtype(torch.bfloat16)
    return m, before, hook, opt


def _flat(m):
    return torch.cat([p.detach().double().flatten() for p in m.parameters()]).cpu()


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_hook_captures_and_replays_sgd_and_adamw(dev, name):
    me, _, he, oe = _run_hook(dev, HOOK_OPT[name], False, 6)
    m2, _, _, _ = _run_hook(dev, HOOK_OPT[name], False, 6)
    mg, _, hg, og = _run_hook(dev, HOOK_OPT[name], True, 6)
    assert he.graph_replays == 0 and he.graph_captures == 0
    assert hg.graph_captures == 1 and hg.graph_replays == 3          # steps 0,1 eager; 2 captured; 3..5 replayed
    assert oe._step_count_fused == og._step_count_fused == 6 and int(og._step_buf.item()) == 6
    pe, p2, pg = _flat(me), _flat(m2), _flat(mg)
    # the bound of test_graph_gpu.py::test_graph_replay_matches_eager (fp32): the spread between two eager runs
    spread, got = float((pe - p2).abs().max()), float((pe - pg).abs().max())
    print("%s: graph against eager %.3g, eager against eager %.3g" % (name, got, spread))
    assert got < max(2e-3, 5 * spread), (got, spread)


@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_frozen_weights_stay_put_under_weight_decay(dev, name):
    m, before, hook, opt = _run_hook(dev, dict(HOOK_OPT[name], weight_decay=1e-2), True, 3, frozen_stages=1)
    assert hook.graph_captures == 1 and opt._step_count_fused == 3      # two eager steps, the third captured
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == 30                                            # conv1, bn1, layer1 of both backbones
    assert opt._run_table(m._arena).shape == (2, 2)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert not torch.equal(p.detach(), before[k]), k
        else:
            assert torch.equal(p.detach(), before[k]), k


# ------------------------------------------------------------------------------------- a small arena, set by hand
class _Holder(torch.nn.Module):
    def __init__(self, tensors, device):
        super().__init__()
        from fsnet_amd.engine.runtime import ParamArena
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone().to(device)) for t in tensors])
        self._arena = ParamArena([("ps.%d" % i, p) for i, p in enumerate(self.ps)], device)


def _tensors(seed, shapes=((33, 7), (1,), (16, 3, 3, 3), (5,))):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def _set_grads(params, grads, scale=1.0):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.copy_(g * scale)


ARENA_OPT = [("sgd", dict(lr=1e-2, momentum=0.9, dampening=0.5, weight_decay=1e-2)),
             ("adamw", dict(lr=1e-3, weight_decay=1e-2))]


@pytest.mark.parametrize("name,kw", ARENA_OPT, ids=["sgd", "adamw"])
def test_checkpoint_round_trip_with_torch_optim(dev, name, kw):
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    init = _tensors(1)
    holder = _Holder(init, dev)
    fused = build_optimizer(holder, name=name, **kw)
    assert fused._arena() is holder._arena
    grads = [_tensors(10 + i) for i in range(4)]
    for i in range(2):
        _set_grads(holder.ps, grads[i])
        fused.step()
    sd = fused.state_dict()
    # fused -> torch: one more step on each side
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in holder.ps]
    ref = TORCH[name](cpu, **kw)
    ref.load_state_dict(sd)
    _set_grads(holder.ps, grads[2])
    _set_grads(cpu, grads[2])
    fused.step()
    ref.step()
    for a, b in zip(holder.ps, cpu):
        assert float((a.detach().cpu() - b.detach()).abs().max()) < TOL
    # torch -> fused: a fresh arena at torch's parameters, torch's checkpoint, one more step on each side
    holder2 = _Holder([p.detach() for p in cpu], dev)
    fused2 = build_optimizer(holder2, name=name, **kw)
    fused2.load_state_dict(ref.state_dict())
    _set_grads(holder2.ps, grads[3])
    _set_grads(cpu, grads[3])
    fused2.step()
    ref.step()
    for a, b in zip(holder2.ps, cpu):
        assert float((a.detach().cpu() - b.detach()).abs().max()) < TOL
    got, want = fused2.state_dict()["state"], ref.state_dict()["state"]
    assert set(got) == set(want)
    for k in want:
        assert set(got[k]) == set(want[k])
        for key, v in want[k].items():
            assert got[k][key].shape == v.shape
            # (the kernel forms 1 - beta2 in fp32, as the Adam kernel always has: 1 - fl(0.999) is 4.7e-5 above torch's
            # 1e-3, and exp_avg_sq carries that factor — 400 units of 2^-23; the parameters above are within TOL)
            assert _state_close(got[k][key], v, 1024 if key == "exp_avg_sq" else 8), (k, key)


@pytest.mark.parametrize("name,kw", ARENA_OPT + [("adam", dict(lr=1e-3, weight_decay=1e-2))], ids=["sgd", "adamw", "adam"])
def test_arena_step_follows_requires_grad_flips(dev, name, kw):
    """the 1-element parameter is frozen for two steps (torch: no gradient, skipped — weight decay included), then
    trained: the run table is rebuilt and the parameter moves.  (Its first update is not torch's: the fused optimizers
    keep one step count for the arena, torch one per parameter — DESIGN.md, "Run table".)"""
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    init = _tensors(2)
    holder = _Holder(init, dev)
    holder.ps[1].requires_grad = False
    fused = build_optimizer(holder, name=name, **kw)
    cpu = [torch.nn.Parameter(t.clone()) for t in init]
    ref = TORCH[name](cpu, **kw)
    for i in range(3):
        grads = _tensors(20 + i)
        if i == 2:
            holder.ps[1].requires_grad = True
        live = holder.ps[1].requires_grad
        if not live:
            grads[1] = torch.zeros(1)              # what the arena holds for a frozen parameter
        _set_grads(holder.ps, grads)
        _set_grads(cpu, grads)
        if not live:
            cpu[1].grad = None
        fused.step(max_norm=35.0)
        torch.nn.utils.clip_grad_norm_(cpu, 35.0)
        ref.step()
        table = fused._run_table(holder._arena)
        assert (table is None) == live
        if i < 2:
            assert table.tolist() == [[0, 232], [236, 676]]
            assert torch.equal(holder.ps[1].detach().cpu(), init[1])
        for k, (a, b) in enumerate(zip(holder.ps, cpu)):
            if k != 1:
                assert float((a.detach().cpu() - b.detach()).abs().max()) < TOL, (i, k)
    assert not torch.equal(holder.ps[1].detach().cpu(), init[1])
