"""Host side of the three arena optimizers, without a GPU: what build_optimizer / adopt_optimizer hand out, how the run
table of trainable parameters is cut from a ParamArena, torch.optim's state_dict layout, and the step without an arena
(which is torch.optim's own)."""
import copy

import pytest
import torch
import torch.nn as nn

from fsnet_amd.engine.runtime import ParamArena
from fsnet_amd.vision_base.networks.optimizers import optimizers as OPT


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(5, 3), nn.Linear(3, 2))


CASES = [("sgd", OPT.FusedSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-2)),
         ("sgd", OPT.FusedSGD, torch.optim.SGD, dict(lr=0.1)),
         ("adamw", OPT.FusedAdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2))]


@pytest.mark.parametrize("name,fused_cls,torch_cls,kw", CASES)
def test_build_optimizer_returns_the_fused_subclasses(name, fused_cls, torch_cls, kw):
    m = _net()
    opt = OPT.build_optimizer(m, name=name, **kw)
    assert type(opt) is fused_cls and isinstance(opt, torch_cls) and isinstance(opt, OPT.ArenaOptimizer)
    ref = torch_cls(_net().parameters(), **kw)
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == \
           {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    with pytest.raises(ValueError):
        OPT.build_optimizer(m, name=name, lr=-1.0)            # torch's own constructor validation


def test_adam_is_still_the_fused_adam():
    opt = OPT.build_optimizer(_net(), name="adam", lr=1e-4)
    assert type(opt) is OPT.FusedAdam and isinstance(opt, OPT.ArenaOptimizer)


@pytest.mark.parametrize("name,fused_cls,torch_cls,kw", CASES)
def test_adopt_optimizer_adopts_torch_sgd_and_adamw(name, fused_cls, torch_cls, kw):
    from fsnet_amd.engine.torch_compat import adopt_optimizer
    m = _net()
    plain = torch_cls(m.parameters(), **kw)
    fused = adopt_optimizer(plain, m)
    assert type(fused) is fused_cls and adopt_optimizer(plain, m) is fused and adopt_optimizer(fused, m) is fused
    assert fused.param_groups is plain.param_groups and fused.state is plain.state
    assert fused.param_groups[0]["lr"] == kw["lr"]
    # not over exactly the module's parameters, or with an option the kernel does not implement: left alone
    part = torch_cls(list(m.parameters())[:2], **kw)
    assert adopt_optimizer(part, m) is part
    odd = torch_cls(m.parameters(), maximize=True, **kw)
    assert adopt_optimizer(odd, m) is odd


class _Holder:
    pass


def _arena(shapes, frozen):
    ps = [nn.Parameter(torch.randn(*s)) for s in shapes]
    for i in frozen:
        ps[i].requires_grad = False
    return ParamArena([("p%d" % i, p) for i, p in enumerate(ps)], torch.device("cpu"))


SHAPES = [(3, 5), (7,), (2, 2), (6,)]          # slots (padded to 4): [0,16) [16,24) [24,28) [28,36)


@pytest.mark.parametrize("frozen,want", [
    ((), [(0, 36)]),
    ((0,), [(16, 36)]),
    ((3,), [(0, 28)]),
    ((0, 2), [(16, 24), (28, 36)]),
    ((1, 3), [(0, 16), (24, 28)]),
    ((0, 1, 2, 3), []),
])
def test_run_table_merges_adjacent_trainable_slots(frozen, want):
    arena = _arena(SHAPES, frozen)
    assert arena.total == 36
    assert OPT.trainable_runs(arena) == want


def test_run_table_boundary_on_a_padded_slot():
    """a frozen 1-element bias between two trainable tensors: its slot is 4 elements wide, both runs end on a 16-byte
    boundary and the padding of the trainable 5-element tensor in front belongs to that tensor's run"""
    arena = _arena([(5,), (1,), (9,)], (1,))
    assert arena.offsets == [0, 8, 12] and arena.total == 24
    assert OPT.trainable_runs(arena) == [(0, 8), (12, 24)]


def test_run_mask_follows_requires_grad_flips():
    arena = _arena(SHAPES, ())
    holder = _Holder()
    holder._arena = arena
    opt = OPT.FusedSGD(arena.params, lr=0.1, model=holder)
    assert opt._arena() is arena and opt.run_mask(arena) is None and opt._run_table(arena) is None
    arena.params[1].requires_grad = False
    assert opt.run_mask(arena) == (True, False, True, True)
    assert opt._run_table(arena).tolist() == [[0, 16], [24, 36]] and opt._run_table(arena).dtype == torch.int64
    first = opt._run_table(arena)
    assert opt._run_table(arena) is first                       # built once per mask
    arena.params[1].requires_grad = True
    assert opt.run_mask(arena) is None and opt._run_table(arena) is None


def test_hook_signature_carries_the_update_constants_and_the_run_mask():
    """what is baked into a captured launch re-captures when it changes: momentum / dampening / nesterov / weight decay
    and which parameters are trainable"""
    from fsnet_amd.vision_base.pipeline_hooks.train_val_hooks.base_training_hooks import BaseTrainingHook
    arena = _arena(SHAPES, ())
    holder = _Holder()
    holder._arena = arena
    opt = OPT.FusedSGD(arena.params, lr=0.1, momentum=0.9, model=holder)
    hook = BaseTrainingHook(clip_gradients=35.0, use_graph=False)
    data = {"x": torch.zeros(2, 3)}
    sig0 = hook._signature(data, holder, opt, arena)
    assert hook._signature(data, holder, opt, arena) == sig0
    opt.param_groups[0]["lr"] = 0.01                            # read from device memory: not part of the signature
    assert hook._signature(data, holder, opt, arena) == sig0
    for key, value in (("momentum", 0.5), ("dampening", 0.1), ("nesterov", True), ("weight_decay", 1e-3)):
        old = opt.param_groups[0][key]
        opt.param_groups[0][key] = value
        assert hook._signature(data, holder, opt, arena) != sig0, key
        opt.param_groups[0][key] = old
    arena.params[2].requires_grad = False
    assert hook._signature(data, holder, opt, arena) != sig0
    arena.params[2].requires_grad = True
    assert hook._signature(data, holder, opt, arena) == sig0


@pytest.mark.parametrize("opts", [dict(maximize=True), dict(foreach=True), dict(differentiable=True)])
def test_options_the_kernel_lacks_leave_the_arena_path(opts):
    arena = _arena(SHAPES, ())
    holder = _Holder()
    holder._arena = arena
    assert OPT.FusedSGD(arena.params, lr=0.1, model=holder, **opts)._arena() is None
    assert OPT.FusedAdamW(arena.params, lr=0.1, model=holder, **opts)._arena() is None
    assert OPT.FusedAdamW(arena.params, lr=0.1, model=holder, amsgrad=True)._arena() is None
    two = OPT.FusedSGD([dict(params=arena.params[:2]), dict(params=arena.params[2:])], lr=0.1, model=holder)
    assert two._arena() is None


@pytest.mark.parametrize("name,fused_cls,torch_cls,kw", CASES)
def test_plain_step_and_state_dict_are_torch_optims(name, fused_cls, torch_cls, kw):
    """no arena (a CPU Linear): step() is torch.optim's to the bit, state_dict() has its keys and shapes, and a
    checkpoint moves between the two classes in both directions"""
    ma, mb = _net(), _net()
    a = OPT.build_optimizer(ma, name=name, **kw)
    b = torch_cls(mb.parameters(), **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            pa.grad = torch.randn(pa.shape, generator=g)
            pb.grad = pa.grad.clone()
        a.step()
        b.step()
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and set(sa["state"]) == set(sb["state"])
    for k in sb["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
        for name_, v in sb["state"][k].items():
            if torch.is_tensor(v):
                assert sa["state"][k][name_].shape == v.shape and torch.equal(sa["state"][k][name_], v)
            else:
                assert sa["state"][k][name_] == v
    b2 = torch_cls(_net().parameters(), **kw)
    b2.load_state_dict(copy.deepcopy(sa))
    a2 = OPT.build_optimizer(_net(), name=name, **kw)
    a2.load_state_dict(copy.deepcopy(sb))
    assert set(a2.state_dict()["state"]) == set(sb["state"])


def test_plain_step_takes_the_hooks_clip_and_scale():
    """the hook hands max_norm / grad_scale to every arena optimizer: without an arena they are clip_grad_norm_ and a
    gradient scale in front of torch.optim's step"""
    ma, mb = _net(), _net()
    a = OPT.build_optimizer(ma, name="sgd", lr=0.1, momentum=0.9)
    b = torch.optim.SGD(mb.parameters(), lr=0.1, momentum=0.9)
    g = torch.Generator().manual_seed(2)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        pa.grad = torch.randn(pa.shape, generator=g) * 10
        pb.grad = pa.grad.clone() * 0.5
    a.step(max_norm=1.0, grad_scale=0.5)
    torch.nn.utils.clip_grad_norm_(mb.parameters(), 1.0)
    b.step()
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
