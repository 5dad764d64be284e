"""Inputs and run helpers shared by tools/gen_golden.py::gen_dla (the reference's DLA classes on the CPU ->
tests/golden/dla.npz) and tests/test_dla_cpu.py / tests/test_dla_gpu.py (this project's module against that file)."""
import torch
import torch.nn as nn

from tests.helpers_dcn import deviation          # (max abs, rms) of a - ref in f64

FACTORIES = ["dla34", "dla46_c", "dla46x_c", "dla60x_c", "dla60", "dla60x", "dla102", "dla102x", "dla102x2", "dla169"]
INIT_SEED = 83            # torch seed of the freshly initialised dla34 whose per-key sums the fixture holds
# the two networks the fixture runs: N = 2 at 64 x 64 leaves 2 x 2 x 2 = 8 values per channel at level 5.  out_indices
# are what keeps the file below 1 MiB (the two full-resolution features of one network are 1 MiB as float32): DLA-34 as
# the depth encoder uses it, the small network with the base layer's feature instead of levels 0 and 1
NETS = {
    "dla34": dict(levels=[1, 1, 1, 2, 2, 1], channels=[16, 32, 64, 128, 256, 512], block="BasicBlock",
                  residual_root=False, out_indices=(1, 2, 3, 4, 5)),
    "small": dict(levels=[1, 1, 1, 2, 2, 1], channels=[16, 32, 64, 64, 128, 256], block="Bottleneck",
                  residual_root=True, out_indices=(-1, 2, 3, 4, 5)),
}
STATE_SEED = {"dla34": 84, "small": 85}
INPUT_SEED = {"dla34": 86, "small": 87}


def build_factory(mod, name):
    """mod.<name>(pretrained=None) with the class attributes the factories leave behind reset first (dla102x2 sets
    BottleneckX.cardinality = 64 for every model built after it)"""
    mod.BottleneckX.cardinality = 32
    mod.Bottleneck.expansion = 2
    return getattr(mod, name)(pretrained=None)


def build_net(mod, which):
    cfg = NETS[which]
    mod.Bottleneck.expansion = 2
    return mod.DLA(list(cfg["levels"]), list(cfg["channels"]), block=getattr(mod, cfg["block"]),
                   residual_root=cfg["residual_root"], out_indices=tuple(cfg["out_indices"]))


def net_state(model, which):
    from tests.helpers_matching import init_state
    return init_state(model.state_dict(), STATE_SEED[which])


def feature_shapes(channels, out_indices, N, H, W):
    """shapes of DLA.forward's list for an N x 3 x H x W batch"""
    shapes = [(N, channels[0], H, W)] if -1 in out_indices else []
    return shapes + [(N, channels[i], H >> i, W >> i) for i in range(6) if i in out_indices]


def net_inputs(which, N=2, H=64, W=64):
    """(image batch, one cotangent per returned feature), f64, seeded"""
    cfg = NETS[which]
    gen = torch.Generator().manual_seed(INPUT_SEED[which])
    x = torch.randn(N, 3, H, W, generator=gen, dtype=torch.float64)
    cots = [torch.randn(s, generator=gen, dtype=torch.float64) for s in feature_shapes(cfg["channels"], cfg["out_indices"], N, H, W)]
    return x, cots


def round_conv_operands_to_bf16(model):
    """the bf16 yardstick: every convolution reads its input and its weight rounded to bf16 (a forward pre-hook; the
    weight is rounded from a master copy kept on the module, the gradient lands on the parameter as usual)"""
    def hook(m, args):
        if not hasattr(m, "_master"):
            m._master = m.weight.detach().clone()
        m.weight.data.copy_(m._master.to(torch.bfloat16).to(m.weight.dtype))
        return (args[0].to(torch.bfloat16).to(args[0].dtype),)
    return [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, nn.Conv2d)]


def bn_buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def run_net(model, x, cots, dtype=None, device="cpu", forward=None):
    """training-mode forward and backward -> (features, {parameter or 'input': gradient}, names without gradient,
    BatchNorm buffers after the forward).  dtype: parameters and input are cast to it (the CPU runs); None leaves the
    parameters as they are and takes no input gradient (the HIP path reads a plain fp32 image batch)."""
    model = model.to(device=device).train() if dtype is None else model.to(device=device, dtype=dtype).train()
    xin = x.detach().to(device=device, dtype=(dtype or torch.float32)).clone()
    if dtype is not None:
        xin.requires_grad_()
    for p in model.parameters():
        p.grad = None
    feats = (forward or model)(xin)
    bufs = bn_buffers(model)
    # (.backward, not autograd.grad: the HIP runner accumulates into .grad from inside its one autograd node)
    torch.autograd.backward(feats, [c.to(device=device, dtype=f.dtype) for c, f in zip(cots, feats)])
    leaves = dict(model.named_parameters())
    if dtype is not None:
        leaves["input"] = xin
    grads = {k: p.grad.detach() for k, p in leaves.items() if p.grad is not None}
    return [f.detach() for f in feats], grads, sorted(k for k, p in leaves.items() if p.grad is None), bufs


def buffer_deviation(bufs, gold_bufs, suffix):
    """(max abs, rms) over every BatchNorm buffer with this suffix, concatenated in key order"""
    keys = sorted(k for k in gold_bufs if k.endswith(suffix))
    a = torch.cat([bufs[k].detach().double().cpu().flatten() for k in keys])
    b = torch.cat([torch.as_tensor(gold_bufs[k]).double().flatten() for k in keys])
    return deviation(a, b)
