"""Inputs and run helpers shared by tools/gen_golden_convnext.py (the reference's ConvNeXt classes on the CPU ->
tests/golden/convnext.npz) and tests/test_convnext_cpu.py / tests/test_convnext_gpu.py (this project's module against it)."""
import torch
import torch.nn as nn

from tests.helpers_dcn import deviation          # noqa: F401  ((max abs, rms) of a - ref in f64)

FACTORIES = {"convnext_tiny": ([3, 3, 9, 3], [96, 192, 384, 768]), "convnext_small": ([3, 3, 27, 3], [96, 192, 384, 768]),
             "convnext_base": ([3, 3, 27, 3], [128, 256, 512, 1024]), "convnext_large": ([3, 3, 27, 3], [192, 384, 768, 1536]),
             "convnext_xlarge": ([3, 3, 27, 3], [256, 512, 1024, 2048])}
INIT_SEED = 91            # torch seed of the freshly initialised convnext_tiny(in_chans=6) whose per-key sums the fixture holds
# small networks: no factory is needed to go wrong.  24, 40, 72 and 136 channels all leave channel padding behind; "odd"
# has no layer scale, six input channels, floors in both directions (36 x 44 -> 9 x 11, 4 x 5, 2 x 2, 1 x 1) and skips features
NETS = {
    "small": dict(dims=[24, 40, 72, 136], depths=[2, 1, 2, 1], in_chans=3, out_indices=(0, 1, 2, 3), N=2, H=64, W=64, extra={}),
    "odd": dict(dims=[24, 40, 72, 136], depths=[1, 1, 1, 1], in_chans=6, out_indices=(1, 3), N=3, H=36, W=44,
                extra=dict(layer_scale_init_value=0)),
}
STATE_SEED = {"small": 92, "odd": 93}
INPUT_SEED = {"small": 94, "odd": 95}
PROJ_SEED = 96


def build_net(mod, which, **over):
    cfg = NETS[which]
    kw = dict(in_chans=cfg["in_chans"], depths=list(cfg["depths"]), dims=list(cfg["dims"]),
              out_indices=tuple(cfg["out_indices"]), **cfg["extra"])
    kw.update(over)
    return mod.ConvNeXt(**kw)


def net_state(model, which):
    from tests.helpers_matching import init_state
    return init_state(model.state_dict(), STATE_SEED[which])


def feature_shapes(which, N=None):
    cfg = NETS[which]
    shapes, h, w = [], cfg["H"] // 4, cfg["W"] // 4
    for i in range(4):
        if i in cfg["out_indices"]:
            shapes.append((N or cfg["N"], cfg["dims"][i], h, w))
        h, w = h // 2, w // 2
    return shapes


def net_inputs(which, N=None):
    """(image batch, one cotangent per returned feature), f64, seeded.  The cotangents hold bf16 values: a feature comes
    back in the compute dtype and its gradient with it, and the cast must not be an error of its own"""
    cfg = NETS[which]
    gen = torch.Generator().manual_seed(INPUT_SEED[which])
    x = torch.randn(N or cfg["N"], cfg["in_chans"], cfg["H"], cfg["W"], generator=gen, dtype=torch.float64)
    return x, [torch.randn(s, generator=gen, dtype=torch.float64).to(torch.bfloat16).double() for s in feature_shapes(which, N)]


def round_operands_to_bf16(model):
    """the bf16 yardstick: every nn.Conv2d and nn.Linear reads its input and its weight rounded to bf16 (a forward
    pre-hook; the weight is rounded from a master copy kept on the module, the gradient lands on the parameter as usual)"""
    def hook(m, args):
        if not hasattr(m, "_master"):
            m._master = m.weight.detach().clone()
        m.weight.data.copy_(m._master.to(torch.bfloat16).to(m.weight.dtype))
        return (args[0].to(torch.bfloat16).to(args[0].dtype),)
    return [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]


def run_net(model, x, cots, dtype=None, device="cpu", forward=None):
    """training-mode forward and backward -> (features, {parameter: gradient}, names without gradient).  dtype: parameters
    and input are cast to it (the CPU runs); None leaves the parameters as they are (the HIP path reads an fp32 batch)"""
    model = model.to(device=device).train() if dtype is None else model.to(device=device, dtype=dtype).train()
    xin = x.detach().to(device=device, dtype=(dtype or torch.float32)).clone()
    for p in model.parameters():
        p.grad = None
    feats = (forward or model)(xin)
    # (.backward, not autograd.grad: the HIP runner accumulates into .grad from inside its one autograd node)
    torch.autograd.backward(feats, [c.to(device=device, dtype=f.dtype) for c, f in zip(cots, feats)])
    leaves = dict(model.named_parameters())
    grads = {k: p.grad.detach() for k, p in leaves.items() if p.grad is not None}
    return [f.detach() for f in feats], grads, sorted(k for k, p in leaves.items() if p.grad is None)


def is_gemm_param(name):
    """parameters whose gradient the convolution launches write — the weights of the pointwise and patch layers (the
    fixture holds their norm and one projection); every other gradient — depthwise weight and bias, every LayerNorm, gamma,
    and every bias — is written by convnext.hip and held in full"""
    if not name.endswith(".weight"):
        return False
    if ".pwconv" in name:
        return True
    return name.startswith("downsample_layers.") and name.split(".")[2] == ("0" if name.startswith("downsample_layers.0.") else "1")


def projection_vectors(names_shapes):
    """one N(0, 1) vector per GEMM parameter, seeded, in the order given: for a deviation delta, <delta, r> has standard
    deviation ||delta||"""
    gen = torch.Generator().manual_seed(PROJ_SEED)
    return {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in names_shapes}
