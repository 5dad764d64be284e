"""ConvNeXt backbone (reference vision_base/networks/models/backbone/convnext.py; Liu et al., "A ConvNet for the 2020s"):
the reference's module tree, registration order, state_dict keys and initialisation, so that its checkpoints load.

  downsample_layers.0      Conv2d(in_chans, d0, 4, stride 4) -> LayerNorm(channels_first)
  downsample_layers.1-3    LayerNorm(channels_first) -> Conv2d(d_{i-1}, d_i, 2, stride 2)
  stages.i.j               Block: dwconv 7x7 -> LayerNorm -> Linear(d, 4d) -> GELU -> Linear(4d, d) -> gamma * . -> x + drop_path(.)
  norm                     nn.LayerNorm(d3): registered, initialised, never called (no gradient)

Four features (strides 4, 8, 16, 32), the stage loop stopping after the last requested one.  The depth decoder reads five
levels, so this is a pose encoder (PoseDecoder reads the last feature) or a stand-alone backbone.  Kept from the
reference: forward_features returns None, num_classes / head_init_scale / unknown keyword arguments are swallowed, gamma is
None for layer_scale_init_value <= 0, drop_path is nn.Identity at rate 0, the "convnext-xt" key, convNext's default
pretrained=True, and any input size is accepted (the patch convolutions floor).

A CPU batch runs forward_torch (plain torch, any dtype); a CUDA batch runs the HIP engine
(fsnet_amd/engine/convnext_net.py).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from fsnet_amd.vision_base.networks.blocks.blocks import DropPath


class LayerNorm(nn.Module):
    """LayerNorm over the channel axis of a channels_last [N, H, W, C] or channels_first [N, C, H, W] tensor"""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        if self.data_format == "channels_last":
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        mean = x.mean(1, keepdim=True)
        var = (x - mean).pow(2).mean(1, keepdim=True)
        xhat = (x - mean) / torch.sqrt(var + self.eps)
        return self.weight[:, None, None] * xhat + self.bias[:, None, None]


class Block(nn.Module):
    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = (nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True)
                      if layer_scale_init_value > 0 else None)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, x):
        y = self.dwconv(x).permute(0, 2, 3, 1)
        y = self.pwconv2(self.act(self.pwconv1(self.norm(y))))
        if self.gamma is not None:
            y = self.gamma * y
        return x + self.drop_path(y.permute(0, 3, 1, 2))


class ConvNeXt(nn.Module):
    def __init__(self, in_chans=3, num_classes=1000, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.,
                 layer_scale_init_value=1e-6, head_init_scale=1., out_indices=(0, 1, 2, 3), **kwargs):
        super().__init__()
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4),
            LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(
                LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths), device="cpu")]
        self.stages = nn.ModuleList()
        first = 0
        for i in range(4):
            self.stages.append(nn.Sequential(*[
                Block(dim=dims[i], drop_path=rates[first + j], layer_scale_init_value=layer_scale_init_value)
                for j in range(depths[i])]))
            first += depths[i]
        self.norm = nn.LayerNorm(dims[-1], eps=1e-6)
        self.apply(self._init_weights)
        self.out_indices = out_indices
        self._runner = None         # engine.convnext_net.ConvNeXtRunner, built at the first CUDA forward
        self._pending = 0
        self._plist = None

    def _init_weights(self, m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=.02)
            nn.init.constant_(m.bias, 0)

    def forward_features(self, x):
        for i in range(4):
            x = self.stages[i](self.downsample_layers[i](x))
        return

    def forward_torch(self, x):
        """plain torch over the module's parameters (any device, any dtype)"""
        outputs = []
        for i in range(max(self.out_indices) + 1):
            x = self.stages[i](self.downsample_layers[i](x))
            if i in self.out_indices:
                outputs.append(x)
        return outputs

    def forward(self, x):
        if not x.is_cuda:
            return self.forward_torch(x)
        from fsnet_amd.engine.convnext_net import run_convnext
        return run_convnext(self, x)


model_urls = {
    "convnext_tiny_1k": "https://dl.fbaipublicfiles.com/convnext/convnext_tiny_1k_224_ema.pth",
    "convnext_small_1k": "https://dl.fbaipublicfiles.com/convnext/convnext_small_1k_224_ema.pth",
    "convnext_base_1k": "https://dl.fbaipublicfiles.com/convnext/convnext_base_1k_224_ema.pth",
    "convnext_large_1k": "https://dl.fbaipublicfiles.com/convnext/convnext_large_1k_224_ema.pth",
    "convnext_base_22k": "https://dl.fbaipublicfiles.com/convnext/convnext_base_22k_224.pth",
    "convnext_large_22k": "https://dl.fbaipublicfiles.com/convnext/convnext_large_22k_224.pth",
    "convnext_xlarge_22k": "https://dl.fbaipublicfiles.com/convnext/convnext_xlarge_22k_224.pth",
}


def _make(depths, dims, url_key, check_hash, kwargs):
    model = ConvNeXt(depths=depths, dims=dims, **kwargs)
    if url_key is not None:
        extra = dict(check_hash=True) if check_hash else {}
        checkpoint = torch.hub.load_state_dict_from_url(url=model_urls[url_key], map_location="cpu", **extra)
        model.load_state_dict(checkpoint["model"], strict=False)
    return model


def convnext_tiny(pretrained=False, **kwargs):
    return _make([3, 3, 9, 3], [96, 192, 384, 768], "convnext_tiny_1k" if pretrained else None, True, kwargs)


def convnext_small(pretrained=False, **kwargs):
    return _make([3, 3, 27, 3], [96, 192, 384, 768], "convnext_small_1k" if pretrained else None, False, kwargs)


def convnext_base(pretrained=False, in_22k=False, **kwargs):
    key = ("convnext_base_22k" if in_22k else "convnext_base_1k") if pretrained else None
    return _make([3, 3, 27, 3], [128, 256, 512, 1024], key, False, kwargs)


def convnext_large(pretrained=False, in_22k=False, **kwargs):
    key = ("convnext_large_22k" if in_22k else "convnext_large_1k") if pretrained else None
    return _make([3, 3, 27, 3], [192, 384, 768, 1536], key, False, kwargs)


def convnext_xlarge(pretrained=False, in_22k=False, **kwargs):
    if pretrained:
        assert in_22k, "only ImageNet-22K pre-trained ConvNeXt-XL is available; please set in_22k=True"
    return _make([3, 3, 27, 3], [256, 512, 1024, 2048], "convnext_xlarge_22k" if pretrained else None, False, kwargs)


def convNext(pretrained_name="ConvNeXt-T", pretrained=True, *args, **kwargs):
    factories = {"convnext-t": convnext_tiny, "convnext-s": convnext_small, "convnext-b": convnext_base,
                 "convnext-l": convnext_large, "convnext-xt": convnext_xlarge}
    return factories[pretrained_name.lower()](pretrained=pretrained, *args, **kwargs)
