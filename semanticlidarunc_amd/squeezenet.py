"""SqueezeNet 1.0 backbone container for the FPN segmenters (reference models/semanticFCN.py:121-123,155-169 and
baselines/Reichert/semanticFCN_opt.py:167-169,201-215 build torchvision's `squeezenet1_0`, replace `features[0]` by a 3x3 / stride-1 conv over
2 + meta channels and wire `stem = features[0:4]`, `layer1 = features[4:6]`, `layer2 = features[6:8]`, `layer3 = features[8:10]`,
`layer4 = features[10:]`).

torchvision is not needed: the classes below re-create the public architecture of torchvision's `squeezenet.py` -- module names, parameter
shapes and therefore `state_dict` keys (including `classifier.1.*`), default initialisation -- without a module forward (the arithmetic lives in
`run_modules` / `encode` below, on the HIP kernels); `pretrained` weights are not downloaded, load a checkpoint.

  features   0 conv 7x7 / stride 2 (replaced), 1 ReLU, 2 MaxPool(3, 2, ceil), 3 Fire(96, 16, 64, 64), 4 Fire(128, 16, 64, 64),
             5 Fire(128, 32, 128, 128), 6 MaxPool, 7 Fire(256, 32, 128, 128), 8 Fire(256, 48, 192, 192), 9 Fire(384, 48, 192, 192),
             10 Fire(384, 64, 256, 256), 11 MaxPool, 12 Fire(512, 64, 256, 256)
  Fire       out = cat(relu(expand1x1(s)), relu(expand3x3(s))), s = relu(squeeze(x)); every conv has a bias, there is no BatchNorm
  classifier 0 Dropout, 1 conv 1x1 512 -> classes, 2 ReLU, 3 AdaptiveAvgPool (never called by the segmenters)"""
from __future__ import annotations

import torch.nn as nn
import torch.nn.init as init

from . import ops
from .encoder_family import EncoderFamily
from .ops import ConvSource

# (in, squeeze, expand 1x1, expand 3x3) of the eight Fires, 'M' = MaxPool2d(3, 2, ceil_mode=True) -- torchvision's version "1_0"
_FEATURES = [(96, 16, 64, 64), (128, 16, 64, 64), (128, 32, 128, 128), "M", (256, 32, 128, 128), (256, 48, 192, 192), (384, 48, 192, 192),
             (384, 64, 256, 256), "M", (512, 64, 256, 256)]
# channel ladder the reference hard-codes (semanticFCN.py:123): [x4, fpn4 out, fpn3 out, fpn2 out, fpn1 out]
BASE_CHANNELS = {"squeezenet1_0": [512, 384, 256, 256, 112]}
# torchvision's published parameter count of the ImageNet classifier
PARAMETER_COUNTS = {"squeezenet1_0": 1248424}


class Fire(nn.Module):
    def __init__(self, inplanes: int, squeeze_planes: int, expand1x1_planes: int, expand3x3_planes: int):
        super().__init__()
        self.inplanes = inplanes
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, kernel_size=1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, kernel_size=1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, kernel_size=3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)


class SqueezeNetContainer(nn.Module):
    """`features` / `classifier` of torchvision's SqueezeNet 1.0 (names, shapes and default initialisation only)."""

    def __init__(self, name: str = "squeezenet1_0", num_classes: int = 1000, dropout: float = 0.5):
        super().__init__()
        if name not in BASE_CHANNELS:
            raise ValueError(f"Unsupported SqueezeNet version {name}: squeezenet1_0 expected")
        self.num_classes = num_classes
        seq = [nn.Conv2d(3, 96, kernel_size=7, stride=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True)]
        for f in _FEATURES:
            seq.append(nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True) if f == "M" else Fire(*f))
        self.features = nn.Sequential(*seq)
        final_conv = nn.Conv2d(512, num_classes, kernel_size=1)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout), final_conv, nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1)))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                if m is final_conv:
                    init.normal_(m.weight, mean=0.0, std=0.01)
                else:
                    init.kaiming_uniform_(m.weight)
                if m.bias is not None:
                    init.constant_(m.bias, 0)


# ----------------------------------------------------------------------------------------------------------------
def build(host, backbone, input_channels, meta_channel_dim):
    """The torchvision-shaped SqueezeNet 1.0 with the reference's surgery (semanticFCN.py:155-169): features[0] replaced by a 3x3 / stride-1
    conv over 2 + meta channels (the reference hard-codes the 2), `stem` = features[0:4], layer1..4 = features[4:6] / [6:8] / [8:10] / [10:].
    Returns the channel ladder."""
    host.meta_channel_dim = meta_channel_dim
    host.backbone = SqueezeNetContainer(backbone)
    f = host.backbone.features
    f[0] = nn.Conv2d(2 + meta_channel_dim, 96, kernel_size=3, stride=1, padding=1, bias=False)
    host.stem, host.layer1, host.layer2, host.layer3, host.layer4 = f[0:4], f[4:6], f[6:8], f[8:10], f[10:]
    return list(BASE_CHANNELS[backbone])


def fire_params(host, name, fire):
    """(wpack, bsq, b1, b3) of a Fire module, cached on `host` per parameter version and conv precision (every product is the exact-fp32 MFMA
    under 'fp32' and 'f16x3' alike)."""
    sq, e1, e3 = fire.squeeze, fire.expand1x1, fire.expand3x3

    def f(t):
        return t.detach().float().contiguous()

    def make():
        wpack = ops.pack_fire_weight(f(sq.weight).reshape(sq.out_channels, sq.in_channels), f(e1.weight).reshape(e1.out_channels, e1.in_channels),
                                     f(e3.weight))
        return wpack, f(sq.bias), f(e1.bias), f(e3.bias)
    return host._cached("_fire_cache", name, (sq.weight, sq.bias, e1.weight, e1.bias, e3.weight, e3.bias), make)


def run_modules(host, lname, modules, x, meta_k):
    """A run of `features`: Fire = one slu_fire_fwd, MaxPool = slu_maxpool3s2_ceil_fwd.  meta_k: the meta channels that replace the last m
    channels of x on the way into the first module (read in place as a second source)."""
    for i, mod in enumerate(modules):
        kw = {}
        if i == 0 and meta_k is not None:
            kw = dict(cuse=x.shape[1] - meta_k.shape[1], src2=meta_k)
        if isinstance(mod, Fire):
            x = ops.fire(x, *fire_params(host, f"{lname}.{i}", mod), **kw)
        elif isinstance(mod, nn.MaxPool2d):
            x = ops.maxpool3s2_ceil(x, **kw)
        else:
            raise NotImplementedError(f"{type(mod).__name__} inside a SqueezeNet stage is not on the HIP path")
    return x


def encode(host, x, meta):
    """(x1, x2, x3, x4) with 256 / 256 / 384 / 512 channels at 1/2, 1/4, 1/4, 1/8 resolution; the meta channels go into layer2 (ahead of its
    pool) and layer3 only, meta3 is unused (semanticFCN.py:287-295)."""
    m1 = m2 = None
    if host.multi_scale_meta:
        m1, m2 = ops.nearest_down(meta, 2), ops.nearest_down(meta, 4)
    h = host._conv("stem", host.stem[0], None, [ConvSource(x), ConvSource(meta)])
    xs = run_modules(host, "stem", list(host.stem)[2:], h, None)
    x1 = run_modules(host, "layer1", host.layer1, xs, None)
    x2 = run_modules(host, "layer2", host.layer2, x1, m1)
    x3 = run_modules(host, "layer3", host.layer3, x2, m2)
    x4 = run_modules(host, "layer4", host.layer4, x3, None)
    return x1, x2, x3, x4


# the Fire kernel and the ceil pool have no backward, so no training
FAMILY = EncoderFamily(backbones=tuple(BASE_CHANNELS), build=build, encode=encode, head_scales=(4, 2, 2),
                       inference_clause="the Fire module kernel has no backward", training_refuses=True, trains_in_opt=False, mc_shared_prefix=False)
