"""SqueezeNet 1.0 backbone container for the FPN segmenters (reference models/semanticFCN.py:121-123,155-169 and
baselines/Reichert/semanticFCN_opt.py:167-169,201-215 build torchvision's `squeezenet1_0`, replace `features[0]` by a 3x3 / stride-1 conv over
2 + meta channels and wire `stem = features[0:4]`, `layer1 = features[4:6]`, `layer2 = features[6:8]`, `layer3 = features[8:10]`,
`layer4 = features[10:]`).

torchvision is not needed: the classes below re-create the public architecture of torchvision's `squeezenet.py` -- module names, parameter
shapes and therefore `state_dict` keys (including `classifier.1.*`), default initialisation -- without a forward (the arithmetic lives in fpn.py
on the HIP kernels); `pretrained` weights are not downloaded, load a checkpoint.

  features   0 conv 7x7 / stride 2 (replaced), 1 ReLU, 2 MaxPool(3, 2, ceil), 3 Fire(96, 16, 64, 64), 4 Fire(128, 16, 64, 64),
             5 Fire(128, 32, 128, 128), 6 MaxPool, 7 Fire(256, 32, 128, 128), 8 Fire(256, 48, 192, 192), 9 Fire(384, 48, 192, 192),
             10 Fire(384, 64, 256, 256), 11 MaxPool, 12 Fire(512, 64, 256, 256)
  Fire       out = cat(relu(expand1x1(s)), relu(expand3x3(s))), s = relu(squeeze(x)); every conv has a bias, there is no BatchNorm
  classifier 0 Dropout, 1 conv 1x1 512 -> classes, 2 ReLU, 3 AdaptiveAvgPool (never called by the segmenters)"""
from __future__ import annotations

import torch.nn as nn
import torch.nn.init as init

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
