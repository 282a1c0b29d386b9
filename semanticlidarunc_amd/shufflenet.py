"""ShuffleNetV2 backbone container for the FPN segmenters (reference models/semanticFCN.py:109-120,181-190 and
baselines/Reichert/semanticFCN_opt.py:155-166,227-236 build torchvision's `shufflenet_v2_x{0_5,1_0,1_5,2_0}`, replace `conv1[0]` by a 3x3 /
stride-1 conv over input + meta channels and wire `stem = conv1` (no maxpool), `layer1..3 = stage2..4`, `layer4 = conv5`).

torchvision is not needed: the classes below re-create the public architecture of torchvision's `shufflenetv2.py` -- module names, parameter
shapes and therefore `state_dict` keys, default initialisation -- without a forward (the arithmetic lives in fpn.py on the HIP kernels);
`pretrained` weights are not downloaded, load a checkpoint.

The unit (`InvertedResidual`):
  stride 1   out = shuffle(cat(x[:, :C/2], branch2(x[:, C/2:])))
  stride 2   out = shuffle(cat(branch1(x), branch2(x)))
  branch1    0 depthwise 3x3 / stride s, 1 BN, 2 1x1, 3 BN, 4 ReLU           (stride-2 units only; an empty Sequential otherwise)
  branch2    0 1x1, 1 BN, 2 ReLU, 3 depthwise 3x3 / stride s, 4 BN, 5 1x1, 6 BN, 7 ReLU
  shuffle    channel_shuffle(., 2): out channel 2 j = first half[j], 2 j + 1 = second half[j]
All convs are bias-free, BatchNorm eps is 1e-5."""
from __future__ import annotations

from typing import List

import torch.nn as nn

# (stage repeats, [conv1, stage2, stage3, stage4, conv5] output channels) -- torchvision's shufflenet_v2_x* constructors
_CONFIGS = {
    "shufflenet_v2_x0_5": ([4, 8, 4], [24, 48, 96, 192, 1024]),
    "shufflenet_v2_x1_0": ([4, 8, 4], [24, 116, 232, 464, 1024]),
    "shufflenet_v2_x1_5": ([4, 8, 4], [24, 176, 352, 704, 1024]),
    "shufflenet_v2_x2_0": ([4, 8, 4], [24, 244, 488, 976, 2048]),
}
# channel ladder the reference hard-codes per backbone (semanticFCN.py:109-120): [x4, fpn4 out, fpn3 out, fpn2 out, fpn1 out]
BASE_CHANNELS = {"shufflenet_v2_x0_5": [1024, 192, 96, 48, 24], "shufflenet_v2_x1_0": [1024, 464, 232, 116, 24],
                 "shufflenet_v2_x1_5": [1024, 704, 352, 176, 24], "shufflenet_v2_x2_0": [2048, 976, 488, 244, 112]}
# torchvision's published parameter counts of the ImageNet classifiers
PARAMETER_COUNTS = {"shufflenet_v2_x0_5": 1366792, "shufflenet_v2_x1_0": 2278604, "shufflenet_v2_x1_5": 3503624, "shufflenet_v2_x2_0": 7393996}


def _dw(c: int, stride: int) -> nn.Conv2d:
    return nn.Conv2d(c, c, 3, stride, 1, bias=False, groups=c)


class InvertedResidual(nn.Module):
    def __init__(self, inp: int, oup: int, stride: int):
        super().__init__()
        if not 1 <= stride <= 3:
            raise ValueError("illegal stride value")
        self.stride = stride
        bf = oup // 2
        if stride == 1 and inp != bf << 1:
            raise ValueError(f"Invalid combination of stride {stride}, inp {inp} and oup {oup} values.")
        if stride > 1:
            self.branch1 = nn.Sequential(_dw(inp, stride), nn.BatchNorm2d(inp), nn.Conv2d(inp, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf),
                                         nn.ReLU(inplace=True))
        else:
            self.branch1 = nn.Sequential()
        self.branch2 = nn.Sequential(nn.Conv2d(inp if stride > 1 else bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True),
                                     _dw(bf, stride), nn.BatchNorm2d(bf), nn.Conv2d(bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf),
                                     nn.ReLU(inplace=True))


class ShuffleNetV2Container(nn.Module):
    """`conv1` / `maxpool` / `stage2..4` / `conv5` / `fc` of torchvision's ShuffleNetV2 (names, shapes and default initialisation only)."""

    def __init__(self, name: str, num_classes: int = 1000):
        super().__init__()
        repeats, chans = _CONFIGS[name]
        self._stage_out_channels: List[int] = list(chans)
        cin, cout = 3, chans[0]
        self.conv1 = nn.Sequential(nn.Conv2d(cin, cout, 3, 2, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        cin = cout
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for sname, rep, cout in zip(("stage2", "stage3", "stage4"), repeats, chans[1:4]):
            seq = [InvertedResidual(cin, cout, 2)] + [InvertedResidual(cout, cout, 1) for _ in range(rep - 1)]
            setattr(self, sname, nn.Sequential(*seq))
            cin = cout
        cout = chans[-1]
        self.conv5 = nn.Sequential(nn.Conv2d(cin, cout, 1, 1, 0, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.fc = nn.Linear(cout, num_classes)
