"""ShuffleNetV2 backbone container for the FPN segmenters (reference models/semanticFCN.py:109-120,181-190 and
baselines/Reichert/semanticFCN_opt.py:155-166,227-236 build torchvision's `shufflenet_v2_x{0_5,1_0,1_5,2_0}`, replace `conv1[0]` by a 3x3 /
stride-1 conv over input + meta channels and wire `stem = conv1` (no maxpool), `layer1..3 = stage2..4`, `layer4 = conv5`).

torchvision is not needed: the classes below re-create the public architecture of torchvision's `shufflenetv2.py` -- module names, parameter
shapes and therefore `state_dict` keys, default initialisation -- without a module forward (the arithmetic lives in `unit_forward` / `encode`
below, on the HIP kernels); `pretrained` weights are not downloaded, load a checkpoint.

The unit (`InvertedResidual`):
  stride 1   out = shuffle(cat(x[:, :C/2], branch2(x[:, C/2:])))
  stride 2   out = shuffle(cat(branch1(x), branch2(x)))
  branch1    0 depthwise 3x3 / stride s, 1 BN, 2 1x1, 3 BN, 4 ReLU           (stride-2 units only; an empty Sequential otherwise)
  branch2    0 1x1, 1 BN, 2 ReLU, 3 depthwise 3x3 / stride s, 4 BN, 5 1x1, 6 BN, 7 ReLU
  shuffle    channel_shuffle(., 2): out channel 2 j = first half[j], 2 j + 1 = second half[j]
All convs are bias-free, BatchNorm eps is 1e-5."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from . import ops
from .encoder_family import EncoderFamily, run_stages
from .ops import ConvSource

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


# ----------------------------------------------------------------------------------------------------------------
def build(host, backbone, input_channels, meta_channel_dim):
    """The torchvision-shaped ShuffleNetV2 with the reference's surgery (semanticFCN.py:181-190): conv1[0] replaced by a 3x3 / stride-1 conv
    over input + meta channels, `stem` = conv1 (no maxpool), layer1..3 = stage2..4, layer4 = conv5.  Returns the channel ladder."""
    host.meta_channel_dim = meta_channel_dim
    host.backbone = ShuffleNetV2Container(backbone)
    host.backbone.conv1[0] = nn.Conv2d(input_channels + meta_channel_dim, host.backbone.conv1[0].out_channels, kernel_size=3, stride=1, padding=1,
                                       bias=False)
    host.stem = host.backbone.conv1
    host.layer1, host.layer2, host.layer3, host.layer4 = host.backbone.stage2, host.backbone.stage3, host.backbone.stage4, host.backbone.conv5
    return list(BASE_CHANNELS[backbone])


def folded_tail(host, name, dw: nn.Conv2d, dw_bn, pw: nn.Conv2d, pw_bn):
    """(wdw [C, 9], bdw [C], wpack, bpw [Co]) of a unit's depthwise 3x3 -> BN -> 1x1 -> BN -> ReLU tail with both BatchNorms folded in, cached on
    `host` per parameter version and conv precision (the pointwise product is the exact-fp32 MFMA under 'fp32' and 'f16x3' alike)."""
    def make():
        w9, b9 = host._fold(dw.weight, None, dw_bn)
        w1, b1 = host._fold(pw.weight, None, pw_bn)
        co, c = w1.shape[0], w1.shape[1]
        return (w9.detach().float().reshape(c, 9).contiguous(), b9.detach().float().contiguous(),
                ops.pack_shuffle_tail_weight(w1.detach().float().reshape(co, c).contiguous()), b1.detach().float().contiguous())
    return host._cached("_shf_cache", name, (dw.weight, dw_bn.weight, dw_bn.bias, dw_bn.running_mean, dw_bn.running_var,
                                             pw.weight, pw_bn.weight, pw_bn.bias, pw_bn.running_mean, pw_bn.running_var), make)


def unit_forward(host, n: str, blk, x, meta_k=None):
    """One InvertedResidual: the fused conv for branch2's first 1x1 (+ BN + ReLU), slu_shuffle_tail_fwd for the rest -- two launches for a
    stride-1 unit, three for a stride-2 one.  meta_k: the meta channels that replace the last m input channels (first unit of a stage)."""
    b2 = blk.branch2
    cx = x.shape[1]
    bf = b2[5].out_channels
    if blk.stride == 1:
        if meta_k is not None:
            raise NotImplementedError("meta injection into a stride-1 ShuffleNetV2 unit does not occur (every stage opens with a stride-2 unit)")
        h = host._conv(n + ".branch2.0", b2[0], b2[1], [ConvSource(x, None, False, 0, bf, cx - bf)])                  # x[:, C/2:]
        return ops.shuffle_tail(h, *folded_tail(host, n + ".branch2.3", b2[3], b2[4], b2[5], b2[6]), bf, 1, passthrough=x)
    m = 0 if meta_k is None else meta_k.shape[1]
    b1 = blk.branch1
    out = torch.empty((x.shape[0], 2 * bf, (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2), dtype=torch.float32, device=x.device)
    ops.shuffle_tail(x, *folded_tail(host, n + ".branch1.0", b1[0], b1[1], b1[2], b1[3]), bf, 2, out=out, parity=0, cuse=cx - m, src2=meta_k)
    src = [ConvSource(x)] if meta_k is None else [ConvSource(meta_k), ConvSource(x, None, False, 0, cx - m)]             # (meta, x[:, :-m])
    h = host._conv(n + ".branch2.0", b2[0], b2[1], src, tail_first=m)
    return ops.shuffle_tail(h, *folded_tail(host, n + ".branch2.3", b2[3], b2[4], b2[5], b2[6]), bf, 2, out=out, parity=1)


def encode(host, x, meta):
    """(x1, x2, x3, x4) at 1/2, 1/4, 1/8, 1/8 resolution: stem (conv + BN + ReLU, stride 1), stage2..4, conv5, with the multi-scale meta
    injection on the way into stage3 / stage4 / conv5 (semanticFCN.py:306-314)."""
    m1 = m2 = m3 = None
    if host.multi_scale_meta:
        m1, m2, m3 = ops.nearest_down(meta, 2), ops.nearest_down(meta, 4), ops.nearest_down(meta, 8)
    h = host._conv("stem", host.stem[0], host.stem[1], [ConvSource(x), ConvSource(meta)])
    x1, x2, x3 = run_stages(host, unit_forward, h, (("layer1", host.layer1, None), ("layer2", host.layer2, m1), ("layer3", host.layer3, m2)))
    m = 0 if m3 is None else m3.shape[1]
    src = [ConvSource(x3)] if m3 is None else [ConvSource(m3), ConvSource(x3, None, False, 0, x3.shape[1] - m)]
    x4 = host._conv("layer4", host.layer4[0], host.layer4[1], src, tail_first=m)
    return x1, x2, x3, x4


# no stride-2 depthwise backward, so no training; model.train() with every BatchNorm in eval mode is not refused (it never was)
FAMILY = EncoderFamily(backbones=tuple(BASE_CHANNELS), build=build, encode=encode, head_scales=(4, 4, 2),
                       inference_clause="the ShuffleNetV2 units have no backward kernels", training_refuses=False, trains_in_opt=False,
                       mc_shared_prefix=False)
