"""RegNetY backbone container for the FPN segmenters, and the forward of one Y block on the HIP kernels (reference
models/semanticFCN.py:97-108,171-179 and baselines/Reichert/semanticFCN_opt.py:143-154 build torchvision's `regnet_y_{400mf,800mf,1_6gf,3_2gf}`,
replace `stem[0]` by a 3x3 / stride-1 conv over input + meta channels and wire `stem = stem`, `layer1..4 = trunk_output[0..3]`).

torchvision is not needed: the classes below re-create the public architecture of torchvision's `regnet.py` -- module names, parameter shapes
and therefore `state_dict` keys (including `fc.*`), default initialisation -- without a forward; `pretrained` weights are not downloaded, load
a checkpoint.

  stem          0 conv 3x3 / stride 2 (replaced), 1 BN, 2 ReLU
  trunk_output  block1 .. block4, each a Sequential of Y blocks named block{i}-{j}; the first block of every stage has stride 2
  Y block       out = relu((proj(x) or x) + f(x));  proj = 1x1 / stride conv + BN where the width or the stride changes
  f             a: 1x1 + BN + ReLU;  b: grouped 3x3 / stride, groups = width / group width, + BN + ReLU;
                se: b * sigmoid(fc2(relu(fc1(mean_HW(b))))), fc1: width -> round(0.25 * block input width), both with bias;  c: 1x1 + BN
  avgpool, fc   never called by the segmenters
Convs other than the SE's are bias-free, BatchNorm eps is 1e-5.

`y_block_forward` is the one forward of a block; both FPN classes reach it through `encode` below."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch.nn as nn

from . import ops
from .encoder_family import EncoderFamily, run_stages
from .ops import ConvSource

# (depth, w_0, w_a, w_m, group width) -- torchvision's regnet_y_* constructors; se_ratio 0.25, bottleneck multiplier 1
_PARAMS = {"regnet_y_400mf": (16, 48, 27.89, 2.09, 8), "regnet_y_800mf": (14, 56, 38.84, 2.4, 16),
           "regnet_y_1_6gf": (27, 48, 20.71, 2.65, 24), "regnet_y_3_2gf": (21, 80, 42.63, 2.66, 24)}
# channel ladder the reference hard-codes per backbone (semanticFCN.py:97-108): [x4, fpn4 out, fpn3 out, fpn2 out, fpn1 out]
BASE_CHANNELS = {"regnet_y_400mf": [440, 208, 104, 48, 32], "regnet_y_800mf": [784, 320, 144, 64, 32],
                 "regnet_y_1_6gf": [888, 336, 120, 48, 32], "regnet_y_3_2gf": [1512, 576, 216, 72, 32]}
# torchvision's published parameter counts of the ImageNet classifiers
PARAMETER_COUNTS = {"regnet_y_400mf": 4344144, "regnet_y_800mf": 6432512, "regnet_y_1_6gf": 11202430, "regnet_y_3_2gf": 19436338}
GROUP_WIDTH = {k: v[4] for k, v in _PARAMS.items()}
STAGE_DEPTHS = {"regnet_y_400mf": [1, 3, 6, 6], "regnet_y_800mf": [1, 3, 8, 2], "regnet_y_1_6gf": [2, 6, 17, 2], "regnet_y_3_2gf": [2, 5, 13, 1]}
# what the FPN classes accept: the two small models stay refused by name until the four tests that use them as the "still unimplemented"
# sentinel move on; container, kernel and block forward cover all four
ENABLED = ("regnet_y_1_6gf", "regnet_y_3_2gf")
STEM_WIDTH = 32
SE_RATIO = 0.25


def stage_widths_and_depths(name: str):
    """torchvision's BlockParams.from_init_params: block widths on a quantised log scale, a stage = a run of equal widths, every width made
    divisible by min(group width, width)."""
    depth, w_0, w_a, w_m, gw = _PARAMS[name]
    widths = []
    for i in range(depth):
        cap = round(math.log((i * w_a + w_0) / w_0) / math.log(w_m))
        widths.append(int(round(w_0 * w_m ** cap / 8) * 8))
    stages, depths = [], []
    for w in widths:
        if stages and stages[-1] == w:
            depths[-1] += 1
        else:
            stages.append(w)
            depths.append(1)
    out = []
    for w in stages:
        g = min(gw, w)
        v = max(g, int(w + g / 2) // g * g)      # torchvision's _make_divisible
        out.append(v + g if v < 0.9 * w else v)
    return out, depths


def _cna(cin, cout, k, stride, groups, act):
    mods = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]
    if act:
        mods.append(nn.ReLU(inplace=True))
    return nn.Sequential(*mods)


class SqueezeExcitation(nn.Module):
    def __init__(self, input_channels: int, squeeze_channels: int):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Sigmoid()


class YBlock(nn.Module):
    """torchvision's ResBottleneckBlock (bottleneck multiplier 1) with its BottleneckTransform `f`."""

    def __init__(self, width_in: int, width_out: int, stride: int, group_width: int, se_ratio: float = SE_RATIO):
        super().__init__()
        self.proj = None
        if width_in != width_out or stride != 1:
            self.proj = _cna(width_in, width_out, 1, stride, 1, False)
        layers = OrderedDict()
        layers["a"] = _cna(width_in, width_out, 1, 1, 1, True)
        layers["b"] = _cna(width_out, width_out, 3, stride, width_out // group_width, True)
        layers["se"] = SqueezeExcitation(width_out, int(round(se_ratio * width_in)))
        layers["c"] = _cna(width_out, width_out, 1, 1, 1, False)
        self.f = nn.Sequential(layers)
        self.activation = nn.ReLU(inplace=True)
        self.stride, self.group_width = stride, group_width


class RegNetYContainer(nn.Module):
    """`stem` / `trunk_output` / `avgpool` / `fc` of torchvision's RegNetY (names, shapes and default initialisation only)."""

    def __init__(self, name: str, num_classes: int = 1000):
        super().__init__()
        if name not in _PARAMS:
            raise ValueError(f"Unsupported RegNetY version {name}: one of {sorted(_PARAMS)} expected")
        widths, depths = stage_widths_and_depths(name)
        gw = GROUP_WIDTH[name]
        self.stem = _cna(3, STEM_WIDTH, 3, 2, 1, True)
        cur = STEM_WIDTH
        stages = []
        for i, (w, d) in enumerate(zip(widths, depths)):
            blocks = OrderedDict()
            for j in range(d):
                blocks[f"block{i + 1}-{j}"] = YBlock(cur if j == 0 else w, w, 2 if j == 0 else 1, gw)
            stages.append((f"block{i + 1}", nn.Sequential(blocks)))
            cur = w
        self.trunk_output = nn.Sequential(OrderedDict(stages))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cur, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                nn.init.normal_(m.weight, mean=0.0, std=math.sqrt(2.0 / fan_out))
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0.0, std=0.01)
                nn.init.zeros_(m.bias)


# ----------------------------------------------------------------------------------------------------------------
def build(host, backbone, input_channels, meta_channel_dim):
    """The torchvision-shaped RegNetY with the reference's surgery (semanticFCN.py:171-179): stem[0] replaced by a 3x3 / stride-1 conv over
    input + meta channels, `stem` = stem (conv + BN + ReLU), layer1..4 = trunk_output[0..3].  Returns the channel ladder."""
    host.meta_channel_dim = meta_channel_dim
    host.backbone = RegNetYContainer(backbone)
    host.backbone.stem[0] = nn.Conv2d(input_channels + meta_channel_dim, host.backbone.stem[0].out_channels, kernel_size=3, stride=1, padding=1,
                                      bias=False)
    host.stem = host.backbone.stem
    t = host.backbone.trunk_output
    host.layer1, host.layer2, host.layer3, host.layer4 = t[0], t[1], t[2], t[3]
    return list(BASE_CHANNELS[backbone])


def folded_gconv(host, name, conv: nn.Conv2d, bn):
    """(wg, bias) of a Y block's grouped 3x3 conv with its BatchNorm folded in, in the order slu_regnet_gconv_fwd reads, cached on `host` per
    parameter version and conv precision (the products are exact fp32 under 'fp32' and 'f16x3' alike)."""
    def make():
        w, b = host._fold(conv.weight, None, bn)
        return ops.pack_regnet_gconv_weight(w.detach().float().contiguous(), conv.in_channels // conv.groups), b.detach().float().contiguous()
    return host._cached("_regnet_cache", name, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), make)


def y_block_forward(host, name: str, blk: YBlock, x, meta_k=None):
    """One Y block, eval mode, on the HIP kernels.  `host` is the FPN model: its `_conv` runs the fused 1x1 convs with their folded BatchNorm
    from its packed-weight cache, `folded_gconv` keeps the folded, re-ordered f.b weights on it.  meta_k: the meta channels, at the block's input
    resolution, that replace the last m channels of x on the way in (first block of layer2..4).

      f.a     fused 1x1 conv (+ BN + ReLU); with meta_k it reads (meta_k, x[:, :-m]) in place, the weight's input channels rotated
      f.b     slu_regnet_gconv_fwd: grouped 3x3 / stride + BN + ReLU + the per-tile sums of the SE's mean, one launch
      gate    slu_regnet_se_gate: tile sums -> mean -> fc1 -> ReLU -> fc2 -> sigmoid, one launch
      proj    stride 2: slu_regnet_sample2 writes cat(x[:, :-m], meta_k)[::2, ::2] (a quarter of the input read, a quarter written), then the
              fused 1x1 conv (+ BN); stride 1 with a width change: the fused 1x1 conv on the sources of f.a
      f.c     fused 1x1 conv (+ BN) with the gate as the per-(sample, channel) input multiplier, + identity, ReLU after the sum"""
    cx = x.shape[1]
    m = 0 if meta_k is None else meta_k.shape[1]
    f = blk.f
    src = [ConvSource(x)] if meta_k is None else [ConvSource(meta_k), ConvSource(x, None, False, 0, cx - m)]      # (meta, x[:, :-m])
    a = host._conv(name + ".f.a", f.a[0], f.a[1], src, tail_first=m)
    stride = f.b[0].stride[0]
    wg, bg = folded_gconv(host, name + ".f.b", f.b[0], f.b[1])
    h, psum = ops.regnet_gconv(a, wg, bg, stride)
    se = f.se
    c, s = se.fc1.in_channels, se.fc1.out_channels
    gate = ops.regnet_se_gate(psum, h.shape[2] * h.shape[3], se.fc1.weight.detach().reshape(s, c), se.fc1.bias.detach(),
                              se.fc2.weight.detach().reshape(c, s), se.fc2.bias.detach())
    if blk.proj is None:
        if meta_k is not None:
            raise NotImplementedError("meta injection into a Y block without a projection does not occur (every stage opens with a stride-2 block)")
        idn = x
    elif blk.proj[0].stride[0] == 2:
        xs = ops.regnet_sample2(x, 0, cx - m, meta_k)
        idn = host._conv(name + ".proj", blk.proj[0], blk.proj[1], [ConvSource(xs)], act="none")
    else:
        idn = host._conv(name + ".proj", blk.proj[0], blk.proj[1], src, act="none", tail_first=m)
    return host._conv(name + ".f.c", f.c[0], f.c[1], [ConvSource(h, gate)], act="relu", resid=idn, late=True)


def encode(host, x, meta):
    """(x1, x2, x3, x4) at 1/2, 1/4, 1/8, 1/16 resolution: stem (conv + BN + ReLU, stride 1), the four stages of Y blocks, with the multi-scale
    meta injection on the way into layer2 / layer3 / layer4 (semanticFCN.py:305-314)."""
    m1 = m2 = m3 = None
    if host.multi_scale_meta:
        m1, m2, m3 = ops.nearest_down(meta, 2), ops.nearest_down(meta, 4), ops.nearest_down(meta, 8)
    h = host._conv("stem", host.stem[0], host.stem[1], [ConvSource(x), ConvSource(meta)])
    return tuple(run_stages(host, y_block_forward, h, (("layer1", host.layer1, None), ("layer2", host.layer2, m1), ("layer3", host.layer3, m2),
                                                       ("layer4", host.layer4, m3))))


# the grouped conv and the gate have no backward, so no training; the default head
FAMILY = EncoderFamily(backbones=ENABLED, build=build, encode=encode, head_scales=(8, 4, 2),
                       inference_clause="the grouped conv kernel of the Y block has no backward", training_refuses=True, trains_in_opt=False,
                       mc_shared_prefix=False)
