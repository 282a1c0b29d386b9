"""EfficientNetV2 backbone container for the FPN segmenters, and the inference forward of one block and of the encoder on the HIP kernels for both
of them (`block_forward`, `encode`; reference models/semanticFCN.py:124-135,192-201,296-304 wires the backbone exactly as `semanticFCN_opt`
does).  The container was written for the `semanticFCN_opt` segmenter (reference baselines/Reichert/semanticFCN_opt.py:170-180 builds
torchvision's `efficientnet_v2_{s,m,l}`, :238-247 replaces `features[0][0]` by a 3x3 / stride-1 conv over input + meta channels and wires
`stem = features[0]`, `layer1..3 = features[2..4]`, `layer4 = features[6:]`; its forward (:396-404) never calls layer4 nor features[1] / [5]).

torchvision is not needed: the classes below re-create the public architecture of torchvision 0.19's `efficientnet.py` -- module names,
parameter shapes and therefore `state_dict` keys -- without a module forward (the arithmetic lives in `block_forward` below and, for
`semanticFCN_opt`'s training path, in fpn_opt.py, on the HIP kernels); `pretrained`
weights are not downloaded, load a checkpoint.  **Parity of the block internals is unpinned** (no reference-held fixture): the
oracle (oracle/effnet.py) restates the same public definition, and the reference's OWN head / meta-injection wiring is pinned through it."""
from __future__ import annotations

import functools
import math
from typing import List, Tuple

import torch.nn as nn

from . import ops
from .encoder_family import EncoderFamily, run_stages
from .ops import ConvSource

# (block kind, expand ratio, kernel, stride, input channels, output channels, layers) -- torchvision's _efficientnet_conf for the V2 family
_CONFIGS = {
    "efficientnet_v2_s": ([("fused", 1, 3, 1, 24, 24, 2), ("fused", 4, 3, 2, 24, 48, 4), ("fused", 4, 3, 2, 48, 64, 4), ("mb", 4, 3, 2, 64, 128, 6),
                           ("mb", 6, 3, 1, 128, 160, 9), ("mb", 6, 3, 2, 160, 256, 15)], 1280, 0.2),
    "efficientnet_v2_m": ([("fused", 1, 3, 1, 24, 24, 3), ("fused", 4, 3, 2, 24, 48, 5), ("fused", 4, 3, 2, 48, 80, 5), ("mb", 4, 3, 2, 80, 160, 7),
                           ("mb", 6, 3, 1, 160, 176, 14), ("mb", 6, 3, 2, 176, 304, 18), ("mb", 6, 3, 1, 304, 512, 5)], 1280, 0.3),
    "efficientnet_v2_l": ([("fused", 1, 3, 1, 32, 32, 4), ("fused", 4, 3, 2, 32, 64, 7), ("fused", 4, 3, 2, 64, 96, 7), ("mb", 4, 3, 2, 96, 192, 10),
                           ("mb", 6, 3, 1, 192, 224, 19), ("mb", 6, 3, 2, 224, 384, 25), ("mb", 6, 3, 1, 384, 640, 7)], 1280, 0.4),
}
# channel ladder the reference hard-codes per backbone (semanticFCN_opt.py:170-180): [x4, fpn4 out, fpn3 out, fpn2 out, fpn1 out]
BASE_CHANNELS = {"efficientnet_v2_s": [128, 128, 64, 48, 168], "efficientnet_v2_m": [160, 160, 80, 48, 168], "efficientnet_v2_l": [192, 192, 96, 64, 168]}
BN_EPS = 1e-3      # torchvision builds the V2 family with norm_layer = partial(nn.BatchNorm2d, eps=1e-03)


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class Conv2dNormActivation(nn.Sequential):
    """conv (bias-free) -> BatchNorm2d(eps 1e-3) -> SiLU (children '0', '1', '2' as in torchvision.ops.misc)."""

    def __init__(self, cin: int, cout: int, kernel_size: int = 3, stride: int = 1, groups: int = 1, act: bool = True):
        layers: List[nn.Module] = [nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False),
                                   nn.BatchNorm2d(cout, eps=BN_EPS)]
        if act:
            layers.append(nn.SiLU(inplace=True))
        super().__init__(*layers)
        self.out_channels = cout


class SqueezeExcitation(nn.Module):
    def __init__(self, channels: int, squeeze: int):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)
        self.activation = nn.SiLU(inplace=True)
        self.scale_activation = nn.Sigmoid()


class StochasticDepth(nn.Module):
    def __init__(self, p: float, mode: str = "row"):
        super().__init__()
        self.p, self.mode = p, mode


class FusedMBConv(nn.Module):
    def __init__(self, expand, kernel, stride, cin, cout, sd_prob):
        super().__init__()
        self.use_res_connect = stride == 1 and cin == cout
        expanded = _make_divisible(cin * expand)
        if expanded != cin:
            layers = [Conv2dNormActivation(cin, expanded, kernel, stride), Conv2dNormActivation(expanded, cout, 1, act=False)]
        else:
            layers = [Conv2dNormActivation(cin, cout, kernel, stride)]
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob)
        self.out_channels, self.stride = cout, stride


class MBConv(nn.Module):
    def __init__(self, expand, kernel, stride, cin, cout, sd_prob):
        super().__init__()
        self.use_res_connect = stride == 1 and cin == cout
        expanded = _make_divisible(cin * expand)
        layers: List[nn.Module] = []
        if expanded != cin:
            layers.append(Conv2dNormActivation(cin, expanded, 1))
        layers.append(Conv2dNormActivation(expanded, expanded, kernel, stride, groups=expanded))
        layers.append(SqueezeExcitation(expanded, max(1, cin // 4)))
        layers.append(Conv2dNormActivation(expanded, cout, 1, act=False))
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob)
        self.out_channels, self.stride = cout, stride


class EfficientNetContainer(nn.Module):
    """`features` / `avgpool` / `classifier` of torchvision's EfficientNet for the V2 configurations (names and shapes only)."""

    def __init__(self, name: str, num_classes: int = 1000, stochastic_depth_prob: float = 0.2):
        super().__init__()
        conf, last_channel, dropout = _CONFIGS[name]
        layers: List[nn.Module] = [Conv2dNormActivation(3, conf[0][4], 3, 2)]
        total = float(sum(c[6] for c in conf))
        bid = 0
        for kind, expand, kernel, stride, cin, cout, n in conf:
            stage = []
            for k in range(n):
                blk = FusedMBConv if kind == "fused" else MBConv
                stage.append(blk(expand, kernel, stride if k == 0 else 1, cin if k == 0 else cout, cout, stochastic_depth_prob * bid / total))
                bid += 1
            layers.append(nn.Sequential(*stage))
        layers.append(Conv2dNormActivation(conf[-1][5], last_channel, 1))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout, inplace=True), nn.Linear(last_channel, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                r = 1.0 / math.sqrt(m.out_features)
                nn.init.uniform_(m.weight, -r, r)
                nn.init.zeros_(m.bias)


def stage_channels(name: str) -> Tuple[int, int, int, int]:
    """(stem, features[2], features[3], features[4]) output channels."""
    conf = _CONFIGS[name][0]
    return conf[0][4], conf[1][5], conf[2][5], conf[3][5]


# ----------------------------------------------------------------------------------------------------------------
def build(host, backbone, input_channels, meta_channel_dim):
    """The torchvision-shaped efficientnet_v2_{s,m,l} with the reference's surgery (semanticFCN.py:192-201): features[0][0] replaced by a 3x3 /
    stride-1 conv over input + meta channels, `stem` = features[0], layer1..3 = features[2..4], layer4 = features[6:] (a slice, which keeps the
    children's names: built, aliased in the state_dict as layer4.6.* / layer4.7.* as in the reference, never called by forward).  Returns the channel ladder."""
    host.meta_channel_dim = meta_channel_dim
    host.backbone = EfficientNetContainer(backbone)
    f = host.backbone.features
    f[0][0] = nn.Conv2d(input_channels + meta_channel_dim, f[0][0].out_channels, kernel_size=3, stride=1, padding=1, bias=False)
    host.stem, host.layer1, host.layer2, host.layer3, host.layer4 = f[0], f[2], f[3], f[4], f[6:]
    return list(BASE_CHANNELS[backbone])


def _cna(host, name, cna, srcs, resid=None, tail_first=0):
    """Conv2dNormActivation with a dense stride-1 conv: conv -> folded BatchNorm -> SiLU (or none) [+ resid] as one fused conv launch."""
    return host._conv(name, cna[0], cna[1], srcs, act="silu" if len(cna) > 2 else "none", resid=resid, tail_first=tail_first)


def folded_depthwise(host, name, cna):
    """(w [C, 9], bias [C]) of a depthwise Conv2dNormActivation with the eval BatchNorm folded in, cached on `host` per parameter version (exact
    fp32 under every conv precision, so the precision is not part of the key's meaning -- it is kept in it as in the packed-conv cache)."""
    conv, bn = cna[0], cna[1]

    def make():
        w, b = host._fold(conv.weight, None, bn)
        return w.detach().float().reshape(w.shape[0], 9).contiguous(), b.detach().float().contiguous()
    return host._cached("_dw_cache", name, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), make)


def block_forward(host, name: str, blk, x, meta_k=None, fused_se: bool = True):
    """One FusedMBConv / MBConv block, eval mode (StochasticDepth = identity), on the HIP kernels.  `host` is the FPN model: its `_conv` /
    `_conv_s2` run the fused convs with their folded BatchNorm from its packed-weight cache.  meta_k: the meta channels, at the block's input
    resolution, that replace the last m channels of x on the way in (first block of layer2 / layer3).  fused_se=False: the composed MBConv
    middle -- slu_dwconv3x3_fwd, then slu_global_avgpool + slu_se_gate (ops.se_scale), three launches, the mean rounded from an fp64 sum --
    which is what `semanticFCN_opt` launches.

      FusedMBConv   3x3 expansion (+ BN + SiLU): the fused conv; at stride 2 the 2x2 conv over space_to_depth2(_cat) of the input; then the 1x1
                    projection (+ BN) with the identity added where the block has one
      MBConv        expand   fused 1x1 conv (+ BN + SiLU); with meta_k it reads (meta_k, x[:, :-m]) in place, the weight's input channels rotated
                    dw       slu_dwconv3x3_se_fwd: depthwise 3x3 / stride + BN + SiLU + the per-tile sums of the SE's mean, one launch
                    gate     slu_se_gate_psum: tile sums -> mean -> fc1 -> SiLU -> fc2 -> sigmoid, one launch
                    project  fused 1x1 conv (+ BN) with the gate as the per-(sample, channel) input multiplier, + identity
                    -- four launches; the expanded map is written once and read once."""
    seq = blk.block
    cx = x.shape[1]
    m = 0 if meta_k is None else meta_k.shape[1]
    resid = x if blk.use_res_connect else None
    src = [ConvSource(x)] if meta_k is None else [ConvSource(meta_k), ConvSource(x, None, False, 0, cx - m)]      # (meta, x[:, :-m])
    if isinstance(blk, FusedMBConv):
        first = seq[0]
        if first[0].stride[0] == 2:
            s2d = ops.space_to_depth2(x) if meta_k is None else ops.space_to_depth2_cat(x, cx - m, meta_k)
            h = host._conv_s2(name + ".0", first[0], first[1], s2d, cx, act="silu" if len(first) > 2 else "none")
        else:
            h = _cna(host, name + ".0", first, src, resid=resid if len(seq) == 1 else None, tail_first=m)
        return h if len(seq) == 1 else _cna(host, name + ".1", seq[1], [ConvSource(h)], resid=resid)
    i, h = 0, x
    if len(seq) == 4:                                               # 1x1 expansion
        h, i = _cna(host, name + ".0", seq[0], src, tail_first=m), 1
    elif meta_k is not None:
        raise NotImplementedError("meta injection into an MBConv without expansion does not occur in the V2 configurations")
    dw, se, proj = seq[i], seq[i + 1], seq[i + 2]
    w9, b9 = folded_depthwise(host, f"{name}.{i}", dw)
    c, s = se.fc1.in_channels, se.fc1.out_channels
    fc = (se.fc1.weight.detach().reshape(s, c), se.fc1.bias.detach(), se.fc2.weight.detach().reshape(c, s), se.fc2.bias.detach())
    if fused_se:
        h, psum = ops.dwconv3x3_se(h, w9, b9, dw[0].stride[0])
        gate = ops.se_gate_psum(psum, h.shape[2] * h.shape[3], *fc)
    else:
        h = ops.dwconv3x3(h, w9, b9, dw[0].stride[0], "silu")
        gate = ops.se_scale(h, *fc)
    return _cna(host, f"{name}.{i + 2}", proj, [ConvSource(h, gate)], resid=resid)      # the SE multiplies the projection's input


def encode(host, x, meta):
    """(x1, x2, x3, x4) at 1/2, 1/4, 1/8, 1/8 resolution: stem (conv + BN + SiLU, stride 1), features[2..4], the meta channels injected on the
    way into layer2 and layer3; x4 = cat(x3[:, :-m], meta3) -- layer4 is never applied (semanticFCN.py:296-304).  The MBConv middle is the
    host class's `mbconv_fused_se`."""
    if not host.multi_scale_meta:
        raise NotImplementedError("efficientnet backbones run with multi_scale_meta=True only (the reference's other branch feeds layer4 = "
                                  "features[6:] a tensor of the wrong channel count)")
    m1, m2, m3 = ops.nearest_down(meta, 2), ops.nearest_down(meta, 4), ops.nearest_down(meta, 8)
    h = host._conv("stem", host.stem[0], host.stem[1], [ConvSource(x), ConvSource(meta)], act="silu")
    block = functools.partial(block_forward, fused_se=host.mbconv_fused_se)
    x1, x2, x3 = run_stages(host, block, h, (("layer1", host.layer1, None), ("layer2", host.layer2, m1), ("layer3", host.layer3, m2)))
    return x1, x2, x3, ops.replace_tail(x3, m3)


# `models.semanticFCN` has no backward for the fused depthwise + gate kernels; `semanticFCN_opt` trains through its own autograd nodes
FAMILY = EncoderFamily(backbones=tuple(BASE_CHANNELS), build=build, encode=encode, head_scales=(4, 4, 2),
                       inference_clause="the fused depthwise + SE kernels of the MBConv block have no backward", training_refuses=True,
                       trains_in_opt=True, mc_shared_prefix=True)
