"""CENet's ResNet-34 range-image segmenter on MI355X, inference only: the reference's `CENet(model="ResNet_34")` / `ResNet_34` contract
(src/baselines/CENet/CENet.py:7-26, CENet_ResNet34.py:91-198) over the fused HIP conv and two decoder kernels (csrc/cenet_ops.hip).

Contract kept: constructor arguments, module names, parameter shapes and default initialisation (the `state_dict` is the reference's, key for
key), `forward(x[B, input_dim, H, W])` -> class probabilities `[B, nclasses, H, W]`, or `[out, res_2, res_3, res_4]` with `aux=True`.  The
containers below hold parameters only; there is no torch module forward (the style of shufflenet.py).  The HarDNet variant and training are not
provided: the reference's CENet trainer imports a class that does not exist (CENet/trainer.py:18), so there is no training run to reproduce.

How the layers map onto kernels (eval BatchNorm folded into the preceding conv's weights and bias, as in fpn.py whose weight preparation and
cache -- per parameter version and conv precision -- this model uses):
  BasicConv2d, BasicBlock conv1 ... conv + BN + LeakyReLU(0.01): one fused conv launch
  BasicBlock tail ................. conv + BN + identity, LeakyReLU after the residual add (late activation)
  stage entry (stride 2) .......... space-to-depth + the 2x2 stride-1 conv with re-indexed weights; the 1x1 / stride-2 downsample conv reads
                                    phase (0, 0) of the same tensor
  res_2 / res_3 / res_4 ........... ONE slu_bilinear_ac_cat launch into a [B, 384, H, W] buffer; conv_1 reads (x, x_1, that buffer) as its
                                    three sources, so the 640-channel torch.cat is never written
  semantic_output + softmax ....... 1x1 conv, then slu_bilinear_ac_softmax at equal sizes
  aux_head_k + softmax ............ the 1x1 conv on the LOW-resolution x_k, then slu_bilinear_ac_softmax: a 1x1 conv commutes with the
                                    interpolation (its four weights sum to 1), so the full-resolution 128 -> C convs are not run; equal to the
                                    reference order up to rounding
Conv precision "fp32" and "f16x3" run; "f16" (half-precision storage) is refused."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from . import fpn as _fpn
from . import ops
from . import salsanext as _sn
from .ops import ConvSource

SLOPE = 0.01      # nn.LeakyReLU()'s default negative slope


# ----------------------------------------------------------------------------------------------------------------
# containers (names, shapes and construction order of CENet_ResNet34.py: the default initialisation draws the reference's random numbers)
# ----------------------------------------------------------------------------------------------------------------
def conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False, dilation=dilation)


def conv1x1(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class _NoTorchForward(nn.Module):
    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} is a parameter container: the forward pass is ResNet_34's (semanticlidarunc_amd/cenet.py)")


class BasicConv2d(_NoTorchForward):
    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, dilation=1, relu=True):
        super().__init__()
        self.relu = relu
        self.conv = nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, bias=False)
        self.bn = nn.BatchNorm2d(out_planes)
        if self.relu:
            self.relu = nn.LeakyReLU()


class BasicBlock(_NoTorchForward):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, if_BN=None):
        super().__init__()
        if not if_BN:
            raise NotImplementedError("BasicBlock without BatchNorm (if_BN=False) is not implemented on the HIP path")
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        self.if_BN = if_BN
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.LeakyReLU()
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


class ResNet_34(nn.Module):
    def __init__(self, nclasses, input_dim=5, aux=False, block=BasicBlock, layers=[3, 4, 6, 3], if_BN=True, zero_init_residual=False,
                 norm_layer=None, groups=1, width_per_group=64):
        super().__init__()
        if block is not BasicBlock or norm_layer not in (None, nn.BatchNorm2d) or not if_BN or groups != 1 or width_per_group != 64:
            raise NotImplementedError("ResNet_34 runs on the HIP path as the reference builds it: BasicBlock, nn.BatchNorm2d, if_BN=True, "
                                      "groups=1, width_per_group=64")
        if not 1 <= int(nclasses) <= 32:
            raise NotImplementedError(f"ResNet_34: 1..32 classes run on the HIP path (the class-column kernels), got {nclasses}")
        self.if_BN, self.dilation, self.aux = if_BN, 1, aux
        self.groups, self.base_width = groups, width_per_group
        self.conv1 = BasicConv2d(input_dim, 64, kernel_size=3, padding=1)
        self.conv2 = BasicConv2d(64, 128, kernel_size=3, padding=1)
        self.conv3 = BasicConv2d(128, 128, kernel_size=3, padding=1)
        self.inplanes = 128
        self.layer1 = self._make_layer(block, 128, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 128, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 128, layers[3], stride=2)
        self.conv_1 = BasicConv2d(640, 256, kernel_size=3, padding=1)
        self.conv_2 = BasicConv2d(256, 128, kernel_size=3, padding=1)
        self.semantic_output = nn.Conv2d(128, nclasses, 1)
        if self.aux:
            self.aux_head1 = nn.Conv2d(128, nclasses, 1)
            self.aux_head2 = nn.Conv2d(128, nclasses, 1)
            self.aux_head3 = nn.Conv2d(128, nclasses, 1)

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        if dilate:
            raise NotImplementedError("dilated stages are not implemented on the HIP path")
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride), nn.BatchNorm2d(planes * block.expansion))
        seq = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, self.dilation, if_BN=self.if_BN)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            seq.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation, if_BN=self.if_BN))
        return nn.Sequential(*seq)

    # ---------------- weight preparation: fpn.py's, cached in self._packed per parameter version and conv precision ----------------
    _prep = _fpn.SemanticNetworkWithFPN._prep
    _fold = staticmethod(_fpn.SemanticNetworkWithFPN._fold)
    _p_conv = _fpn.SemanticNetworkWithFPN._p_conv
    _p_conv_s2 = _fpn.SemanticNetworkWithFPN._p_conv_s2

    def _conv(self, name, conv: nn.Conv2d, bn, srcs, act=True, resid=None):
        """conv + folded BN [+ resid] [+ LeakyReLU(0.01), after the residual where there is one]."""
        p = self._p_conv(name, conv, bn)
        return ops.conv2d_fused(srcs, p.wpack, p.cout, p.k, p.dil, p.pad, bias=p.bias, slope=SLOPE if act else None, resid=resid,
                                precision=p.precision, act_after_resid=act and resid is not None)

    def _cbr(self, name, m: BasicConv2d, srcs):
        return self._conv(name, m.conv, m.bn, srcs)

    def _stage(self, lname: str, layer: nn.Sequential, x):
        for bi, blk in enumerate(layer):
            n = f"{lname}.{bi}"
            if blk.stride == 2:
                cin = x.shape[1]
                s2d = ops.space_to_depth2(x)
                p = self._p_conv_s2(n + ".conv1", blk.conv1, blk.bn1, cin)
                o1 = ops.conv2d_fused([ConvSource(s2d)], p.wpack, p.cout, 2, 1, 1, bias=p.bias, slope=SLOPE, precision=p.precision)
                idn = self._conv(n + ".down", blk.downsample[0], blk.downsample[1], [ConvSource(s2d, None, False, 0, cin)], act=False)   # phase (0,0)
            else:
                o1 = self._conv(n + ".conv1", blk.conv1, blk.bn1, [ConvSource(x)])
                idn = x if blk.downsample is None else self._conv(n + ".down", blk.downsample[0], blk.downsample[1], [ConvSource(x)], act=False)
            x = self._conv(n + ".conv2", blk.conv2, blk.bn2, [ConvSource(o1)], resid=idn)
        return x

    def _guard(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.conv1.conv.in_channels:
            raise RuntimeError(f"ResNet_34 expects x[B, {self.conv1.conv.in_channels}, H, W]")
        if any(isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training for m in self.modules()) or \
                (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            raise NotImplementedError("CENet's ResNet_34 is inference only on the HIP path: call model.eval() and run under torch.no_grad() "
                                      "(there is no backward, and the reference's CENet trainer does not run: CENet/trainer.py:18 imports a "
                                      "class that does not exist)")
        if not x.is_cuda:
            raise RuntimeError(f"semanticlidarunc_amd CENet runs on MI355X only: input is on '{x.device}' and there is no CPU fallback")
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise RuntimeError(f"ResNet_34 needs H and W divisible by 8 (three stride-2 stages), got {x.shape[2]} x {x.shape[3]}")
        if _sn.get_conv_precision() == "f16":
            raise RuntimeError("CENet's ResNet_34 does not run with conv precision 'f16': there is no half-precision storage path for this "
                               "model; use set_conv_precision('fp32') or set_conv_precision('f16x3')")
        return x.contiguous().float()

    def _head(self, name, conv: nn.Conv2d, x, size):
        """softmax over the classes of the 1x1 conv `conv` of x, interpolated (align_corners=True) to `size` -- the conv first."""
        return ops.bilinear_ac_softmax(self._conv(name, conv, None, [ConvSource(x)], act=False), size)

    def forward(self, x):
        x = self._guard(x)
        size = x.shape[2:]
        x = self._cbr("conv1", self.conv1, [ConvSource(x)])
        x = self._cbr("conv2", self.conv2, [ConvSource(x)])
        x = self._cbr("conv3", self.conv3, [ConvSource(x)])
        x_1 = self._stage("layer1", self.layer1, x)        # 1
        x_2 = self._stage("layer2", self.layer2, x_1)      # 1/2
        x_3 = self._stage("layer3", self.layer3, x_2)      # 1/4
        x_4 = self._stage("layer4", self.layer4, x_3)      # 1/8
        res = ops.bilinear_ac_cat([x_2, x_3, x_4], size)   # cat(res_2, res_3, res_4)
        out = self._cbr("conv_1", self.conv_1, [ConvSource(x), ConvSource(x_1), ConvSource(res)])
        out = self._cbr("conv_2", self.conv_2, [ConvSource(out)])
        out = self._head("semantic_output", self.semantic_output, out, size)
        if not self.aux:
            return out
        return [out, self._head("aux_head1", self.aux_head1, x_2, size), self._head("aux_head2", self.aux_head2, x_3, size),
                self._head("aux_head3", self.aux_head3, x_4, size)]


class CENet(nn.Module):
    def __init__(self, nclasses, aux=True, model="HarDNet", modeldir=None):
        super().__init__()
        self.aux = aux
        if model == "ResNet_34":
            self.model = ResNet_34(nclasses, aux=aux)
        elif model == "HarDNet":
            raise NotImplementedError("CENet(model='HarDNet') is not implemented on the HIP path; model='ResNet_34' is")
        else:
            raise ValueError(f"unknown CENet model {model!r}: 'ResNet_34' runs on the HIP path ('HarDNet' is the reference's other variant)")

    def forward(self, x) -> List[torch.Tensor]:
        return self.model.forward(x)
