"""FIDNet's ResNet34_point range-image segmenter on MI355X, inference only: the reference's `FIDNet(nclasses, backbone="ResNet34_point",
with_normal)` contract (src/baselines/FIDNet/FIDNet.py:21-42, ResNet.py:29-170, 451-593, 668-675) over the fused HIP conv, the fused point-MLP
stem (csrc/point_mlp.hip) and the decoder kernels of csrc/cenet_ops.hip.

Contract kept: constructor arguments, module names, parameter shapes and default initialisation (the `state_dict` is the reference's, key for
key), `forward(x[B, 5 or 8, H, W])` -> class LOGITS `[B, nclasses, H, W]` (the reference applies no softmax).  BasicBlock holds parameters only;
`ResNet_34_point.forward` and `SemanticHead.forward` keep the reference's own contracts (the 1024-channel concatenation; the three convs over any
`[B, input_channel, H, W]` tensor) and `Final_Model.forward` / `FIDNet.forward` take the fast route below.  The two ASPP backbones and training are
not provided.

How the layers map onto kernels (eval BatchNorm folded into the preceding conv's weights and bias; fpn.py's weight preparation and cache, per
parameter version and conv precision):
  conv1 .. conv4 + BN + LeakyReLU .. ONE slu_point_mlp launch: Cin -> 64 -> 128 -> 256 -> 512 per pixel, the 64-, 128- and 256-channel maps stay in
                                    LDS (exact fp32 products under both conv precisions); composed form: four 1x1 fused-conv launches
  layer1 .. layer4 ................ CENet's block mapping (cenet.py): conv + BN + LeakyReLU in one launch, LeakyReLU after the residual add, a
                                    stride-2 entry as space-to-depth + the re-indexed 2x2 conv with the downsample conv on phase (0, 0);
                                    layer1.0 has a stride-1 1x1 downsample from 512 to 128 channels
  head, commuted .................. conv_1 (+ bn1) over cat(x, x_1, res_2, res_3, res_4) is linear in its input and a 1x1 conv commutes with the
                                    bilinear interpolation (its four weights sum to 1): the column slices [640:768], [768:896], [896:1024] of
                                    the folded weight run as 128 -> 512 convs on the LOW-resolution x_2, x_3, x_4 (no bias, no activation), ONE
                                    slu_bilinear_ac_sum launch interpolates and adds the three, and conv_1 runs over (x, x_1) with that sum as
                                    its residual, its bias, and the LeakyReLU after the add.  Equal to the reference order up to rounding.
                                    composed form: slu_bilinear_ac_cat into a 384-channel buffer and conv_1 over (x, x_1, buffer)
  conv_2 (+ bn2), semantic_output . plain fused 1x1 convs
Which form a precision runs by default is `FUSED_STEM` / `COMMUTED_HEAD` below, decided by tools/fidnet_bench.py: as measured, the
fused stem under f16x3 only, and the composed head under both precisions; the other forms stay reachable (`Final_Model._forward`) and tested.
Conv precision "fp32" and "f16x3" run; "f16" (half-precision storage) is refused."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import cenet as _cenet
from . import fpn as _fpn
from . import ops
from . import salsanext as _sn
from .cenet import SLOPE, conv1x1, conv3x3  # noqa: F401  (conv3x3 / conv1x1: the reference module's names)
from .ops import ConvSource

# conv precision -> whether the fused form is the model's default.  A fused route is the default only where it is not slower than its composed
# form at 64 x 2048 and at 128 x 2048 (profiles/r32).  Measured, fused / composed ms at the two shapes:
#   stem   fp32   0.511 / 0.512, 0.997 / 0.977
#          f16x3  0.515 / 0.715, 1.002 / 1.340
#   head   fp32   1.257 / 1.221, 2.498 / 2.464
#          f16x3  1.581 / 1.384, 3.069 / 2.693
FUSED_STEM = {"fp32": False, "f16x3": True}
COMMUTED_HEAD = {"fp32": False, "f16x3": False}

RUNS = "backbone='ResNet34_point' runs on the HIP path (inference, conv precision 'fp32' or 'f16x3', CUDA tensors, H and W divisible by 8)"


class _Prepared(nn.Module):
    """fpn.py's weight preparation, cached in the module per parameter version and conv precision."""
    _cached = _fpn.SemanticNetworkWithFPN._cached
    _prep = _fpn.SemanticNetworkWithFPN._prep
    _fold = staticmethod(_fpn.SemanticNetworkWithFPN._fold)
    _p_conv = _fpn.SemanticNetworkWithFPN._p_conv
    _p_conv_s2 = _fpn.SemanticNetworkWithFPN._p_conv_s2
    _conv = _cenet.ResNet_34._conv          # conv + folded BN [+ resid] [+ LeakyReLU(0.01), after the residual where there is one]

    def _guard(self, x, cin, what):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != cin:
            raise RuntimeError(f"{what} expects x[B, {cin}, H, W]")
        if any(isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training for m in self.modules()) or \
                (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            raise NotImplementedError("FIDNet is inference only on the HIP path: call model.eval() and run under torch.no_grad() (there is no "
                                      f"backward); {RUNS}")
        if not x.is_cuda:
            raise RuntimeError(f"semanticlidarunc_amd FIDNet runs on MI355X only: input is on '{x.device}' and there is no CPU fallback; {RUNS}")
        if _sn.get_conv_precision() == "f16":
            raise RuntimeError("FIDNet does not run with conv precision 'f16': there is no half-precision storage path for this model; use "
                               "set_conv_precision('fp32') or set_conv_precision('f16x3')")
        return x.contiguous().float()


# ----------------------------------------------------------------------------------------------------------------
# containers (names, shapes and construction order of FIDNet/ResNet.py: the default initialisation draws the reference's random numbers)
# ----------------------------------------------------------------------------------------------------------------
class BasicBlock(_cenet.BasicBlock):
    def forward(self, *args, **kwargs):
        raise NotImplementedError("BasicBlock is a parameter container: the forward pass is ResNet_34_point's (semanticlidarunc_amd/fidnet.py)")


class SemanticHead(_Prepared):
    def __init__(self, num_class=20, input_channel=1024):
        super().__init__()
        self.conv_1 = nn.Conv2d(input_channel, 512, 1)
        self.bn1 = nn.BatchNorm2d(512)
        self.relu_1 = nn.LeakyReLU()
        self.conv_2 = nn.Conv2d(512, 128, 1)
        self.bn2 = nn.BatchNorm2d(128)
        self.relu_2 = nn.LeakyReLU()
        self.semantic_output = nn.Conv2d(128, num_class, 1)

    def _tail(self, res):
        res = self._conv("conv_2", self.conv_2, self.bn2, [ConvSource(res)])
        return self._conv("semantic_output", self.semantic_output, None, [ConvSource(res)], act=False)

    def forward(self, input_tensor):
        """The reference's contract: conv_1 + bn1 + LeakyReLU, conv_2 + bn2 + LeakyReLU, semantic_output over a materialised tensor."""
        t = self._guard(input_tensor, self.conv_1.in_channels, "SemanticHead")
        return self._tail(self._conv("conv_1", self.conv_1, self.bn1, [ConvSource(t)]))

    def _p_slice(self, name, lo, hi, bias):
        """conv_1 + bn1 restricted to the input channels [lo, hi), with or without the folded bias."""
        def make():
            w, b = self._fold(self.conv_1.weight, self.conv_1.bias, self.bn1)
            return w[:, lo:hi], b if bias else None, 1, 1, 0
        bn = self.bn1
        return self._prep(name, make, self.conv_1.weight, self.conv_1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def _from_pyramid(self, x, x_1, lows, size, commuted):
        """The logits from the backend's maps without the 1024-channel concatenation: x [B, 512, H, W], x_1 [B, 128, H, W], lows = (x_2, x_3, x_4)."""
        return self._tail(self._conv_1_from_pyramid(x, x_1, lows, size, commuted))

    def _conv_1_from_pyramid(self, x, x_1, lows, size, commuted):
        """relu_1(bn1(conv_1(cat(x, x_1, the maps of `lows` interpolated to `size`)))) in the commuted or the composed form (head of the file)."""
        c0, c1 = x.shape[1], x_1.shape[1]
        at = c0 + c1
        if at + sum(t.shape[1] for t in lows) != self.conv_1.in_channels:
            raise RuntimeError(f"SemanticHead: the maps have {at + sum(t.shape[1] for t in lows)} channels, conv_1 takes {self.conv_1.in_channels}")
        if commuted:
            parts = []
            for k, t in enumerate(lows):
                p = self._p_slice(f"conv_1.low{k}", at, at + t.shape[1], False)
                parts.append(ops.conv2d_fused([ConvSource(t)], p.wpack, p.cout, 1, 1, 0, precision=p.precision))
                at += t.shape[1]
            p = self._p_slice("conv_1.full_res", 0, c0 + c1, True)
            res = ops.conv2d_fused([ConvSource(x), ConvSource(x_1)], p.wpack, p.cout, 1, 1, 0, bias=p.bias, slope=SLOPE,
                                   resid=ops.bilinear_ac_sum(parts, size), precision=p.precision, act_after_resid=True)
        else:
            res = self._conv("conv_1", self.conv_1, self.bn1, [ConvSource(x), ConvSource(x_1), ConvSource(ops.bilinear_ac_cat(list(lows), size))])
        return res


class ResNet_34_point(_Prepared):
    def __init__(self, block, layers, if_BN, if_remission, if_range, with_normal, zero_init_residual=False, norm_layer=None, groups=1,
                 width_per_group=64):
        super().__init__()
        if block is not BasicBlock or norm_layer not in (None, nn.BatchNorm2d) or not if_BN or groups != 1 or width_per_group != 64:
            raise NotImplementedError("ResNet_34_point runs on the HIP path as the reference builds it: BasicBlock, nn.BatchNorm2d, if_BN=True, "
                                      "groups=1, width_per_group=64")
        self._norm_layer = nn.BatchNorm2d
        self.if_BN, self.if_remission, self.if_range, self.with_normal = if_BN, if_remission, if_range, with_normal
        self.inplanes, self.dilation = 512, 1
        self.groups, self.base_width = groups, width_per_group
        cin = {(False, False, False): 3, (True, False, False): 4, (True, True, False): 5, (True, True, True): 8}.get(
            (bool(if_remission), bool(if_range), bool(with_normal)))
        if cin is None:
            raise ValueError("ResNet_34_point: the reference builds conv1 for (if_remission, if_range, with_normal) = (F, F, F), (T, F, F), "
                             "(T, T, F) and (T, T, T) only (ResNet.py:469-487)")
        self.conv1 = nn.Conv2d(cin, 64, kernel_size=1, stride=1, padding=0, bias=True)
        self.bn_0 = nn.BatchNorm2d(64)
        self.relu_0 = nn.LeakyReLU()
        self.conv2 = nn.Conv2d(64, 128, kernel_size=1, stride=1, padding=0, bias=True)
        self.bn = nn.BatchNorm2d(128)
        self.relu = nn.LeakyReLU()
        self.conv3 = nn.Conv2d(128, 256, kernel_size=1, stride=1, padding=0, bias=True)
        self.bn_1 = nn.BatchNorm2d(256)
        self.relu_1 = nn.LeakyReLU()
        self.conv4 = nn.Conv2d(256, 512, kernel_size=1, stride=1, padding=0, bias=True)
        self.bn_2 = nn.BatchNorm2d(512)
        self.relu_2 = nn.LeakyReLU()
        self.layer1 = self._make_layer(block, 128, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 128, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 128, layers[3], stride=2)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)

    _make_layer = _cenet.ResNet_34._make_layer
    _stage = _cenet.ResNet_34._stage

    def _stem_layers(self):
        return (("conv1", self.conv1, self.bn_0), ("conv2", self.conv2, self.bn), ("conv3", self.conv3, self.bn_1), ("conv4", self.conv4, self.bn_2))

    def _stem(self, x, fused):
        layers = self._stem_layers()
        if not fused:
            for name, conv, bn in layers:
                x = self._conv(name, conv, bn, [ConvSource(x)])
            return x

        def make():
            folded = [self._fold(conv.weight, conv.bias, bn) for _, conv, bn in layers]
            return ops.pack_point_mlp([w.float().contiguous() for w, _ in folded]), torch.cat([b.float() for _, b in folded]).contiguous()
        deps = [t for _, conv, bn in layers for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        wpack, bias = self._cached("_stem_cache", "stem", deps, make)
        return ops.point_mlp(x, wpack, bias, [conv.out_channels for _, conv, _ in layers], SLOPE)

    def _features(self, x, fused_stem=None):
        """(x, x_1, x_2, x_3, x_4) of ResNet.py:563-581 at 1, 1, 1/2, 1/4, 1/8 resolution."""
        x = self._guard(x, self.conv1.in_channels, "ResNet_34_point")
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise RuntimeError(f"ResNet_34_point needs H and W divisible by 8 (three stride-2 stages), got {x.shape[2]} x {x.shape[3]}")
        x = self._stem(x, FUSED_STEM[_sn.get_conv_precision()] if fused_stem is None else fused_stem)
        x_1 = self._stage("layer1", self.layer1, x)
        x_2 = self._stage("layer2", self.layer2, x_1)
        x_3 = self._stage("layer3", self.layer3, x_2)
        x_4 = self._stage("layer4", self.layer4, x_3)
        return x, x_1, x_2, x_3, x_4

    def forward(self, x):
        """The reference's contract: torch.cat([x, x_1, res_2, res_3, res_4], 1), materialised as [B, 1024, H, W]."""
        x, x_1, x_2, x_3, x_4 = self._features(x)
        c0, c1 = x.shape[1], x_1.shape[1]
        out = torch.empty((x.shape[0], c0 + c1 + x_2.shape[1] + x_3.shape[1] + x_4.shape[1]) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        out[:, :c0].copy_(x)
        out[:, c0:c0 + c1].copy_(x_1)
        at = c0 + c1
        return ops.bilinear_ac_cat([x_2, x_3, x_4], x.shape[2:], out=out, c_offs=(at, at + x_2.shape[1], at + x_2.shape[1] + x_3.shape[1]))


class Final_Model(nn.Module):
    def __init__(self, backbone_net, semantic_head):
        super().__init__()
        self.backend = backbone_net
        self.semantic_head = semantic_head

    def forward(self, x):
        """semantic_head(backend(x)) without the 1024-channel concatenation, each part in the default form of the conv precision."""
        return self._forward(x)

    def _forward(self, x, fused_stem=None, commuted_head=None):
        """fused_stem / commuted_head: None takes the default of the conv precision (FUSED_STEM / COMMUTED_HEAD), True / False force a form
        (the A/B of tools/fidnet_bench.py and the tests of the forms that are not a default)."""
        if not isinstance(self.backend, ResNet_34_point):
            return self.semantic_head(self.backend(x))
        self.semantic_head._guard(x, self.backend.conv1.in_channels, "FIDNet")
        x0, x_1, x_2, x_3, x_4 = self.backend._features(x, fused_stem)
        commuted = COMMUTED_HEAD[_sn.get_conv_precision()] if commuted_head is None else commuted_head
        return self.semantic_head._from_pyramid(x0, x_1, (x_2, x_3, x_4), x0.shape[2:], commuted)


def resnet34_point(if_BN, if_remission, if_range, with_normal):
    return ResNet_34_point(BasicBlock, [3, 4, 6, 3], if_BN, if_remission, if_range, with_normal, zero_init_residual=False)


class FIDNet(nn.Module):
    def __init__(self, nclasses, backbone="ResNet34_aspp_1", with_normal=False):
        super().__init__()
        if backbone in ("ResNet34_aspp_1", "ResNet34_aspp_2"):
            raise NotImplementedError(f"FIDNet(backbone={backbone!r}) is not implemented on the HIP path (its dilated 3x3 convs read a 768- or "
                                      f"896-channel concatenation of five maps); {RUNS}")
        if backbone != "ResNet34_point":
            raise ValueError(f"unknown FIDNet backbone {backbone!r}; {RUNS}")
        Backend = resnet34_point(if_BN=True, if_remission=True, if_range=True, with_normal=with_normal)
        S_H = SemanticHead(nclasses, 1024)
        self.model = Final_Model(Backend, S_H)

    def forward(self, x):
        return self.model(x)
