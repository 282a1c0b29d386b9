"""The `semanticFCN_opt` variant of the ResNet-FPN segmenter on MI355X -- what the reference's `train_semantics.py:134` builds for
`baseline: Reichert` (src/baselines/Reichert/semanticFCN_opt.py:109-455) -- for the resnet18 / resnet34 / resnet50, efficientnet_v2_s / m / l
and (inference only, MC dropout on the stacked schedule) shufflenet_v2_x0_5 / x1_0 / x1_5 / x2_0, squeezenet1_0 and regnet_y_1_6gf / regnet_y_3_2gf
backbones (RegNetY: the default head -- UpsampleBlock scales 8 / 4 / 2 -- over `regnet.encode`; regnet_y_400mf / 800mf stay refused by name).

Same encoder as `fpn.SemanticNetworkWithFPN` (shared code: the family's `EncoderFamily.encode`, found with `fpn.family_of`; EfficientNetV2 with the
composed MBConv middle, `mbconv_fused_se = False`); the head differs:
  SpatialAttention (:73-85)   1x1 (C -> C/8, no bias) + ReLU -> 1x1 (-> 1) -> softmax over H*W -> x * w + x
                              = two fused conv launches + `slu_spatial_softmax_gate`
  UpsampleBlock (:10-28)      bilinear x8 / x4 / x2 (align_corners=False) -> conv3x3 (no bias) -> GroupNorm -> ReLU
                              = `slu_bilinear_upsample` + one conv launch + `slu_groupnorm_fwd` (ReLU fused)
  dropout_pyramid (:266)      nn.Dropout2d(0.1) on cat([x1, x2, x3, x4]): drawn by the real child on a [B,C,1,1] tensor of ones and folded
                              into the first decoder conv as per-(sample, channel) input multipliers -- so MC-dropout
                              (`utils.mc_dropout`) works on this model, unlike on `models/semanticFCN.py` which has no dropout
  decoder (:286-296)          conv3x3 -> GN -> ReLU -> conv3x3 -> GN -> ReLU -> UpsampleBlock(x2) -> conv1x1: RAW LOGITS (no ELU)
Contract kept: constructor keywords, `forward(x, meta) -> logits [B,num_classes,H,W]`, `state_dict` keys / shapes of the reference
class (checked against it in tools/gen_golden_r02.py), genuine `nn.Dropout2d` / `nn.GroupNorm` children.  Inference: folded launches
(`_forward`); training / any gradient: one autograd node per layer (`_forward_train_opt`), ResNet and EfficientNetV2 encoders alike.
Conv precision "f16" (resnet18 / resnet34, inference): fp16 storage throughout -- h8 convs with `slu_bilinear_upsample_h8`,
`slu_groupnorm_stats_h8` / `slu_groupnorm_apply_h8` and `slu_spatial_softmax_gate_h8` between them (`_pyramid_h8`, `_decoder_h8`).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import effnet as _eff
from . import h8 as _h8
from . import ops
from . import salsanext as _sn
from .fpn import RESNET_FAMILY
from .fpn import SemanticNetworkWithFPN as _FPNBase
from .fpn import family_of
from .ops import ConvSource


def _head_mc_h8_fits(blocks: int, classes: int, hw: int) -> bool:
    """What slu_head_mc_h8 takes (include/slu.h): 16 / 32 / 64 head input channels, at most 32 classes, H W a multiple of 32."""
    return blocks in (2, 4, 8) and classes <= 32 and hw % 32 == 0


class UpsampleBlock(nn.Module):
    """Interpolate -> 3x3 conv -> GroupNorm -> ReLU (module layout of the reference, :10-28)."""

    def __init__(self, in_ch: int, out_ch: int, scale: int, mode: str = "bilinear", groups: int = 8):
        super().__init__()
        self.scale, self.mode = scale, mode
        self.block = nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, padding=1, bias=False), nn.GroupNorm(math.gcd(groups, out_ch) or 1, out_ch),
                                   nn.ReLU(inplace=True))


def GN(channels, groups=32):
    g = min(groups, channels)
    return nn.GroupNorm(math.gcd(g, channels) or 1, channels)


class SpatialAttention(nn.Module):
    def __init__(self, in_ch, reduction=8):
        super().__init__()
        hid = max(1, in_ch // reduction)
        self.proj = nn.Conv2d(in_ch, hid, kernel_size=1, bias=False)
        self.score = nn.Conv2d(hid, 1, kernel_size=1, bias=False)


class SemanticNetworkWithFPN(_FPNBase):
    mbconv_fused_se = False      # the composed MBConv middle: slu_dwconv3x3_fwd, slu_global_avgpool + slu_se_gate (effnet.block_forward)

    def __init__(self, backbone="resnet18", input_channels=2, meta_channel_dim=3, interpolation_mode="nearest", num_classes=3,
                 attention=True, multi_scale_meta=True):
        nn.Module.__init__(self)
        fam = family_of(backbone)
        if fam is None:
            known = ("regnet_y_400mf", "regnet_y_800mf", "regnet_y_1_6gf", "regnet_y_3_2gf")
            if backbone in known:
                raise NotImplementedError(f"backbone '{backbone}' is not implemented on the HIP path yet (resnet18 / 34 / 50, efficientnet_v2_s / m / l, "
                                          "shufflenet_v2_x0_5 / x1_0 / x1_5 / x2_0 and squeezenet1_0 are, and so are regnet_y_1_6gf / regnet_y_3_2gf)")
            raise ValueError("Invalid ResNet type. Supported types: 'resnet18', 'resnet34', 'resnet50', 'regnet_y_400mf','regnet_y_800mf', "
                             "'regnet_y_1_6gf', 'regnet_y_3_2gf', 'shufflenet_v2_x0_5', 'shufflenet_v2_x1_0', 'shufflenet_v2_x1_5', "
                             "'shufflenet_v2_x2_0.")
        if interpolation_mode != "nearest":
            raise NotImplementedError("only interpolation_mode='nearest' (the reference default) runs on the HIP path")
        self.backbone_name, self.interpolation_mode = backbone, interpolation_mode
        self.num_classes, self.attention, self.multi_scale_meta = num_classes, attention, multi_scale_meta
        bc = fam.build(self, backbone, input_channels, meta_channel_dim)
        self.attention4, self.attention3 = SpatialAttention(bc[1]), SpatialAttention(bc[2])
        self.attention2, self.attention1 = SpatialAttention(bc[3]), SpatialAttention(bc[4])
        self.fpn_block4, self.fpn_block3 = self._fpn(bc[0], bc[1]), self._fpn(bc[1], bc[2])
        self.fpn_block2, self.fpn_block1 = self._fpn(bc[2], bc[3]), self._fpn(bc[3], bc[4])
        self.dropout_pyramid = nn.Dropout2d(p=0.1)
        # semanticFCN_opt.py:270-285: the shufflenet and efficientnet branches set is_shuffle (x4 and x3 both sit at 1/8 resolution there)
        # (and :274-278: x2 and x3 both sit at 1/4 resolution under SqueezeNet)
        scales = fam.head_scales
        out_chs = [bc[1] // scales[0], bc[2] // scales[1], bc[3] // scales[2]]
        self.upsample_layer_x4 = UpsampleBlock(bc[1], out_chs[0], scale=scales[0], mode="bilinear")
        self.upsample_layer_x3 = UpsampleBlock(bc[2], out_chs[1], scale=scales[1], mode="bilinear")
        self.upsample_layer_x2 = UpsampleBlock(bc[3], out_chs[2], scale=scales[2], mode="bilinear")
        self.decoder_semantic = nn.Sequential(
            nn.Conv2d(sum(out_chs) + bc[4], bc[4], 3, padding=1, bias=False), GN(bc[4]), nn.ReLU(inplace=True),
            nn.Conv2d(bc[4], bc[4], 3, padding=1, bias=False), GN(bc[4]), nn.ReLU(inplace=True),
            UpsampleBlock(bc[4], bc[4] // 2, scale=2),
            nn.Conv2d(bc[4] // 2, num_classes, kernel_size=1))

    # ---------------- head pieces ----------------
    def _spatial_attention(self, name, att: SpatialAttention, x):
        hid = self._conv(name + ".proj", att.proj, None, [ConvSource(x)], act="relu")
        score = self._conv(name + ".score", att.score, None, [ConvSource(hid)], act="none")
        return ops.spatial_softmax_gate(x, score)

    def _upsample_block(self, name, up: UpsampleBlock, srcs_before_interp):
        """UpsampleBlock.forward: the (single) input is interpolated, then conv -> GroupNorm -> ReLU."""
        if up.mode != "bilinear":
            raise NotImplementedError("UpsampleBlock: only mode='bilinear' (what the reference constructs) runs on the HIP path")
        xi = ops.bilinear_upsample(srcs_before_interp, up.scale)
        conv, gn = up.block[0], up.block[1]
        y = self._conv(name, conv, None, [ConvSource(xi)], act="none")
        return ops.groupnorm(y, gn.num_groups, gn.weight.detach(), gn.bias.detach(), gn.eps, relu=True, inplace=True)

    def _pyramid_dropout(self, n, c, device, scale_override: Optional[torch.Tensor]):
        """[n, c] multipliers of dropout_pyramid (None = identity), drawn by the real nn.Dropout2d child (its .training flag is what
        utils.mc_dropout.set_dropout_mode toggles)."""
        if scale_override is not None:
            return scale_override.reshape(n, c).to(device=device, dtype=torch.float32).contiguous()
        d = self.dropout_pyramid
        if not d.training or d.p == 0.0:
            return None
        return d(torch.ones((n, c, 1, 1), dtype=torch.float32, device=device)).reshape(n, c)

    def forward(self, x, meta_channel):
        return self._forward(x, meta_channel, None)

    def forward_with_dropout_scale(self, x, meta_channel, scale: torch.Tensor):
        """forward() with the dropout_pyramid multipliers given explicitly ([B, C_pyramid] or [B, C_pyramid, 1, 1]); parity tests."""
        return self._forward(x, meta_channel, scale)

    # ---------------- training path (fpn_autograd.py nodes; trainer.py:783-786 calls loss.backward() on this model) ----------------
    def _t_spatial_attention(self, name, att: SpatialAttention, x):
        from . import fpn_autograd as fa
        hid = fa.conv2d([x], att.proj.weight, None, 1, 0, 1, 0.0, None, None, self._dg(name + ".proj"))            # 1x1 -> ReLU in one node
        score = fa.conv2d([hid], att.score.weight, None, 1, 0, 1, None, None, None, self._dg(name + ".score"))
        return fa.SpatialGateFn.apply(x, score)

    def _t_upsample_block(self, name, up: UpsampleBlock, x):
        from . import fpn_autograd as fa
        if up.mode != "bilinear":
            raise NotImplementedError("UpsampleBlock: only mode='bilinear' (what the reference constructs) runs on the HIP path")
        conv, gn = up.block[0], up.block[1]
        y = fa.conv2d([fa.BilinearUpFn.apply(x, up.scale)], conv.weight, None, 3, 1, 1, None, None, None, self._dg(name))
        return fa.group_norm(gn, y, relu_after=True)

    # EfficientNetV2 encoder, training: the same blocks as effnet.block_forward, one autograd node per layer, batch-statistics BatchNorm (eps 1e-3),
    # StochasticDepth('row') live on the residual blocks (torchvision: `result = stochastic_depth(result); result += input`)
    def _t_cna(self, name, cna, srcs, resid=None):
        """Conv2dNormActivation (dense, stride 1): conv -> BatchNorm [+ resid] -> SiLU.  The residual form is only legal without activation (the
        projection of a block): the one configuration that adds it AFTER the SiLU (a FusedMBConv with expansion 1) sits in features[1], which the
        reference never calls."""
        from . import fpn_autograd as fa
        conv, bn = cna[0], cna[1]
        if resid is not None and len(cna) > 2:
            raise NotImplementedError("residual after the activation (FusedMBConv with expansion ratio 1) is not on the reference's path")
        y = fa.conv2d(srcs, conv.weight, None, conv.kernel_size[0], conv.padding[0], 1, None, bn, resid, self._dg(name))
        return fa.silu(y) if len(cna) > 2 else y

    def _sd_noise(self, name, blk, n, c, device):
        """[n, c] multipliers of torchvision's stochastic_depth(mode='row') for this block in train mode, None when it is the identity."""
        sd = blk.stochastic_depth
        if not sd.training or sd.p == 0.0:
            return None
        override = self.__dict__.get("_sd_noise_override")
        if override is not None:
            noise = override[name].to(device=device, dtype=torch.float32).reshape(n, 1)
        else:
            survival = 1.0 - sd.p
            noise = torch.empty((n, 1), dtype=torch.float32, device=device).bernoulli_(survival)
            if survival > 0.0:
                noise.div_(survival)
        return noise.expand(n, c).contiguous()

    def _t_project(self, name, blk, proj, h, x):
        """The block's last Conv2dNormActivation (no activation) + StochasticDepth + residual."""
        from . import fpn_autograd as fa
        if not blk.use_res_connect:
            return self._t_cna(name, proj, [h])
        noise = self._sd_noise(name.rsplit(".", 1)[0], blk, x.shape[0], proj[0].out_channels, x.device)
        if noise is None:
            return self._t_cna(name, proj, [h], resid=x)
        return fa.ScaleAddFn.apply(self._t_cna(name, proj, [h]), noise, x)

    def _t_eff_block(self, name, blk, x):
        import torch.nn.functional as F
        from . import fpn_autograd as fa
        seq = blk.block
        if isinstance(blk, _eff.FusedMBConv):
            first = seq[0]
            if len(seq) == 1:
                raise NotImplementedError("FusedMBConv with expansion ratio 1 (features[1]) is not on the reference's path")
            h = fa.silu(self._t_conv_s2(name + ".0", first[0], first[1], x)) if first[0].stride[0] == 2 else self._t_cna(name + ".0", first, [x])
            return self._t_project(name + ".1", blk, seq[1], h, x)
        i, h = 0, x
        if len(seq) == 4:                                               # 1x1 expansion
            h, i = self._t_cna(name + ".0", seq[0], [x]), 1
        dw, se, proj = seq[i], seq[i + 1], seq[i + 2]
        d = fa.DepthwiseConv3x3Fn.apply(h, dw[0].weight)
        if dw[0].stride[0] == 2:
            d = fa.NearestDownFn.apply(d, 2)                            # the stride-2 depthwise conv = the stride-1 one sampled at even pixels
        d = fa.silu(fa.batch_norm(dw[1], d))
        c, sq = se.fc1.in_channels, se.fc1.out_channels
        pooled = fa.GlobalAvgPoolFn.apply(d)                            # [N, C]; the two tiny fully-connected layers run as library GEMMs
        gate = torch.sigmoid(F.linear(F.silu(F.linear(pooled, se.fc1.weight.view(sq, c), se.fc1.bias)), se.fc2.weight.view(c, sq), se.fc2.bias))
        return self._t_project(f"{name}.{i + 2}", blk, proj, fa.ChannelGateFn.apply(d, gate), x)

    def _t_encode_effnet(self, x, meta):
        from . import fpn_autograd as fa
        if not self.multi_scale_meta:
            raise NotImplementedError("efficientnet backbones run with multi_scale_meta=True only (the reference's other branch feeds layer4 = "
                                      "features[6:] a tensor of the wrong channel count)")
        m1, m2, m3 = (fa.NearestDownFn.apply(meta, f) for f in (2, 4, 8))
        h = self._t_cna("stem", self.stem, [x, meta])
        outs = []
        for lname, stage, mk in (("layer1", self.layer1, None), ("layer2", self.layer2, m1), ("layer3", self.layer3, m2)):
            if mk is not None:
                h = fa.ReplaceTailFn.apply(h, mk)                       # :399-403: the stage sees cat(x[:, :-m], meta_k)
            for bi, blk in enumerate(stage):
                h = self._t_eff_block(f"{lname}.{bi}", blk, h)
            outs.append(h)
        return outs[0], outs[1], outs[2], fa.ReplaceTailFn.apply(outs[2], m3)      # :404: x4 = cat(x3[:, :-m], meta3) -- layer4 is never applied

    def _forward_train_opt(self, x, meta, drop_scale):
        from . import fpn_autograd as fa
        from . import autograd as _ag
        _ag.nbt_scope_enter()
        try:
            x1, x2, x3, x4 = self._t_encode_effnet(x, meta) if self.family is _eff.FAMILY else self._t_encode(x, meta)
            f4 = self._t_cbr("fpn4", self.fpn_block4[0], self.fpn_block4[1], [x4])
            f3 = self._t_cbr("fpn3", self.fpn_block3[0], self.fpn_block3[1], [x3])
            f2 = self._t_cbr("fpn2", self.fpn_block2[0], self.fpn_block2[1], [x2])
            f1 = self._t_cbr("fpn1", self.fpn_block1[0], self.fpn_block1[1], [x1])
            if self.attention:
                f4, f3 = self._t_spatial_attention("att4", self.attention4, f4), self._t_spatial_attention("att3", self.attention3, f3)
                f2, f1 = self._t_spatial_attention("att2", self.attention2, f2), self._t_spatial_attention("att1", self.attention1, f1)
            u4 = self._t_upsample_block("up4", self.upsample_layer_x4, f4)
            u3 = self._t_upsample_block("up3", self.upsample_layer_x3, f3)
            u2 = self._t_upsample_block("up2", self.upsample_layer_x2, f2)
            n = f1.shape[0]
            c1, c2, c3, c4 = f1.shape[1], u2.shape[1], u3.shape[1], u4.shape[1]
            s = self._pyramid_dropout(n, c1 + c2 + c3 + c4, f1.device, drop_scale)
            u34 = fa.DepthToSpaceCatFn.apply((1, 1), u3, u4)              # channel concatenation (the fused conv takes up to three sources)
            sc = None if s is None else (s[:, :c1].contiguous(), s[:, c1:c1 + c2].contiguous(), s[:, c1 + c2:].contiguous())
            d = self.decoder_semantic
            y = fa.conv2d([f1, u2, u34], d[0].weight, None, 3, 1, 1, None, None, None, self._dg("dec0"), scales=sc)
            y = fa.group_norm(d[1], y, relu_after=True)
            y = fa.conv2d([y], d[3].weight, None, 3, 1, 1, None, None, None, self._dg("dec1"))
            y = fa.group_norm(d[4], y, relu_after=True)
            y = self._t_upsample_block("dec_up", d[6], y)
            return fa.conv2d([y], d[7].weight, d[7].bias, 1, 0, 1, None, None, None, self._dg("dec_out"))
        finally:
            _ag.nbt_scope_exit()

    def _pyramid(self, x, meta):
        """The part of the inference forward no dropout can reach: encoder, FPN blocks, attention, UpsampleBlocks -> (f1, u2, u34), the three
        sources of the first decoder conv (cat([x1, x2, x3, x4]) with x3 and x4 sharing a buffer)."""
        x1, x2, x3, x4 = self.family.encode(self, x, meta)
        f4 = self._conv("fpn4", self.fpn_block4[0], self.fpn_block4[1], [ConvSource(x4)])
        f3 = self._conv("fpn3", self.fpn_block3[0], self.fpn_block3[1], [ConvSource(x3)])
        f2 = self._conv("fpn2", self.fpn_block2[0], self.fpn_block2[1], [ConvSource(x2)])
        f1 = self._conv("fpn1", self.fpn_block1[0], self.fpn_block1[1], [ConvSource(x1)])
        if self.attention:
            f4, f3 = self._spatial_attention("att4", self.attention4, f4), self._spatial_attention("att3", self.attention3, f3)
            f2, f1 = self._spatial_attention("att2", self.attention2, f2), self._spatial_attention("att1", self.attention1, f1)
        u4 = self._upsample_block("up4", self.upsample_layer_x4, f4)
        u3 = self._upsample_block("up3", self.upsample_layer_x3, f3)
        u2 = self._upsample_block("up2", self.upsample_layer_x2, f2)
        c3 = u3.shape[1]                                       # the fused conv takes up to three sources: x3 and x4 share a buffer
        u34 = torch.empty((u3.shape[0], c3 + u4.shape[1], u3.shape[2], u3.shape[3]), dtype=torch.float32, device=u3.device)
        u34[:, :c3].copy_(u3)
        u34[:, c3:].copy_(u4)
        return f1, u2, u34

    def _decoder(self, f1, u2, u34, s, passes: int = 0, raw_head_input: bool = False):
        """dropout_pyramid multipliers s ([N, C_pyramid] or None) -> decoder_semantic.  passes = T > 0: the pyramid holds B images and the
        decoder runs T * B stacked passes, its first conv reading image n % B in place.  raw_head_input: stop at the UpsampleBlock's raw conv
        output (what slu_head_mc_f32 normalises itself)."""
        b = f1.shape[0]
        c1, c2 = f1.shape[1], u2.shape[1]
        sc = (None, None, None) if s is None else (s[:, :c1].contiguous(), s[:, c1:c1 + c2].contiguous(), s[:, c1 + c2:].contiguous())
        d = self.decoder_semantic
        if passes:
            y = self._conv("dec0", d[0], None, [ConvSource(f1, sc[0], False, b), ConvSource(u2, sc[1], False, b), ConvSource(u34, sc[2], False, b)],
                           act="none", n_out=passes * b)
        else:
            y = self._conv("dec0", d[0], None, [ConvSource(f1, sc[0]), ConvSource(u2, sc[1]), ConvSource(u34, sc[2])], act="none")
        y = ops.groupnorm(y, d[1].num_groups, d[1].weight.detach(), d[1].bias.detach(), d[1].eps, relu=True, inplace=True)
        y = self._conv("dec1", d[3], None, [ConvSource(y)], act="none")
        y = ops.groupnorm(y, d[4].num_groups, d[4].weight.detach(), d[4].bias.detach(), d[4].eps, relu=True, inplace=True)
        if raw_head_input:
            up = d[6]
            if up.mode != "bilinear":
                raise NotImplementedError("UpsampleBlock: only mode='bilinear' (what the reference constructs) runs on the HIP path")
            return self._conv("dec_up", up.block[0], None, [ConvSource(ops.bilinear_upsample(y, up.scale))], act="none")
        y = self._upsample_block("dec_up", d[6], y)
        return self._conv("dec_out", d[7], None, [ConvSource(y)], act="none")

    # ---------------- half-precision storage path (conv precision "f16"): h8 tensors [N, G, H, W, 8] fp16 throughout ----------------
    def _use_h8(self) -> bool:
        """Conv precision "f16" selects the h8 route; it covers the BasicBlock encoders only."""
        if _sn.get_conv_precision() != "f16":
            return False
        if self.family is not RESNET_FAMILY or self.backbone_name == "resnet50":
            raise RuntimeError(f"semanticFCN_opt with the {self.backbone_name} backbone does not run with conv precision 'f16': the half-precision "
                               "storage path covers the BasicBlock backbones (resnet18 / resnet34) only; use set_conv_precision('fp32')")
        return True

    @staticmethod
    def _gn_h8(y, gn: nn.GroupNorm, out=None, g_off=0):
        """GroupNorm + ReLU of an h8 tensor: statistics, then apply in place (or into blocks [g_off, ...) of `out`)."""
        stats = _h8.groupnorm_stats_h8(y, gn.num_channels, gn.num_groups, gn.eps)
        return _h8.groupnorm_apply_h8(y, gn.num_channels, gn.num_groups, stats, gn.weight.detach(), gn.bias.detach(), True,
                                      y if out is None else out, g_off)

    def _head_h8(self, name, conv: nn.Conv2d, x):
        """A 1x1 conv of an h8 tensor with fp32 NCHW output and no activation (the `score` conv of an attention, the logits head)."""
        p = self._p_conv(name, conv, None)
        return _h8.conv2d_h8([_h8.H8Source(x)], p.wpack, p.cin, p.cout, p.k, p.dil, p.pad, bias=p.bias, out_f32_nchw=True)

    def _spatial_attention_h8(self, name, att: SpatialAttention, x):
        hid = self._run_h8(self._p_conv(name + ".proj", att.proj, None), [x])
        return _h8.spatial_softmax_gate_h8(x, self._head_h8(name + ".score", att.score, hid))

    def _upsample_conv_h8(self, name, up: UpsampleBlock, x):
        """UpsampleBlock up to its raw conv output: bilinear kernel, then the 3x3 conv with no bias and no activation."""
        if up.mode != "bilinear":
            raise NotImplementedError("UpsampleBlock: only mode='bilinear' (what the reference constructs) runs on the HIP path")
        return self._run_h8(self._p_conv(name, up.block[0], None), [_h8.bilinear_upsample_h8(x, up.scale)], relu=False)

    def _pyramid_h8(self, x, meta):
        """`_pyramid` on the h8 path -> (f1, ups): the two sources of the first decoder conv, the three UpsampleBlocks in block slices of one
        buffer (cat([x2, x3, x4]) of the reference's forward)."""
        x1, x2, x3, x4 = self._encode_h8(x, meta)
        f4 = self._run_h8(self._p_conv("fpn4", self.fpn_block4[0], self.fpn_block4[1]), [x4])
        f3 = self._run_h8(self._p_conv("fpn3", self.fpn_block3[0], self.fpn_block3[1]), [x3])
        f2 = self._run_h8(self._p_conv("fpn2", self.fpn_block2[0], self.fpn_block2[1]), [x2])
        f1 = self._run_h8(self._p_conv("fpn1", self.fpn_block1[0], self.fpn_block1[1]), [x1])
        if self.attention:
            f4, f3 = self._spatial_attention_h8("att4", self.attention4, f4), self._spatial_attention_h8("att3", self.attention3, f3)
            f2, f1 = self._spatial_attention_h8("att2", self.attention2, f2), self._spatial_attention_h8("att1", self.attention1, f1)
        blocks = (("up2", self.upsample_layer_x2, f2), ("up3", self.upsample_layer_x3, f3), ("up4", self.upsample_layer_x4, f4))
        chans = [up.block[0].out_channels for _, up, _ in blocks]
        if any(c % 8 for c in chans):
            raise RuntimeError(f"semanticFCN_opt on the h8 path: UpsampleBlock widths {chans} are not whole blocks of 8 channels")
        ups = torch.empty((f1.shape[0], sum(chans) // 8, f1.shape[2], f1.shape[3], 8), dtype=torch.float16, device=f1.device)
        g_off = 0
        for (name, up, f), c in zip(blocks, chans):
            self._gn_h8(self._upsample_conv_h8(name, up, f), up.block[1], ups, g_off)
            g_off += c // 8
        return f1, ups

    def _decoder_h8(self, f1, ups, s, passes: int = 0, raw_head_input: bool = False):
        """`_decoder` on the h8 path: the dropout multipliers are the first conv's per-source scales (each rounded to fp16, the product rounded
        once: slu.h); passes = T > 0: both sources are batch-broadcast and the conv writes T * B images.  Returns fp32 NCHW logits, or with
        raw_head_input the h8 output of the last UpsampleBlock's conv (before its GroupNorm)."""
        b = f1.shape[0]
        c1 = 8 * f1.shape[1]
        d = self.decoder_semantic
        if c1 + 8 * ups.shape[1] != d[0].in_channels:
            raise RuntimeError("semanticFCN_opt on the h8 path: the pyramid's channels are not whole blocks of 8")
        sc = (None, None) if s is None else (s[:, :c1].contiguous(), s[:, c1:].contiguous())
        nb = b if passes else 0
        p = self._p_conv("dec0", d[0], None)
        y = _h8.conv2d_h8([_h8.H8Source(f1, sc[0], nb), _h8.H8Source(ups, sc[1], nb)], p.wpack, p.cin, p.cout, p.k, p.dil, p.pad, bias=p.bias,
                          n_out=passes * b if passes else None)
        y = self._gn_h8(y, d[1])
        y = self._gn_h8(self._run_h8(self._p_conv("dec1", d[3], None), [y], relu=False), d[4])
        y = self._upsample_conv_h8("dec_up", d[6], y)
        if raw_head_input:
            return y
        return self._head_h8("dec_out", d[7], self._gn_h8(y, d[6].block[1]))

    def _forward(self, x, meta_channel, drop_scale):
        x, meta = self._check_inputs(x, meta_channel)
        if not self.family.trains_in_opt:
            self._inference_guard(x, meta, "semanticFCN_opt")
        if self._wants_autograd(x, meta):
            return self._forward_train_opt(x, meta, drop_scale)
        if self._use_h8():
            f1, ups = self._pyramid_h8(x, meta)
            s = self._pyramid_dropout(f1.shape[0], self.decoder_semantic[0].in_channels, f1.device, drop_scale)
            return self._decoder_h8(f1, ups, s)
        f1, u2, u34 = self._pyramid(x, meta)
        # cat([x1, x2, x3, x4]) -> dropout_pyramid -> decoder conv: three sources (x1 | x2 | x3 + x4 share a buffer), multipliers per source
        s = self._pyramid_dropout(f1.shape[0], f1.shape[1] + u2.shape[1] + u34.shape[1], f1.device, drop_scale)
        return self._decoder(f1, u2, u34, s)

    # ---------------- MC dropout with the pyramid computed once (utils.mc_dropout, share_prefix=True) ----------------
    def _mc_shared(self, x, meta_channel, T: int, scale, raw_head_input: bool):
        if self.training:
            raise RuntimeError("forward_mc needs the model in eval mode (use utils.mc_dropout.mc_forward)")
        if not self.family.mc_shared_prefix:
            # the shared-prefix schedule runs the encoder at N = B and the stacked one at N = T B: equal to rounding, not verified bit for bit
            # for these encoders, so it is refused rather than allowed to differ silently
            raise RuntimeError(f"semanticFCN_opt with the {self.backbone_name} backbone runs MC dropout on the stacked schedule only: "
                               "use utils.mc_dropout.mc_predict / mc_forward with share_prefix=False")
        x, meta = self._check_inputs(x, meta_channel)
        if self._wants_autograd(x, meta):
            raise RuntimeError("forward_mc is inference only: no train-mode BatchNorm and no gradients")
        t = int(T)
        if t < 1:
            raise RuntimeError("forward_mc: T must be at least 1")
        if self._use_h8():
            f1, ups = self._pyramid_h8(x, meta)
            s = self._pyramid_dropout(t * f1.shape[0], self.decoder_semantic[0].in_channels, f1.device, scale)
            return self._decoder_h8(f1, ups, s, passes=t, raw_head_input=raw_head_input)
        f1, u2, u34 = self._pyramid(x, meta)
        s = self._pyramid_dropout(t * f1.shape[0], f1.shape[1] + u2.shape[1] + u34.shape[1], f1.device, scale)
        return self._decoder(f1, u2, u34, s, passes=t, raw_head_input=raw_head_input)

    @torch.no_grad()
    def forward_mc(self, x, meta_channel, T: int, scale: Optional[torch.Tensor] = None):
        """T stochastic passes of a batch -> logits [T*B, num_classes, H, W] (pass-major).  dropout_pyramid is the model's only dropout and sits
        behind the encoder, the FPN blocks, the attentions and the UpsampleBlocks, so all of that runs ONCE at N = B; only decoder_semantic runs
        at N = T*B, its first conv reading the B pyramid images in place.  The multipliers are one draw of the real dropout_pyramid child on
        ones(T*B, C_pyramid, 1, 1) -- the draw the stacked forward makes, so the same seed gives the same passes -- unless `scale`
        ([T*B, C_pyramid]) gives them.  Equals forward() on the inputs repeated T times.  Inference only."""
        return self._mc_shared(x, meta_channel, T, scale, False)

    def mc_fused_ok(self, x, meta_channel, T: int) -> bool:
        """slu_head_mc_f32 covers this model's head: eval-mode inference on fp32 GPU inputs, at most 32 classes and 128 head input channels
        (under conv precision "f16" mc_predict_fused takes slu_head_mc_h8 or, where that does not fit, the unfused reduction)."""
        if self.training or not all(isinstance(t, torch.Tensor) and t.dim() == 4 and t.is_cuda and t.dtype == torch.float32 for t in (x, meta_channel)):
            return False
        head = self.decoder_semantic[7]
        return int(T) >= 1 and head.out_channels <= 32 and head.in_channels <= 128 and not self._wants_autograd(x, meta_channel)

    @torch.no_grad()
    def mc_predict_fused(self, x, meta_channel, T: int, eps: float = 1e-12, scale: Optional[torch.Tensor] = None):
        """(p_bar, H_norm, MI_norm, preds) of T stochastic passes: the shared pyramid and the decoder up to the last UpsampleBlock's raw conv
        output, then its GroupNorm statistics, then GroupNorm apply + ReLU + the 1x1 head + the MC reduction in one launch
        (csrc/head_mc_f32.hip): neither the normalised tensor nor the T*B logit maps are written.  Under conv precision "f16": GroupNorm + ReLU in
        place on the h8 tensor, then head + reduction in one launch (csrc/head_mc_h8.hip).  Call under utils.mc_dropout.dropout_sampling."""
        y = self._mc_shared(x, meta_channel, T, scale, True)
        gn, head = self.decoder_semantic[6].block[1], self.decoder_semantic[7]
        if y.dtype == torch.float16:
            # the h8 route: GroupNorm + ReLU in place, then the 1x1 head + the MC reduction in one launch (slu_head_mc_h8: 16 / 32 / 64 input
            # channels, H W a multiple of 32); any other shape: the head conv's fp32 logits through the reduction kernel
            y = self._gn_h8(y, gn)
            t = int(T)
            if _head_mc_h8_fits(y.shape[1], head.out_channels, y.shape[2] * y.shape[3]):
                p = self._p_conv("dec_out", head, None)
                return _h8.head_mc_h8(y, p.wpack, p.bias, head.out_channels, t, y.shape[0] // t, eps)
            logits = self._head_h8("dec_out", head, y)
            return ops.mc_reduce(logits.view(t, logits.shape[0] // t, *logits.shape[1:]), eps)
        stats = ops.groupnorm_stats(y, gn.num_groups, gn.eps)
        return ops.head_mc_f32(y, head.weight.detach(), None if head.bias is None else head.bias.detach(), int(T), y.shape[0] // int(T), eps,
                               gn_stats=stats, gn_groups=gn.num_groups, gn_gamma=gn.weight.detach(), gn_beta=gn.bias.detach(), relu=True)
