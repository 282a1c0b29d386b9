"""Independent restatement of the two FPN segmenters with a RegNetY encoder, as pure functions of a ``state_dict`` (plain torch CPU ops; fp64
when given fp64 tensors).  TEST INFRASTRUCTURE ONLY -- it never imports semanticlidarunc_amd/regnet.py.

  RegNetYRef           torchvision's public RegNetY (regnet_y_400mf / 800mf / 1_6gf / 3_2gf) written out with a forward: what
                       tools/gen_golden_regnet.py serves to the reference's classes as `torchvision.models.regnet_y_*`
  y_block              one ResBottleneckBlock from a state_dict prefix
  encode               stem (conv 3x3 / stride 1 without bias, BN, ReLU), layer1..4 = trunk_output[0..3], the meta channels injected into
                       layer2, layer3 and layer4 (reference models/semanticFCN.py:171-179, :305-314)
  fpn_forward          models/semanticFCN.py: ConvTranspose k8s8 / k4s4 / k2s2, ELU + 1
  fpn_opt_forward      baselines/Reichert/semanticFCN_opt.py: UpsampleBlock scales 8 / 4 / 2 (oracle.fpn_opt's head)
  he_fixture_          the fixture of the tests: He weights over the whole model, N(0, 0.5) SE biases, random BatchNorms, and the weight of every
                       block's last BatchNorm (f.c.1) times 0.25 -- without that factor the residual stream of the 27-block 1_6gf grows to 5e4
Four wrong variants a fixture must notice: `leaky_halo` (f.b sees relu(f.a's BatchNorm shift) -- f.a of a zero-padded input -- instead of 0
outside the image), `se_half` (every SE gate replaced by 0.5), `phase11` (the stride-2 convs sample phase (1, 1) instead of (0, 0)) and zeroed
meta channels (the caller passes zeros)."""
import math
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.fpn import _attention, _bn, _cbr
from oracle.fpn_opt import _head as _opt_head

# name -> (depth, w_0, w_a, w_m, group width), and what the generator must give for it
PARAMS = {"regnet_y_400mf": (16, 48, 27.89, 2.09, 8), "regnet_y_800mf": (14, 56, 38.84, 2.4, 16),
          "regnet_y_1_6gf": (27, 48, 20.71, 2.65, 24), "regnet_y_3_2gf": (21, 80, 42.63, 2.66, 24)}
WIDTHS = {"regnet_y_400mf": [48, 104, 208, 440], "regnet_y_800mf": [64, 144, 320, 784],
          "regnet_y_1_6gf": [48, 120, 336, 888], "regnet_y_3_2gf": [72, 216, 576, 1512]}
DEPTHS = {"regnet_y_400mf": [1, 3, 6, 6], "regnet_y_800mf": [1, 3, 8, 2], "regnet_y_1_6gf": [2, 6, 17, 2], "regnet_y_3_2gf": [2, 5, 13, 1]}
PUBLISHED_PARAMETERS = {"regnet_y_400mf": 4344144, "regnet_y_800mf": 6432512, "regnet_y_1_6gf": 11202430, "regnet_y_3_2gf": 19436338}
STATE_DICT_ENTRIES = {"regnet_y_400mf": 384, "regnet_y_800mf": 340, "regnet_y_1_6gf": 626, "regnet_y_3_2gf": 494}
# the reference's hard-coded ladders (models/semanticFCN.py:97-108)
BASE_CHANNELS = {"regnet_y_400mf": [440, 208, 104, 48, 32], "regnet_y_800mf": [784, 320, 144, 64, 32],
                 "regnet_y_1_6gf": [888, 336, 120, 48, 32], "regnet_y_3_2gf": [1512, 576, 216, 72, 32]}
ENABLED = ("regnet_y_1_6gf", "regnet_y_3_2gf")
# the two configurations of the fixtures: (meta_channel_dim, attention, multi_scale_meta)
CONFIGS = {"m6_att_msm": (6, True, True), "m3_plain": (3, False, False)}
KINDS = ("plain", "opt")      # models/semanticFCN, baselines/Reichert/semanticFCN_opt
GOLDEN = {"plain": ("regnet_y_1_6gf", "m6_att_msm"), "opt": ("regnet_y_3_2gf", "m3_plain")}
VARIANTS = ("leaky_halo", "se_half", "phase11")


def golden_name(kind):
    return f"regnet_{kind}_{GOLDEN[kind][0][len('regnet_y_'):]}"


def generate(name):
    """(stage widths, stage depths) from the published generator parameters."""
    depth, w_0, w_a, w_m, gw = PARAMS[name]
    wc = torch.arange(depth, dtype=torch.float64) * w_a + w_0
    cap = torch.round(torch.log(wc / w_0) / math.log(w_m))
    bw = (torch.round(w_0 * torch.pow(torch.tensor(w_m, dtype=torch.float64), cap) / 8) * 8).int().tolist()
    widths, depths = [], []
    for w in bw:
        if widths and widths[-1] == w:
            depths[-1] += 1
        else:
            widths.append(w)
            depths.append(1)
    fixed = []
    for w in widths:
        g = min(gw, w)
        v = max(g, int(w + g / 2) // g * g)
        fixed.append(v + g if v < 0.9 * w else v)
    return fixed, depths


# ---- the container (module form) ----
class _CNA(nn.Sequential):
    def __init__(self, cin, cout, k, stride, groups, act):
        mods = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]
        if act:
            mods.append(nn.ReLU(inplace=True))
        super().__init__(*mods)


class _SERef(nn.Module):
    def __init__(self, c, s):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(c, s, 1)
        self.fc2 = nn.Conv2d(s, c, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Sigmoid()

    def forward(self, x):
        return x * self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


class _YBlockRef(nn.Module):
    def __init__(self, win, wout, stride, gw):
        super().__init__()
        self.proj = None
        if win != wout or stride != 1:
            self.proj = _CNA(win, wout, 1, stride, 1, False)
        self.f = nn.Sequential(OrderedDict([("a", _CNA(win, wout, 1, 1, 1, True)), ("b", _CNA(wout, wout, 3, stride, wout // gw, True)),
                                            ("se", _SERef(wout, int(round(0.25 * win)))), ("c", _CNA(wout, wout, 1, 1, 1, False))]))
        self.activation = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.activation((x if self.proj is None else self.proj(x)) + self.f(x))


class RegNetYRef(nn.Module):
    def __init__(self, name, num_classes=1000):
        super().__init__()
        widths, depths = generate(name)
        gw = PARAMS[name][4]
        self.stem = _CNA(3, 32, 3, 2, 1, True)
        cur, stages = 32, []
        for i, (w, d) in enumerate(zip(widths, depths)):
            stages.append((f"block{i + 1}", nn.Sequential(OrderedDict(
                (f"block{i + 1}-{j}", _YBlockRef(cur if j == 0 else w, w, 2 if j == 0 else 1, gw)) for j in range(d)))))
            cur = w
        self.trunk_output = nn.Sequential(OrderedDict(stages))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cur, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0.0, std=math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0.0, std=0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.fc(self.avgpool(self.trunk_output(self.stem(x))).flatten(1))


def add_to_stub(models_module):
    """Give a stand-in `torchvision.models` the four regnet_y_* constructors (`pretrained` ignored); the published counts are asserted."""
    def maker(name):
        def make(*a, **k):
            net = RegNetYRef(name)
            assert sum(p.numel() for p in net.parameters()) == PUBLISHED_PARAMETERS[name]
            assert len(net.state_dict()) == STATE_DICT_ENTRIES[name]
            return net
        return make
    for name in PARAMS:
        setattr(models_module, name, maker(name))
    return models_module


# ---- the fixture ----
def he_fixture_(model, bn_seed=3, conv_seed=7, bias_seed=11, last_bn=0.25):
    """Re-draw every 4-D parameter of the model (sorted-name order) as randn * sqrt(2 / fan_in) from Generator(conv_seed) -- fan_in = Cin / groups
    kh kw of a conv, in_channels of a transposed conv --, then the SE biases (1-D parameters under `backbone.` with `.se.` in the name) as
    randn * 0.5 from Generator(bias_seed), then the BatchNorms as semanticlidarunc_amd.testing.randomize_bn_(model, bn_seed) does, then the weight
    of every block's last BatchNorm (`.f.c.1`) times `last_bn`."""
    transposed = {id(m.weight) for m in model.modules() if isinstance(m, nn.ConvTranspose2d)}
    g = torch.Generator().manual_seed(conv_seed)
    gf = torch.Generator().manual_seed(bias_seed)
    with torch.no_grad():
        params = sorted(model.named_parameters(), key=lambda kv: kv[0])
        for name, p in params:
            if p.dim() == 4:
                fan_in = p.shape[0] if id(p) in transposed else p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        for name, p in params:
            if p.dim() == 1 and name.startswith("backbone.") and ".se." in name:
                p.copy_(torch.randn(p.shape, generator=gf) * 0.5)
        gb = torch.Generator().manual_seed(bn_seed)
        for name, m in sorted(model.named_modules(), key=lambda kv: kv[0]):
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=gb) + 0.5)
                m.bias.copy_(torch.randn(c, generator=gb) * 0.1)
                m.running_mean.copy_(torch.randn(c, generator=gb) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=gb) + 0.5)
        for name, m in model.named_modules():
            if name.startswith("backbone.") and name.endswith(".f.c.1"):
                m.weight.mul_(last_bn)
    return model


def build(cls, backbone, config, num_classes, seed=0):
    """cls(...) under manual_seed(seed) with the He fixture applied, in eval mode."""
    m, att, msm = CONFIGS[config]
    torch.manual_seed(seed)
    return he_fixture_(cls(backbone=backbone, input_channels=2, meta_channel_dim=m, num_classes=num_classes, attention=att, multi_scale_meta=msm)).eval()


def inputs(config, b, h, w, seed=13):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 2, h, w, generator=g)
    meta = torch.randn(b, CONFIGS[config][0], h, w, generator=g)
    return x, meta


def sd_digest(sd):
    s = sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point())
    a = sum(float(v.double().abs().sum()) for v in sd.values() if v.is_floating_point())
    return [s, a]


# ---- functional restatement ----
def _bn_shift(sd, p):
    """bn(0) per channel."""
    return sd[p + ".bias"] - sd[p + ".running_mean"] * sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + 1e-5)


def se_gate(hb, sd, p):
    """[N, C, 1, 1] multiplier of the SqueezeExcitation at prefix p (`....f.se`)."""
    pooled = hb.mean((2, 3), keepdim=True)
    return torch.sigmoid(F.conv2d(F.relu(F.conv2d(pooled, sd[p + ".fc1.weight"], sd[p + ".fc1.bias"])), sd[p + ".fc2.weight"], sd[p + ".fc2.bias"]))


def y_block(x, sd, p, leaky_halo=False, se_half=False, phase11=False):
    """torchvision's ResBottleneckBlock.forward at prefix p; stride and groups are read off the tensors (a block has a projection exactly when it is
    the first of its stage, and that block has stride 2; groups = channels / f.b's input channels per group)."""
    has_proj = p + ".proj.0.weight" in sd
    stride = 2 if has_proj else 1
    a = F.relu(_bn(F.conv2d(x, sd[p + ".f.a.0.weight"]), sd, p + ".f.a.1"))
    wb = sd[p + ".f.b.0.weight"]
    groups = wb.shape[0] // wb.shape[1]
    if leaky_halo:
        n, c, h, w = a.shape
        ap = F.relu(_bn_shift(sd, p + ".f.a.1")).view(1, c, 1, 1).expand(n, c, h + 2, w + 2).clone()
        ap[:, :, 1:-1, 1:-1] = a
        pad = 0
    else:
        ap, pad = a, 1
    if stride == 2 and phase11:
        hb = F.conv2d(ap, wb, None, 1, pad, 1, groups)[:, :, 1::2, 1::2]
    else:
        hb = F.conv2d(ap, wb, None, stride, pad, 1, groups)
    hb = F.relu(_bn(hb, sd, p + ".f.b.1"))
    gate = torch.full_like(hb[:, :, :1, :1], 0.5) if se_half else se_gate(hb, sd, p + ".f.se")
    c = _bn(F.conv2d(hb * gate, sd[p + ".f.c.0.weight"]), sd, p + ".f.c.1")
    if has_proj:
        xs = x[:, :, 1::2, 1::2] if phase11 else x[:, :, ::2, ::2]
        idn = _bn(F.conv2d(xs, sd[p + ".proj.0.weight"]), sd, p + ".proj.1")
    else:
        idn = x
    return F.relu(idn + c)


def _stage(x, sd, i, **variant):
    j = 0
    while f"backbone.trunk_output.block{i}.block{i}-{j}.f.a.0.weight" in sd:
        x = y_block(x, sd, f"backbone.trunk_output.block{i}.block{i}-{j}", **variant)
        j += 1
    assert j > 0
    return x


def encode(sd, x, meta, multi_scale_meta=True, **variant):
    m = meta.shape[1]
    xs = F.relu(_bn(F.conv2d(torch.cat([x, meta], 1), sd["backbone.stem.0.weight"], None, padding=1), sd, "backbone.stem.1"))
    x1 = _stage(xs, sd, 1, **variant)
    if multi_scale_meta:
        m1, m2, m3 = (F.interpolate(meta, scale_factor=s, mode="nearest") for s in (1 / 2, 1 / 4, 1 / 8))
        x2 = _stage(torch.cat([x1[:, :-m], m1], 1), sd, 2, **variant)
        x3 = _stage(torch.cat([x2[:, :-m], m2], 1), sd, 3, **variant)
        x4 = _stage(torch.cat([x3[:, :-m], m3], 1), sd, 4, **variant)
    else:
        x2 = _stage(x1, sd, 2, **variant)
        x3 = _stage(x2, sd, 3, **variant)
        x4 = _stage(x3, sd, 4, **variant)
    return x1, x2, x3, x4


def fpn_forward(sd, x, meta, attention=True, multi_scale_meta=True, **variant):
    x1, x2, x3, x4 = encode(sd, x, meta, multi_scale_meta, **variant)
    f4, f3, f2, f1 = _cbr(x4, sd, "fpn_block4"), _cbr(x3, sd, "fpn_block3"), _cbr(x2, sd, "fpn_block2"), _cbr(x1, sd, "fpn_block1")
    if attention:
        f4, f3 = _attention(f4, sd, "attention4"), _attention(f3, sd, "attention3")
        f2, f1 = _attention(f2, sd, "attention2"), _attention(f1, sd, "attention1")
    u4 = F.conv_transpose2d(f4, sd["upsample_layer_x4.weight"], sd["upsample_layer_x4.bias"], stride=8)
    u3 = F.conv_transpose2d(f3, sd["upsample_layer_x3.weight"], sd["upsample_layer_x3.bias"], stride=4)
    u2 = F.conv_transpose2d(f2, sd["upsample_layer_x2.weight"], sd["upsample_layer_x2.bias"], stride=2)
    y = torch.cat([f1, u2, u3, u4], 1)
    y = F.relu(_bn(F.conv2d(y, sd["decoder_semantic.0.weight"], sd["decoder_semantic.0.bias"], padding=1), sd, "decoder_semantic.1"))
    y = F.relu(_bn(F.conv2d(y, sd["decoder_semantic.3.weight"], sd["decoder_semantic.3.bias"], padding=1), sd, "decoder_semantic.4"))
    y = F.conv_transpose2d(y, sd["decoder_semantic.6.weight"], sd["decoder_semantic.6.bias"], stride=2, padding=1)
    return F.elu(y) + 1.0


def fpn_opt_forward(sd, x, meta, attention=True, multi_scale_meta=True, dropout_scale=None, **variant):
    x1, x2, x3, x4 = encode(sd, x, meta, multi_scale_meta, **variant)
    return _opt_head(sd, x1, x2, x3, x4, attention, dropout_scale, (8, 4, 2))


def forward(kind, sd, x, meta, config, dtype=None, dropout_scale=None, **variant):
    """kind 'plain' (models/semanticFCN) or 'opt' (semanticFCN_opt); dtype torch.float64 converts the state_dict and the inputs first;
    variant: leaky_halo=True / se_half=True / phase11=True."""
    _, att, msm = CONFIGS[config]
    if dtype is not None:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        x, meta = x.to(dtype), meta.to(dtype)
        dropout_scale = None if dropout_scale is None else dropout_scale.to(dtype)
    with torch.no_grad():
        if kind == "plain":
            return fpn_forward(sd, x, meta, att, msm, **variant)
        return fpn_opt_forward(sd, x, meta, att, msm, dropout_scale, **variant)


def scale_of(y):
    return max(1.0, float(y.abs().max()))


def flips(a, b):
    return float((a.argmax(1) != b.argmax(1)).double().mean())


# ---- the fixtures the model tests share ----
def model_cases():
    """(id, kind, backbone, config, batch, H, W, classes, input seed, golden name or None): the two goldens (1 x 32 x 64, 5 classes) and, per
    class, B = 2 at 48 x 80 with fresh inputs on the other backbone and the other configuration."""
    out = []
    for kind in KINDS:
        bb, config = GOLDEN[kind]
        out.append((f"golden-{kind}-{bb[9:]}", kind, bb, config, 1, 32, 64, 5, 13, golden_name(kind)))
    out.append(("plain-3_2gf-m3_plain", "plain", "regnet_y_3_2gf", "m3_plain", 2, 48, 80, 7, 17, None))
    out.append(("opt-1_6gf-m6_att_msm", "opt", "regnet_y_1_6gf", "m6_att_msm", 2, 48, 80, 7, 17, None))
    return out


def package_class(kind):
    if kind == "plain":
        from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN
    else:
        from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN
    return SemanticNetworkWithFPN
