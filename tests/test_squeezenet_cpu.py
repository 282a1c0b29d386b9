"""CPU: the SqueezeNet 1.0 backbone container, the construction of both FPN classes on it, the fp64 restatement against the goldens the
reference's own classes produced, and the conditions a fixture must meet before a GPU comparison on it means anything."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import squeezenet_restatement as R
from conftest import GOLDEN, golden
from semanticlidarunc_amd import squeezenet as sqz

CASES = R.model_cases()


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_container_has_the_published_parameter_count():
    net = sqz.SqueezeNetContainer("squeezenet1_0")
    n = sum(p.numel() for p in net.parameters())
    assert n == R.PUBLISHED_PARAMETERS == sqz.PARAMETER_COUNTS["squeezenet1_0"] == 1248424
    assert sqz.BASE_CHANNELS["squeezenet1_0"] == [512, 384, 256, 256, 112]
    assert list(net.state_dict().keys()) == list(R.SqueezeNetRef().state_dict().keys())
    assert "classifier.1.weight" in net.state_dict() and "classifier.1.bias" in net.state_dict()
    for i, f in R.FEATURES.items():
        mod = net.features[i]
        if f == "M":
            assert isinstance(mod, nn.MaxPool2d) and mod.ceil_mode and mod.padding == 0 and mod.kernel_size == 3 and mod.stride == 2
        else:
            assert (mod.squeeze.in_channels, mod.squeeze.out_channels, mod.expand1x1.out_channels, mod.expand3x3.out_channels) == f
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in net.modules() if isinstance(m, nn.Conv2d))      # torchvision's initialisation
    assert 0.005 < float(net.classifier[1].weight.detach().std()) < 0.02


@pytest.mark.parametrize("kind", R.KINDS)
def test_both_classes_are_built_with_the_reference_state_dict_layout(kind):
    cls = R.package_class(kind)
    md = R.CONFIGS[R.GOLDEN_CONFIG[kind]][0]          # the key lists were written from the golden models
    m = cls(backbone="squeezenet1_0", input_channels=2, meta_channel_dim=md, num_classes=5)
    sd = m.state_dict()
    assert len(sd) == R.STATE_DICT_KEYS[kind] == (182 if kind == "plain" else 156)
    want = json.load(open(os.path.join(GOLDEN, f"squeezenet_{kind}_state_dict_keys.json")))
    assert list(sd.keys()) == list(want.keys())
    assert all(list(v.shape) == want[k] for k, v in sd.items())
    # stem / layerN are slices of backbone.features: the same modules under both names (a slice keeps the indices as names)
    f = m.backbone.features
    assert m.is_squeeze and m.backbone_name == "squeezenet1_0" and isinstance(m.backbone, sqz.SqueezeNetContainer)
    assert len(m.stem) == 4 and all(a is b for a, b in zip(m.stem, f[0:4]))
    assert [len(m.layer1), len(m.layer2), len(m.layer3), len(m.layer4)] == [2, 2, 2, 3]
    assert m.layer1[0] is f[4] and m.layer2[0] is f[6] and m.layer2[1] is f[7] and m.layer3[0] is f[8] and m.layer4[0] is f[10] and m.layer4[2] is f[12]
    assert sd["stem.0.weight"].data_ptr() == sd["backbone.features.0.weight"].data_ptr()
    assert sd["layer3.9.expand3x3.bias"].data_ptr() == sd["backbone.features.9.expand3x3.bias"].data_ptr()
    assert f[0].in_channels == 2 + md and f[0].out_channels == 96 and f[0].stride == (1, 1) and f[0].kernel_size == (3, 3) and f[0].bias is None
    if kind == "plain":
        ups = [(u.in_channels, u.out_channels, u.kernel_size, u.stride) for u in (m.upsample_layer_x4, m.upsample_layer_x3, m.upsample_layer_x2)]
        assert ups == [(384, 96, (4, 4), (4, 4)), (256, 128, (2, 2), (2, 2)), (256, 128, (2, 2), (2, 2))]
    else:
        ups = [(u.block[0].in_channels, u.block[0].out_channels, u.scale) for u in (m.upsample_layer_x4, m.upsample_layer_x3, m.upsample_layer_x2)]
        assert ups == [(384, 96, 4), (256, 128, 2), (256, 128, 2)]


def test_the_stale_resnet_type_keyword_is_honoured():
    from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN
    m = SemanticNetworkWithFPN(resnet_type="squeezenet1_0", meta_channel_dim=3, num_classes=3)
    assert m.backbone_name == "squeezenet1_0" and isinstance(m.backbone, sqz.SqueezeNetContainer)
    with pytest.raises(NotImplementedError, match="squeezenet1_0 are"):
        SemanticNetworkWithFPN(backbone="regnet_y_400mf")
    from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN as Opt
    with pytest.raises(NotImplementedError, match="squeezenet1_0 are"):
        Opt(backbone="regnet_y_800mf")


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_reproduces_the_reference_golden(kind):
    g = golden(R.golden_name(kind))
    config = R.GOLDEN_CONFIG[kind]
    model = R.build(R.package_class(kind), config, 5)
    sd = model.state_dict()
    assert np.allclose(R.sd_digest(sd), g["sd_digest"], rtol=1e-10)      # the package's container draws the reference's initialisation
    got = R.forward(kind, sd, _t(g["x"]), _t(g["meta"]), config, dtype=torch.float64)
    want = _t(g["out"]).double()
    s = R.scale_of(want)
    err = float((got - want).abs().max())
    print(f"{kind} {config}: S = {s:.3g}, restatement (fp64) - golden (stored fp32) = {err:.2e}")
    assert err <= 1e-6 * s


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixture_conditions(case):
    """Conditions, not measurements, on the restatement alone: a fixture of the GPU model test must have a bounded output scale, be stable in
    fp32, and react to a leaky halo by at least a hundredth and to the padded pool and to zeroed meta channels by at least a tenth of its
    output scale."""
    _, kind, config, b, h, w, classes, seed, gname = case
    sd = R.build(R.package_class(kind), config, classes).state_dict()
    if gname is None:
        x, meta = R.inputs(config, b, h, w, seed)
    else:
        g = golden(gname)
        x, meta = _t(g["x"]), _t(g["meta"])
    y64 = R.forward(kind, sd, x, meta, config, dtype=torch.float64)
    y32 = R.forward(kind, sd, x, meta, config).double()
    s = R.scale_of(y64)
    e32 = float((y32 - y64).abs().max())
    nflip = int((y32.argmax(1) != y64.argmax(1)).sum())
    d_halo = float((R.forward(kind, sd, x, meta, config, dtype=torch.float64, leaky_halo=True) - y64).abs().max())
    d_pool = float((R.forward(kind, sd, x, meta, config, dtype=torch.float64, pool311=True) - y64).abs().max())
    d_meta = float((R.forward(kind, sd, x, torch.zeros_like(meta), config, dtype=torch.float64) - y64).abs().max())
    print(f"{case[0]}: S = {s:.3g}, fp32 - fp64 = {e32 / s:.1e} S with {nflip} flips, leaky halo {d_halo / s:.3f} S, pool311 {d_pool / s:.2f} S, "
          f"no meta {d_meta / s:.2f} S")
    assert s <= 100
    assert e32 <= 1e-4 * s and nflip <= 1
    assert d_halo >= 0.01 * s
    assert d_pool >= 0.1 * s
    assert d_meta >= 0.1 * s
