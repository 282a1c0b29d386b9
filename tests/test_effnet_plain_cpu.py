"""CPU: `models/semanticFCN` on the EfficientNetV2 encoders -- the fp64 restatement against the golden the reference's own class produced, the
state_dict layout, the constructor contract, the C ABI of the fused depthwise + SE kernels (nothing here launches a kernel), and the conditions a
fixture must meet before the GPU comparison on it (tests/test_gpu_effnet_plain.py) means anything."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import effnet_plain_restatement as R
from conftest import GOLDEN, ROOT, golden
from semanticlidarunc_amd import _lib, effnet as eff, ops

CASES = R.model_cases()
NEW = ("slu_dwconv3x3_se_fwd", "slu_dwconv3x3_se_tiles", "slu_se_gate_psum")
PTR = 0x10000          # non-null, 16-byte aligned; a refused call never dereferences it


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_restatement_reproduces_the_reference_golden():
    g = golden(R.GOLDEN_NAME)
    backbone, config = R.GOLDEN
    model = R.build(R.package_class(), backbone, config, R.GOLDEN_CLASSES)
    sd = model.state_dict()
    assert np.allclose(R.sd_digest(sd), g["sd_digest"], rtol=1e-10)
    assert g["x"].shape == (1, 2, 32, 64) and g["meta"].shape == (1, 6, 32, 64)
    got = R.forward(sd, _t(g["x"]), _t(g["meta"]), backbone, config, dtype=torch.float64)
    want = _t(g["out"]).double()
    s = R.scale_of(want)
    err = float((got - want).abs().max())
    print(f"{backbone} {config}: S = {s:.3g}, restatement (fp64) - golden (stored fp32) = {err:.2e}")
    assert got.shape == want.shape == (1, R.GOLDEN_CLASSES, 32, 64)
    assert err <= 1e-6 * s


def test_state_dict_keys_and_shapes_equal_the_reference_class():
    backbone, config = R.GOLDEN
    m = R.package_class()(backbone=backbone, input_channels=2, meta_channel_dim=R.CONFIGS[config][0], num_classes=R.GOLDEN_CLASSES)
    sd = m.state_dict()
    want = json.load(open(os.path.join(GOLDEN, R.GOLDEN_KEYS)))
    assert list(sd.keys()) == list(want.keys())
    assert all(list(v.shape) == want[k] for k, v in sd.items())
    # layer4 = features[6:] is a slice of a Sequential: it keeps the children's names, so its aliases are layer4.6.* / layer4.7.* in the reference too
    assert sd["layer4.6.0.block.0.0.weight"].data_ptr() == sd["backbone.features.6.0.block.0.0.weight"].data_ptr()
    assert sd["layer4.7.0.weight"].data_ptr() == sd["backbone.features.7.0.weight"].data_ptr()
    assert not any(k.startswith(("layer4.0.", "layer4.1.")) for k in sd)
    assert sd["stem.0.weight"].data_ptr() == sd["backbone.features.0.0.weight"].data_ptr()
    assert sd["layer3.0.block.2.fc1.bias"].data_ptr() == sd["backbone.features.4.0.block.2.fc1.bias"].data_ptr()
    assert "backbone.classifier.1.weight" in sd and "backbone.features.1.0.block.0.0.weight" in sd and "backbone.features.5.0.block.0.0.weight" in sd


@pytest.mark.parametrize("backbone", R.NAMES)
def test_constructor_contract(backbone):
    cls = R.package_class()
    m = cls(backbone=backbone, input_channels=2, meta_channel_dim=3, num_classes=7)
    assert m.is_effnet and not m.is_shuffle and not m.is_squeeze and not m.is_regnet and m.backbone_name == backbone
    assert isinstance(m.backbone, eff.EfficientNetContainer)
    assert sum(p.numel() for p in eff.EfficientNetContainer(backbone).parameters()) == R.PUBLISHED_PARAMETERS[backbone]
    f = m.backbone.features
    assert m.stem is f[0] and m.layer1 is f[2] and m.layer2 is f[3] and m.layer3 is f[4]
    assert len(m.layer4) == len(f) - 6 and all(a is b for a, b in zip(m.layer4, list(f)[6:]))
    c = m.stem[0]
    assert (c.in_channels, c.out_channels, c.stride, c.kernel_size, c.padding) == (5, eff.stage_channels(backbone)[0], (1, 1), (3, 3), (1, 1)) and c.bias is None
    assert isinstance(m.stem[1], nn.BatchNorm2d) and m.stem[1].eps == 1e-3 and isinstance(m.stem[2], nn.SiLU)
    bc = R.BASE_CHANNELS[backbone]
    assert eff.BASE_CHANNELS[backbone] == bc and bc[0] == eff.stage_channels(backbone)[3]
    assert [b[0].in_channels for b in (m.fpn_block4, m.fpn_block3, m.fpn_block2, m.fpn_block1)] == bc[:4]
    ups = [(u.in_channels, u.out_channels, u.kernel_size, u.stride) for u in (m.upsample_layer_x4, m.upsample_layer_x3, m.upsample_layer_x2)]
    assert ups == [(bc[1], bc[1] // 4, (4, 4), (4, 4)), (bc[2], bc[2] // 4, (4, 4), (4, 4)), (bc[3], bc[3] // 2, (2, 2), (2, 2))]
    assert m.decoder_semantic[0].in_channels == bc[1] // 4 + bc[2] // 4 + bc[3] // 2 + bc[4] and m.decoder_semantic[6].out_channels == 7
    assert sum(isinstance(b, eff.MBConv) for b in m.layer3) == len(m.layer3) == R.MBCONV_BLOCKS[backbone]
    assert all(isinstance(b, eff.FusedMBConv) for b in list(m.layer1) + list(m.layer2))
    alias = cls(resnet_type=backbone, meta_channel_dim=3, num_classes=3)            # the stale keyword of inference_ouster.py
    assert alias.backbone_name == backbone and alias.is_effnet


def test_the_new_symbols_are_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slu.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/slu.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.ABI_VERSION >= 42 and _lib.load().slu_abi_version() == _lib.ABI_VERSION
    assert callable(ops.dwconv3x3_se) and callable(ops.se_gate_psum) and callable(eff.block_forward)


def test_null_and_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    ok = (PTR, PTR, PTR, PTR, PTR)
    for i in range(5):                                                                         # each pointer in turn
        args = list(ok)
        args[i] = None
        assert lib.slu_dwconv3x3_se_fwd(*args, 1, 2, 8, 8, 1, None) == -1, i
    for n, c, h, w, stride in ((0, 2, 8, 8, 1), (1, 0, 8, 8, 1), (1, 2, 0, 8, 1), (1, 2, 8, -1, 2), (1, 2, 8, 8, 0), (1, 2, 8, 8, 3)):
        assert lib.slu_dwconv3x3_se_fwd(*ok, n, c, h, w, stride, None) == -1, (n, c, h, w, stride)
    assert lib.slu_dwconv3x3_se_tiles(0, 8, 1) == 0 and lib.slu_dwconv3x3_se_tiles(8, 8, 3) == 0 and lib.slu_dwconv3x3_se_tiles(8, 0, 2) == 0
    # a tile is a run of whole output rows of about 2048 outputs: the 8 x 256 plane of the judged shapes is one tile at both strides
    assert lib.slu_dwconv3x3_se_tiles(8, 256, 1) == 1 and lib.slu_dwconv3x3_se_tiles(16, 512, 2) == 1
    assert lib.slu_dwconv3x3_se_tiles(32, 512, 2) == 2 and lib.slu_dwconv3x3_se_tiles(16, 256, 1) == 2
    assert lib.slu_dwconv3x3_se_tiles(1, 1, 1) == 1 and lib.slu_dwconv3x3_se_tiles(37, 132, 1) == 3 and lib.slu_dwconv3x3_se_tiles(33, 257, 2) == 2
    gate_ok = (PTR, 1, 1.0, PTR, PTR, PTR, PTR, PTR)
    for i in (0, 3, 4, 5, 6, 7):
        args = list(gate_ok)
        args[i] = None
        assert lib.slu_se_gate_psum(*args, 1, 8, 2, None) == -1, i
    assert lib.slu_se_gate_psum(PTR, 0, 1.0, PTR, PTR, PTR, PTR, PTR, 1, 8, 2, None) == -1     # T = 0
    for n, c, s in ((0, 8, 2), (1, 0, 2), (1, 8, 0), (1, 1537, 96), (1, 1536, 97)):            # sizes; outside slu_se_gate's range
        assert lib.slu_se_gate_psum(*gate_ok, n, c, s, None) == -1, (n, c, s)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fixture_conditions(case):
    """Conditions, not measurements, on the restatement alone: on every fixture of the GPU model test the reference's arithmetic in fp32 stays inside
    the caps the GPU test applies (err <= 1e-3 S, argmax flips <= 1e-3 of the pixels) with a margin of ten on the error, and the output reacts
    to the SqueezeExcitation (gates of 0.5 instead of the computed ones) and to the meta channels."""
    _, backbone, config, b, h, w, classes, seed, gname = case
    sd = R.build(R.package_class(), backbone, config, classes).state_dict()
    if gname is None:
        x, meta = R.inputs(config, b, h, w, seed)
    else:
        g = golden(gname)
        x, meta = _t(g["x"]), _t(g["meta"])
    y64 = R.forward(sd, x, meta, backbone, config, dtype=torch.float64)
    y32 = R.forward(sd, x, meta, backbone, config).double()
    s = R.scale_of(y64)
    e32 = float((y32 - y64).abs().max())
    fl = R.flips(y32, y64)
    flat = {k: (torch.zeros_like(v) if k.startswith("backbone.features.4.") and k.endswith((".fc2.weight", ".fc2.bias")) else v) for k, v in sd.items()}
    d_se = float((R.forward(flat, x, meta, backbone, config, dtype=torch.float64) - y64).abs().max())
    d_meta = float((R.forward(sd, x, torch.zeros_like(meta), backbone, config, dtype=torch.float64) - y64).abs().max())
    print(f"{case[0]}: S = {s:.3g}, fp32 - fp64 = {e32 / s:.1e} S with {fl:.1e} flips, gates 0.5 {d_se / s:.3f} S, no meta {d_meta / s:.2f} S")
    assert y64.shape == (b, classes, h, w) and bool(torch.isfinite(y64).all())
    assert e32 <= 1e-4 * s and fl <= 1e-3
    assert d_se >= 0.01 * s and d_meta >= 0.1 * s
