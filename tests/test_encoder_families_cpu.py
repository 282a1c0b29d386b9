"""CPU: the encoder-family table both FPN classes read (semanticlidarunc_amd/encoder_family.py, fpn.FAMILIES, fpn.family_of): every accepted
backbone has exactly one family, every refused one is still refused with the same exception, the module trees are the committed key lists, and
the `is_*` chains have not grown back in fpn.py / fpn_opt.py."""
import json
import os
import re

import pytest

from conftest import GOLDEN
from semanticlidarunc_amd import effnet, fpn, fpn_opt, regnet, shufflenet, squeezenet

CLASSES = {"plain": fpn.SemanticNetworkWithFPN, "opt": fpn_opt.SemanticNetworkWithFPN}
ACCEPTED = (["resnet18", "resnet34", "resnet50"] + list(shufflenet.BASE_CHANNELS) + list(squeezenet.BASE_CHANNELS) + list(regnet.ENABLED)
            + list(effnet.BASE_CHANNELS))
# (class, backbone) -> golden key list: one backbone per family and class
KEYS = {("plain", "resnet18"): "fpn_resnet18", ("opt", "resnet18"): "fpn_opt_resnet18",
        ("plain", "shufflenet_v2_x0_5"): "shufflenet_plain_x0_5", ("opt", "shufflenet_v2_x0_5"): "shufflenet_opt_x0_5",
        ("plain", "squeezenet1_0"): "squeezenet_plain", ("opt", "squeezenet1_0"): "squeezenet_opt",
        ("plain", "regnet_y_1_6gf"): "regnet_plain_1_6gf", ("opt", "regnet_y_3_2gf"): "regnet_opt_3_2gf",
        ("plain", "efficientnet_v2_s"): "effnet_plain_v2_s", ("opt", "efficientnet_v2_s"): "fpn_opt_efficientnet_v2_s"}


def test_every_accepted_backbone_has_exactly_one_family():
    assert len(fpn.FAMILIES) == 5 and len(ACCEPTED) == 13
    for name in ACCEPTED:
        owners = [fam for fam in fpn.FAMILIES if name in fam.backbones]
        assert len(owners) == 1 and fpn.family_of(name) is owners[0], name
    assert sorted(n for fam in fpn.FAMILIES for n in fam.backbones) == sorted(ACCEPTED)      # and nothing else is accepted
    assert [fam.head_scales for fam in fpn.FAMILIES] == [(8, 4, 2), (4, 4, 2), (4, 2, 2), (8, 4, 2), (4, 4, 2)]
    assert [fam.trains_in_opt for fam in fpn.FAMILIES] == [True, False, False, False, True]
    assert [fam.mc_shared_prefix for fam in fpn.FAMILIES] == [True, False, False, False, True]
    assert [fam.training_refuses for fam in fpn.FAMILIES if fam.inference_clause] == [False, True, True, True]
    assert fpn.RESNET_FAMILY.inference_clause is None


@pytest.mark.parametrize("kind", sorted(CLASSES))
def test_refused_names_are_still_refused(kind):
    cls = CLASSES[kind]
    for name in ("regnet_y_400mf", "regnet_y_800mf"):
        assert fpn.family_of(name) is None
        with pytest.raises(NotImplementedError, match="squeezenet1_0 are"):
            cls(backbone=name)
    for name in ("resnet19", "vgg", "efficientnet_v2_xl", "squeezenet1_1", None):
        assert fpn.family_of(name) is None
        with pytest.raises(ValueError, match="Invalid ResNet type. Supported types: 'resnet18'"):
            cls(backbone=name)
    with pytest.raises(NotImplementedError, match="interpolation_mode='nearest'"):
        cls(backbone="resnet18", interpolation_mode="bilinear")


@pytest.mark.parametrize("kind,backbone", sorted(KEYS), ids=[f"{k}-{b}" for k, b in sorted(KEYS)])
def test_state_dict_keys_are_the_committed_lists(kind, backbone):
    m = CLASSES[kind](backbone=backbone, input_channels=2, meta_channel_dim=3, num_classes=5)
    want = json.load(open(os.path.join(GOLDEN, KEYS[(kind, backbone)] + "_state_dict_keys.json")))
    assert list(m.state_dict().keys()) == list(want.keys())
    fam = fpn.family_of(backbone)
    assert m.family is fam and m.backbone_name == backbone
    assert (m.is_shuffle, m.is_squeeze, m.is_regnet, m.is_effnet) == tuple(fam is f for f in fpn.FAMILIES[1:])
    scales = [m.upsample_layer_x4, m.upsample_layer_x3, m.upsample_layer_x2]
    assert tuple(u.scale if kind == "opt" else u.stride[0] for u in scales) == fam.head_scales


def test_no_flag_chains_in_the_fpn_classes():
    for mod in (fpn, fpn_opt):
        src = open(mod.__file__).read()
        assert not re.search(r"\b(el)?if (not )?self\.is_", src), mod.__name__
