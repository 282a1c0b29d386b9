"""CPU: the CENet ResNet-34 containers (state_dict layout and default initialisation of the reference), the plain-torch restatement against the
goldens the reference's own classes produced, the conditions a fixture must meet before a GPU comparison on it means anything, the refusals that
need no GPU, and the C ABI of the two decoder kernels (argument checks only, nothing is launched)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import cenet_restatement as R
from conftest import GOLDEN, golden
from semanticlidarunc_amd import _lib, cenet, ops


def _model(case):
    m = R.package_model(case).eval()
    g = golden(case[0])
    assert int(g["seed"]) == case[-1]
    return m, g


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_state_dict_layout_and_default_initialisation_are_the_reference_s(case):
    m, g = _model(case)
    sd = m.state_dict()
    want = json.load(open(os.path.join(GOLDEN, R.KEYS_JSON)))[R.keys_label(case)]
    assert list(sd.keys()) == list(want.keys())
    assert all(list(v.shape) == want[k] for k, v in sd.items())
    assert np.allclose(R.sd_digest(sd), g["sd_digest"], rtol=1e-10)      # the package's container draws the reference's initialisation
    assert sum(p.numel() for p in m.parameters()) > 6.7e6


def test_import_paths_mirror_the_reference():
    from semanticlidarunc_amd.baselines.CENet.CENet import CENet
    from semanticlidarunc_amd.baselines.CENet.CENet_ResNet34 import BasicBlock, BasicConv2d, ResNet_34
    assert CENet is cenet.CENet and ResNet_34 is cenet.ResNet_34 and BasicBlock is cenet.BasicBlock and BasicConv2d is cenet.BasicConv2d
    m = ResNet_34(20)
    assert m.aux is False and not hasattr(m, "aux_head1") and m.conv1.conv.in_channels == 5
    assert isinstance(CENet(20, model="ResNet_34").model, ResNet_34) and CENet(20, model="ResNet_34").aux is True


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_restatement_reproduces_the_reference_golden(case):
    m, g = _model(case)
    R.randomise_bn(m, case[-1], float(g["gain"]))
    x = torch.from_numpy(g["x"])
    assert torch.equal(x, R.case_input(case))
    sd, aux, pre = m.state_dict(), case[4], R.prefix_of(case)
    want = R.load_outputs(g)
    y32 = R.as_list(R.forward(sd, x, aux, pre))
    y64 = R.as_list(R.forward(sd, x, aux, pre, dtype=torch.float64))
    assert len(want) == len(y32) == len(y64) == (4 if aux else 1)
    for i, (w, a, b) in enumerate(zip(want, y32, y64)):
        e32, e64 = float((a - w).abs().max()), float((b - w.double()).abs().max())
        print(f"{case[0]} map {i}: restatement fp32 - golden = {e32:.1e}, fp64 - golden = {e64:.1e}")
        assert a.shape == w.shape and e32 <= 1e-5
        assert e64 <= 1e-5 and float((b.sum(1) - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_goldens_are_neither_saturated_nor_uniform(case):
    """A saturated softmax (every pixel at probability ~1) or a uniform one would pass any parity bar: at least 20 % of the pixels of each
    returned map have a largest probability below 0.9, and the main output is above 2 / C on at least 20 %."""
    g = golden(case[0])
    outs = R.load_outputs(g)
    for o in outs:
        assert R.unsaturated_fraction(o) >= 0.2
    assert float((outs[0].max(1).values > 2.0 / case[2]).double().mean()) >= 0.2


def test_refusals_that_need_no_gpu():
    with pytest.raises(NotImplementedError, match="ResNet_34"):
        cenet.CENet(20)                                  # the reference's default variant
    with pytest.raises(NotImplementedError, match="ResNet_34"):
        cenet.CENet(20, aux=False, model="HarDNet")
    m = cenet.ResNet_34(3, input_dim=5)
    x = torch.zeros(1, 5, 8, 16)
    with pytest.raises(NotImplementedError, match="inference only"):      # train-mode BatchNorm
        with torch.no_grad():
            m(x)
    m.eval()
    with pytest.raises(NotImplementedError, match="inference only"):      # a gradient may be asked for
        m(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)
        with pytest.raises(RuntimeError, match="x\\[B, 5, H, W\\]"):
            m(torch.zeros(1, 7, 8, 16))
    with pytest.raises(NotImplementedError):
        m.conv1(x)                                       # containers have no torch forward
    with pytest.raises(NotImplementedError, match="1..32 classes"):
        cenet.ResNet_34(33)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bilinear_ac_cat([torch.zeros(1, 1, 2, 2)], (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bilinear_ac_softmax(torch.zeros(1, 3, 2, 2), (4, 4))


def test_new_symbols_are_typed_and_refuse_bad_arguments_without_a_launch():
    assert _lib.ABI_VERSION >= 45 and _lib.load().slu_abi_version() == _lib.ABI_VERSION
    lib = _lib.load()
    assert ctypes.sizeof(_lib.BilinearSrc) == 24
    for name in ("slu_bilinear_ac_cat", "slu_bilinear_ac_softmax"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    inval, unsup = -1, -2
    fake = 0x1000                                       # never dereferenced: every call below is refused on the host
    arr = (_lib.BilinearSrc * 3)()

    def src(k, c, h, w, off, ptr=fake):
        arr[k].ptr, arr[k].C, arr[k].h, arr[k].w, arr[k].c_off = ptr, c, h, w, off
    src(0, 4, 2, 2, 0), src(1, 4, 2, 2, 4), src(2, 4, 2, 2, 8)
    cat = lib.slu_bilinear_ac_cat
    assert cat(None, 1, fake, 1, 4, 4, 4, None) == inval and cat(arr, 1, None, 1, 4, 4, 4, None) == inval
    assert cat(arr, 0, fake, 1, 12, 4, 4, None) == inval and cat(arr, 4, fake, 1, 12, 4, 4, None) == inval
    assert cat(arr, 3, fake, 0, 12, 4, 4, None) == inval and cat(arr, 3, fake, 1, 12, 0, 4, None) == inval and cat(arr, 3, fake, 1, 12, 4, 0, None) == inval
    assert cat(arr, 3, fake, 1, 11, 4, 4, None) == inval                 # the last slice leaves C_tot
    src(1, 4, 2, 2, 3)
    assert cat(arr, 2, fake, 1, 12, 4, 4, None) == inval                 # slices [0, 4) and [3, 7) overlap
    src(1, 4, 2, 2, -1)
    assert cat(arr, 2, fake, 1, 12, 4, 4, None) == inval
    src(1, 4, 2, 2, 4, ptr=None)
    assert cat(arr, 2, fake, 1, 12, 4, 4, None) == inval
    src(1, 4, 0, 2, 4)
    assert cat(arr, 2, fake, 1, 12, 4, 4, None) == inval
    src(1, 4, 2, 2, 4)
    assert cat(arr, 2, fake, 8192, 8, 4, 4, None) == unsup               # N * sum C_k = 65536 planes
    src(1, 4, 2, 4, 4)
    assert cat(arr, 2, fake, 1, 8, 4, 1 << 30, None) == unsup            # (out - 1) * (in - 1) = 3 (2^30 - 1) >= 2^31
    sm = lib.slu_bilinear_ac_softmax
    assert sm(None, fake, 1, 3, 2, 2, 4, 4, None) == inval and sm(fake, None, 1, 3, 2, 2, 4, 4, None) == inval
    assert sm(fake, fake, 1, 33, 2, 2, 4, 4, None) == inval and sm(fake, fake, 1, 0, 2, 2, 4, 4, None) == inval
    assert sm(fake, fake, 0, 3, 2, 2, 4, 4, None) == inval and sm(fake, fake, 1, 3, 0, 2, 4, 4, None) == inval and sm(fake, fake, 1, 3, 2, 2, 4, 0, None) == inval
    assert sm(fake, fake, 65536, 3, 2, 2, 4, 4, None) == unsup and sm(fake, fake, 1, 3, 2, 2, 65536, 4, None) == unsup
