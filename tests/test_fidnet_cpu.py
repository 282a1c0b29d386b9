"""CPU: the FIDNet ResNet34_point containers (state_dict layout and default initialisation of the reference), the plain-torch restatement against
the goldens the reference's own class produced (logits and the backend's 1024-channel map, slice by slice), the conditions a fixture must meet
before a GPU comparison on it means anything, the refusals that need no GPU, and the C ABI of the three new entry points (argument checks only,
nothing is launched)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fidnet_restatement as R
from conftest import GOLDEN, golden
from semanticlidarunc_amd import _lib, fidnet, ops


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
    assert np.allclose(R.sd_digest(sd), g["sd_digest"], rtol=1e-10)      # the package's containers draw the reference's initialisation
    assert m.model.backend.conv1.in_channels == case[3][1] and sum(p.numel() for p in m.parameters()) > 6.0e6


def test_the_four_conv1_input_widths_exist():
    for (rem, rng, nrm), cin in (((False, False, False), 3), ((True, False, False), 4), ((True, True, False), 5), ((True, True, True), 8)):
        assert fidnet.resnet34_point(True, rem, rng, nrm).conv1.in_channels == cin
    with pytest.raises(ValueError, match="conv1"):
        fidnet.resnet34_point(True, False, True, False)


def test_import_paths_mirror_the_reference():
    from semanticlidarunc_amd.baselines.FIDNet.FIDNet import FIDNet
    from semanticlidarunc_amd.baselines.FIDNet.ResNet import BasicBlock, Final_Model, ResNet_34_point, SemanticHead, resnet34_point
    assert FIDNet is fidnet.FIDNet and ResNet_34_point is fidnet.ResNet_34_point and BasicBlock is fidnet.BasicBlock
    assert Final_Model is fidnet.Final_Model and SemanticHead is fidnet.SemanticHead and resnet34_point is fidnet.resnet34_point
    m = FIDNet(20, "ResNet34_point")
    assert isinstance(m.model, Final_Model) and isinstance(m.model.backend, ResNet_34_point) and isinstance(m.model.semantic_head, SemanticHead)
    assert m.model.semantic_head.conv_1.in_channels == 1024 and m.model.backend.layer1[0].downsample[0].in_channels == 512


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_restatement_reproduces_the_reference_golden(case):
    m, g = _model(case)
    R.randomise_bn(m, case[-1], float(g["gain"]))
    x = torch.from_numpy(g["x"])
    assert torch.equal(x, R.case_input(case))
    sd = m.state_dict()
    want = torch.from_numpy(g["logits"])
    scale = float(want.abs().max())
    y32, mid32 = R.forward(sd, x, want_backend=True)
    y64, mid64 = R.forward(sd, x, dtype=torch.float64, want_backend=True)
    e32, e64 = float((y32 - want).abs().max()), float((y64 - want.double()).abs().max())
    print(f"{case[0]}: scale {scale:.3g}, restatement fp32 - golden = {e32:.1e}, fp64 - golden = {e64:.1e}")
    assert y32.shape == want.shape and e32 <= 1e-5 * scale and e64 <= 1e-5 * scale
    sums, samples = R.backend_digest(mid32)             # the fp32 restatement: every stored number at rtol 1e-5
    assert mid32.shape[1] == 1024
    assert np.allclose(sums, g["backend_sums"], rtol=1e-5, atol=0) and np.allclose(samples, g["backend_samples"], rtol=1e-5, atol=0)
    # the fp64 restatement differs from the fp32 reference by fp32 rounding, which a signed sum or a sample near 0 does not scale down with
    # itself: the abs-sums at rtol 1e-5, the rest to 1e-5 of its slice's magnitude
    sums, samples = R.backend_digest(mid64)
    assert np.allclose(sums[:, 1], g["backend_sums"][:, 1], rtol=1e-5, atol=0)
    assert bool((np.abs(sums[:, 0] - g["backend_sums"][:, 0]) <= 1e-5 * g["backend_sums"][:, 1]).all())
    assert bool((np.abs(samples - g["backend_samples"]) <= 1e-5 * np.abs(g["backend_samples"]).max(1, keepdims=True)).all())


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_goldens_meet_the_gain_conditions(case):
    """Logits far above 20 are one class everywhere and logits that do not vary over the pixels would pass any parity bar: 1 <= max|logit| <= 20
    and some logit is at least a quarter of that away from its class's mean over the pixels; the stored gain is the first of GAINS that does."""
    g = golden(case[0])
    logits = torch.from_numpy(g["logits"])
    scale, dev = R.gain_conditions(logits)
    assert 1.0 <= scale <= 20.0 and dev >= 0.25 * scale and R.gain_ok(logits)
    assert float(g["gain"]) in R.GAINS and g["backend_samples"].shape == (len(R.SLICES), R.N_SAMPLE)


def test_refusals_that_need_no_gpu():
    for backbone in ("ResNet34_aspp_1", "ResNet34_aspp_2"):
        with pytest.raises(NotImplementedError, match="ResNet34_point"):
            fidnet.FIDNet(20, backbone)
    with pytest.raises(NotImplementedError, match="ResNet34_point"):
        fidnet.FIDNet(20)                                # the reference's default backbone
    with pytest.raises(ValueError, match="ResNet34_point"):
        fidnet.FIDNet(20, "ResNet50")
    m = fidnet.FIDNet(3, "ResNet34_point")
    x = torch.zeros(1, 5, 8, 16)
    for f in (m, m.model.backend, lambda t: m.model.semantic_head(torch.zeros(1, 1024, 8, 16))):
        with pytest.raises(NotImplementedError, match="inference only"):      # train-mode BatchNorm
            with torch.no_grad():
                f(x)
    m.eval()
    for f in (m, m.model.backend, lambda t: m.model.semantic_head(torch.zeros(1, 1024, 8, 16))):
        with pytest.raises(NotImplementedError, match="inference only"):      # a gradient may be asked for
            f(x)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="x\\[B, 5, H, W\\]"):
            m(torch.zeros(1, 8, 8, 16))
        with pytest.raises(RuntimeError, match="x\\[B, 1024, H, W\\]"):
            m.model.semantic_head(torch.zeros(1, 640, 8, 16))
    with pytest.raises(NotImplementedError):
        m.model.backend.layer1[0](x)                     # BasicBlock has no torch forward
    assert fidnet.FIDNet(40, "ResNet34_point").model.semantic_head.semantic_output.out_channels == 40      # no class limit: the head is a conv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bilinear_ac_sum([torch.zeros(1, 1, 2, 2)], (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_point_mlp([torch.zeros(32, 5)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.point_mlp(torch.zeros(1, 5, 2, 2), torch.zeros(1), torch.zeros(32), [32], 0.01)


def test_new_symbols_are_typed_and_refuse_bad_arguments_without_a_launch():
    assert _lib.ABI_VERSION >= 46 and _lib.load().slu_abi_version() == _lib.ABI_VERSION
    lib = _lib.load()
    for name in ("slu_point_mlp_pack", "slu_point_mlp", "slu_bilinear_ac_sum"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    inval, unsup = -1, -2
    fake = 0x1000                                       # never dereferenced: every call below is refused on the host
    assert ops.point_mlp_packed_floats(64, 5) == 2 * 8 * 64 and ops.point_mlp_packed_floats(512, 256) == 16 * 128 * 64

    pack = lib.slu_point_mlp_pack
    assert pack(None, 32, 5, fake, None) == inval and pack(fake, 32, 5, None, None) == inval
    assert pack(fake, 0, 5, fake, None) == inval and pack(fake, 32, 0, fake, None) == inval
    assert pack(fake, 48, 5, fake, None) == unsup and pack(fake, 544, 5, fake, None) == unsup and pack(fake, 32, 513, fake, None) == unsup

    def mlp(x=fake, w=fake, b=fake, widths=(64, 128, 256, 512), nl=None, n=1, c0=5, hw=64, out=fake, no_widths=False):
        arr = (ctypes.c_int * max(1, len(widths)))(*widths)
        return lib.slu_point_mlp(x, w, b, None if no_widths else arr, len(widths) if nl is None else nl, n, c0, hw, 0.01, 1, out, None)
    assert mlp(x=None) == inval and mlp(w=None) == inval and mlp(b=None) == inval and mlp(out=None) == inval and mlp(no_widths=True) == inval
    assert mlp(widths=(32,), nl=0) == inval and mlp(widths=(32, 32, 32, 32, 32)) == inval
    assert mlp(n=0) == inval and mlp(c0=0) == inval and mlp(hw=0) == inval and mlp(widths=(64, 0)) == inval and mlp(widths=(64, -32)) == inval
    assert mlp(c0=33) == unsup and mlp(widths=(64, 48)) == unsup and mlp(widths=(544,)) == unsup
    assert mlp(n=65536) == unsup and mlp(hw=2 ** 31 - 1) == unsup

    arr = (_lib.BilinearSrc * 3)()

    def src(k, c, h, w, off=0, ptr=fake):
        arr[k].ptr, arr[k].C, arr[k].h, arr[k].w, arr[k].c_off = ptr, c, h, w, off
    src(0, 4, 2, 2), src(1, 4, 1, 2), src(2, 4, 4, 4)
    acs = lib.slu_bilinear_ac_sum
    assert acs(None, 1, fake, 1, 4, 4, 4, None) == inval and acs(arr, 1, None, 1, 4, 4, 4, None) == inval
    assert acs(arr, 0, fake, 1, 4, 4, 4, None) == inval and acs(arr, 4, fake, 1, 4, 4, 4, None) == inval
    assert acs(arr, 3, fake, 0, 4, 4, 4, None) == inval and acs(arr, 3, fake, 1, 0, 4, 4, None) == inval
    assert acs(arr, 3, fake, 1, 4, 0, 4, None) == inval and acs(arr, 3, fake, 1, 4, 4, 0, None) == inval
    assert acs(arr, 3, fake, 1, 5, 4, 4, None) == inval                  # the sources have 4 channels
    src(1, 3, 1, 2)
    assert acs(arr, 2, fake, 1, 4, 4, 4, None) == inval                  # channel mismatch between sources
    src(1, 4, 1, 2, off=4)
    assert acs(arr, 2, fake, 1, 4, 4, 4, None) == inval                  # a sum has no channel offsets
    src(1, 4, 1, 2, ptr=None)
    assert acs(arr, 2, fake, 1, 4, 4, 4, None) == inval
    src(1, 4, 0, 2)
    assert acs(arr, 2, fake, 1, 4, 4, 4, None) == inval
    src(1, 4, 1, 2)
    assert acs(arr, 2, fake, 16384, 4, 4, 4, None) == unsup              # N * C = 65536 planes
    src(1, 4, 2, 4)
    assert acs(arr, 2, fake, 1, 4, 4, 1 << 30, None) == unsup            # (out - 1) * (in - 1) = 3 (2^30 - 1) >= 2^31
