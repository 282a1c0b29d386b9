"""GPU: `models/semanticFCN` on the efficientnet_v2_s / _m / _l encoders against the fp64 restatement (tests/effnet_plain_restatement.py) and the
golden of the reference's own class.

Bars (those of test_gpu_regnet.py): err <= 1e-3 S and at most 1e-3 of the pixels with another argmax, S = max(1, max|want|), under 'fp32' and
'f16x3'.  The flip cap is a condition: the CPU fp32 run of the restatement is within 6e-7 S and flips no pixel on these fixtures
(test_effnet_plain_cpu.py::test_fixture_conditions)."""
import copy

import numpy as np
import pytest
import torch

import effnet_plain_restatement as R
from conftest import golden
from semanticlidarunc_amd import _lib, ops, salsanext as sn

pytestmark = pytest.mark.gpu

CASES = R.model_cases()
_REFERENCE = {}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _case(case):
    """(model on the CPU, x, meta, fp64 restatement output), computed once per case."""
    if case[0] not in _REFERENCE:
        _, backbone, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(), backbone, config, classes)
        if gname is None:
            x, meta = R.inputs(config, b, h, w, seed)
        else:
            g = golden(gname)
            assert np.allclose(R.sd_digest(model.state_dict()), g["sd_digest"], rtol=1e-10)
            x, meta = _t(g["x"]), _t(g["meta"])
        want = R.forward(model.state_dict(), x, meta, backbone, config, dtype=torch.float64)
        if gname is not None:      # the reference's own class produced the golden; the restatement agrees with it (test_effnet_plain_cpu.py)
            assert float((want - _t(golden(gname)["out"]).double()).abs().max()) <= 1e-6 * R.scale_of(want)
        _REFERENCE[case[0]] = (model, x, meta, want)
    return _REFERENCE[case[0]]


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_models_against_the_fp64_restatement(cuda, case, prec):
    """'f16x3': split-fp16 products in the dense convs (stem, 3x3 and 1x1 convs of the blocks, FPN blocks, head); the depthwise convs stay exact
    fp32.  The same bar."""
    model, x, meta, want = _case(case)
    m = copy.deepcopy(model).to(cuda)
    sn.set_conv_precision(prec)
    try:
        with torch.no_grad():
            y = m(x.to(cuda), meta.to(cuda)).cpu()
    finally:
        sn.set_conv_precision("fp32")
    assert y.shape == want.shape
    s = R.scale_of(want)
    err = float((y.double() - want).abs().max()) / s
    fl = R.flips(y, want)
    print(f"{case[0]} {prec}: S = {s:.3g}, err = {err:.2e} S, flips = {fl:.2e}")
    assert err <= 1e-3 and fl <= 1e-3


def test_the_fused_route_is_the_route_and_the_caches_follow_the_parameters(cuda, monkeypatch):
    case = CASES[0]
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    lib = _lib.load()
    counts = {"dw": 0, "gate": 0}
    real = {"dw": lib.slu_dwconv3x3_se_fwd, "gate": lib.slu_se_gate_psum}

    def counted(key):
        def f(*a):
            counts[key] += 1
            return real[key](*a)
        return f

    def boom(*a, **k):
        raise AssertionError("the composed route was taken")
    monkeypatch.setattr(lib, "slu_dwconv3x3_se_fwd", counted("dw"))
    monkeypatch.setattr(lib, "slu_se_gate_psum", counted("gate"))
    monkeypatch.setattr(ops, "dwconv3x3", boom)
    monkeypatch.setattr(ops, "global_avgpool", boom)
    monkeypatch.setattr(ops, "se_scale", boom)
    blocks = R.MBCONV_BLOCKS[case[1]]
    with torch.no_grad():
        y0 = m(xd, md)
        assert counts == {"dw": blocks, "gate": blocks}                     # once per MBConv
        m.layer3[1].block[1][1].weight.mul_(1.5)                            # a depthwise BatchNorm weight, in place: the folded cache must notice
        y1 = m(xd, md)
        m.layer3[2].block[2].fc2.bias.add_(0.5)                             # an SE bias: read in place, no cache to follow
        y2 = m(xd, md)
        m.layer3[0].block[3][0].weight.mul_(1.25)                           # a projection weight: the packed 1x1 cache
        y3 = m(xd, md)
    assert counts == {"dw": 4 * blocks, "gate": 4 * blocks}
    assert min(float((b - a).abs().max()) for a, b in ((y0, y1), (y1, y2), (y2, y3))) > 1e-4
    fresh = copy.deepcopy(m)
    for name in ("_packed", "_dw_cache"):
        fresh.__dict__.pop(name, None)
    with torch.no_grad():
        assert torch.equal(fresh(xd, md), y3)
