"""GPU: MC dropout on `semanticFCN_opt` with the pyramid computed once (fpn_opt.SemanticNetworkWithFPN.forward_mc) and with GroupNorm apply +
head + reduction in one launch (mc_predict_fused -> slu_head_mc_f32), against the stacked path on the same multipliers.  Bars: shared against
stacked logits 1e-6 (what tests/test_gpu_model.py holds for SalsaNext's shared prefix), against the oracle 1e-3 (the project's bar), fused
against ops.mc_reduce of the stacked logits p_bar 2e-6 / entropies 2e-5 / at most 2 argmax pixels (tests/test_gpu_head_mc.py).
The argmax cap was meant to hold under the condition that the stacked p_bar's two largest values differ by more than 1e-4 on all but at most
2 pixels.  No seed gives that here: a randomly initialised 20-class model leaves 24 (resnet18), 18 (resnet34), 6 (efficientnet_v2_s) and 14
(resnet18, T = 5) of the 4096 / 2048 pixels closer than that (resnet50 / 5 classes: 0).  So the cap is held on ALL pixels, without the
condition's protection, and a pixel that does differ must be one of the close ones; measured: no pixel differs in any case."""
import pytest
import torch

from oracle import fpn_opt as ofpo
from semanticlidarunc_amd import ops, salsanext as sn
from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN
from semanticlidarunc_amd.testing import randomize_bn_
from semanticlidarunc_amd.utils import mc_dropout
from semanticlidarunc_amd.utils.mc_dropout import mc_forward, mc_predict

pytestmark = pytest.mark.gpu
R18 = dict(backbone="resnet18", input_channels=2, meta_channel_dim=6, num_classes=20)
LADDERS = {"resnet34_noatt_c21": dict(backbone="resnet34", input_channels=2, meta_channel_dim=3, num_classes=21, attention=False, multi_scale_meta=False),
           "resnet50_c5": dict(backbone="resnet50", input_channels=2, meta_channel_dim=3, num_classes=5),                  # head Cin 64
           "efficientnet_v2_s_c20": dict(backbone="efficientnet_v2_s", input_channels=2, meta_channel_dim=3, num_classes=20)}   # head Cin 84


def _model(kw, cuda):
    torch.manual_seed(0)
    m = randomize_bn_(SemanticNetworkWithFPN(**kw), 3).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(9)
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.copy_(torch.rand(mod.num_channels, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_channels, generator=g) * 0.1)
    return m.to(cuda)


def _inputs(kw, b, seed=13, h=32, w=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 2, h, w, generator=g) * torch.tensor([20.0, 0.3]).view(1, 2, 1, 1)
    meta = torch.randn(b, kw["meta_channel_dim"], h, w, generator=g) * 5.0
    return x, meta


def _scale(m, n, seed=21):
    """Dropout2d(0.1) multipliers [n, C_pyramid]: zeros and 1 / 0.9"""
    g = torch.Generator().manual_seed(seed)
    c = m.decoder_semantic[0].in_channels
    s = (torch.rand(n, c, generator=g) >= 0.1).float() / 0.9
    assert int((s == 0).sum()) > 0
    return s


@pytest.fixture(scope="module")
def r18(cuda):
    m = _model(R18, cuda)
    x, meta = _inputs(R18, 2)
    return m, x, meta


def _undecided(p_bar):
    """[B,H,W] mask of the pixels whose two largest p_bar are closer than 1e-4"""
    top = p_bar.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= 1e-4


def _check_reduction(got, want, tag=""):
    und = _undecided(want[0])
    d = [float((got[i] - want[i]).abs().max()) for i in range(3)]
    differs = got[3] != want[3]
    n_arg = int(differs.sum())
    print(f"{tag}: undecided {int(und.sum())}; p_bar {d[0]:.2e} H {d[1]:.2e} MI {d[2]:.2e} argmax {n_arg}")
    assert d[0] <= 2e-6 and d[1] <= 2e-5 and d[2] <= 2e-5
    assert n_arg <= 2 and not bool((differs & ~und).any())


def _shared_vs_scaled(m, x, meta, t, cuda, tag=""):
    s = _scale(m, t * x.shape[0]).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        got = m.forward_mc(xd, md, t, s)
        want = m.forward_with_dropout_scale(xd.repeat(t, 1, 1, 1), md.repeat(t, 1, 1, 1), s)
    err = float((got - want).abs().max())
    print(f"{tag}: forward_mc vs stacked forward {err:.2e}")
    assert got.shape == want.shape and err <= 1e-6
    return got, s


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_forward_mc_equals_the_stacked_forward_and_the_oracle(cuda, r18, prec):
    m, x, meta = r18
    t = 3
    sn.set_conv_precision(prec)
    try:
        got, s = _shared_vs_scaled(m, x, meta, t, cuda, prec)
    finally:
        sn.set_conv_precision("fp32")
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        want = ofpo.fpn_opt_forward(sd, x.repeat(t, 1, 1, 1), meta.repeat(t, 1, 1, 1), "resnet18", dropout_scale=s.cpu().view(t * 2, -1, 1, 1))
    err = float((got.cpu() - want).abs().max())
    print(f"{prec}: forward_mc vs oracle {err:.2e}")
    assert err <= 1e-3
    g5 = got.view(t, 2, *got.shape[1:])
    assert float((g5[0] - g5[1]).abs().max()) > 1e-3 and float((g5[1] - g5[2]).abs().max()) > 1e-3      # the passes differ


def test_mc_forward_shared_equals_stacked_and_restores_the_model(cuda, r18):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        before = m(xd, md)
    torch.manual_seed(5)
    stacked = mc_forward(m, [xd, md], T=3, share_prefix=False)
    torch.manual_seed(5)
    shared = mc_forward(m, [xd, md], T=3, share_prefix=True)
    assert shared.shape == (3, 2, 20, 32, 64)
    assert float((shared - stacked).abs().max()) <= 1e-6
    assert float((shared[0] - shared[1]).abs().max()) > 1e-3
    assert not m.dropout_pyramid.training and not m.training
    with torch.no_grad():
        assert torch.equal(m(xd, md), before)


def _predict_both(m, xd, md, t, seed=5):
    torch.manual_seed(seed)
    want = ops.mc_reduce(mc_forward(m, [xd, md], T=t, share_prefix=False).contiguous())
    torch.manual_seed(seed)
    got = mc_predict(m, [xd, md], T=t, share_prefix=True)
    return got, want


def test_mc_predict_shared_is_fused_and_agrees(cuda, r18):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        assert m.mc_fused_ok(xd, md, 3) and not m.mc_fused_ok(x, meta, 3)
    got, want = _predict_both(m, xd, md, 3)
    _check_reduction(got, want, "resnet18")
    assert not m.dropout_pyramid.training
    ops.TIMING, ops.TIMING_TAGS[:] = [], []
    try:
        torch.manual_seed(5)
        timed = mc_predict(m, [xd, md], T=3, share_prefix=True)
        names, tags = [e[0] for e in ops.TIMING], list(ops.TIMING_TAGS)
    finally:
        ops.TIMING, ops.TIMING_TAGS[:] = None, []
    assert all(torch.equal(a, b) for a, b in zip(timed, got))
    assert sum("head_mc_f32" in n for n in names) == 1
    assert not any("->20 k1" in tg for tg in tags), tags              # the head conv is not launched on its own


def test_the_pyramid_runs_once(cuda, r18):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    ops.TIMING, ops.TIMING_TAGS[:] = [], []
    try:
        with torch.no_grad():
            m(xd, md)
        plain = list(ops.TIMING_TAGS)
        ops.TIMING, ops.TIMING_TAGS[:] = [], []
        with torch.no_grad():
            m.forward_mc(xd, md, 3, _scale(m, 6).to(cuda))
        tags = list(ops.TIMING_TAGS)
    finally:
        ops.TIMING, ops.TIMING_TAGS[:] = None, []
    assert len(tags) == len(plain) > 4
    dec0 = len(tags) - 4                                              # dec0, dec1, dec_up, dec_out
    assert f" {m.decoder_semantic[0].in_channels}->{m.decoder_semantic[0].out_channels} k3d1 " in tags[dec0], tags
    assert all(tg.startswith("N2 ") for tg in tags[:dec0]), tags
    assert all(tg.startswith("N6 ") for tg in tags[dec0:]), tags
    assert [tg.split(" ", 1)[1] for tg in tags] == [tg.split(" ", 1)[1] for tg in plain]


@pytest.mark.parametrize("tag", list(LADDERS))
def test_other_ladders(cuda, tag):
    kw = LADDERS[tag]
    m = _model(kw, cuda)
    x, meta = _inputs(kw, 1)
    _shared_vs_scaled(m, x, meta, 2, cuda, tag)
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        assert m.mc_fused_ok(xd, md, 2)
    got, want = _predict_both(m, xd, md, 2)
    _check_reduction(got, want, tag)


def test_chunked_passes(cuda, r18, monkeypatch):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    monkeypatch.setattr(mc_dropout, "MAX_STACK", 2)
    torch.manual_seed(7)
    stacked = mc_forward(m, [xd, md], T=5, share_prefix=False)
    torch.manual_seed(7)
    shared = mc_forward(m, [xd, md], T=5, share_prefix=True)
    assert shared.shape == (5, 2, 20, 32, 64) and float((shared - stacked).abs().max()) <= 1e-6
    got, want = _predict_both(m, xd, md, 5, seed=7)                    # T > MAX_STACK: mc_predict reduces the chunked logits
    _check_reduction(got, want, "chunked")


def test_contracts(cuda, r18):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.forward_mc(xd, md, 2)
        with torch.no_grad():
            assert not m.mc_fused_ok(xd, md, 2)
    finally:
        m.eval()
    with pytest.raises(RuntimeError):
        m.forward_mc(x, meta, 2)                                      # CPU tensors
    with pytest.raises(RuntimeError):
        m.forward_mc(xd, md, 0)
    # the plain FPN has no dropout and no forward_mc: share_prefix changes nothing
    from semanticlidarunc_amd.models.semanticFCN import SemanticNetworkWithFPN as PlainFPN
    torch.manual_seed(0)
    plain = randomize_bn_(PlainFPN("resnet18", 2, 6, num_classes=20), 3).eval().to(cuda)
    assert not hasattr(plain, "forward_mc")
    a = mc_predict(plain, [xd, md], T=2, share_prefix=True)
    b = mc_predict(plain, [xd, md], T=2, share_prefix=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
