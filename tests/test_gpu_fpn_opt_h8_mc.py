"""GPU: MC dropout on `semanticFCN_opt` under conv precision "f16": the pyramid once as h8 tensors, the decoder's first conv reading it
batch-broadcast with the dropout multipliers as per-source scales, and GroupNorm apply -> slu_head_mc_h8 for the fused evaluation step.
resnet18, B = 2, 32 x 64, T = 3, explicit multipliers.
The shared and the stacked schedule run the pyramid at different N, so the conv dispatch may pick other tiles for them: no equal bits are asked
between the two; each is held to the emulated fp16-storage bar of tests/test_gpu_fpn_opt_h8.py against the fp32 oracle.  Where both runs have
the same N (the decoder on the broadcast pyramid against the decoder on the pyramid repeated T times) the kernels are the same and the
results must be bit-identical."""
import pytest
import torch

from semanticlidarunc_amd import ops, salsanext as sn
from semanticlidarunc_amd.utils import mc_dropout
from semanticlidarunc_amd.utils.mc_dropout import mc_forward, mc_predict
from test_gpu_fpn_opt_h8 import check_against_emulated_bar, emulated_fp16_storage
from test_gpu_fpn_opt_mc import R18, _inputs, _model, _scale

pytestmark = pytest.mark.gpu
T, B = 3, 2


@pytest.fixture(scope="module")
def r18(cuda):
    m = _model(R18, cuda)
    x, meta = _inputs(R18, B)
    return m, x, meta


@pytest.fixture()
def f16():
    sn.set_conv_precision("f16")
    yield
    sn.set_conv_precision("fp32")


@pytest.fixture(scope="module")
def reference(r18):
    """(multipliers, fp32 oracle, CPU emulation of fp16 storage) of the T stacked passes, computed once"""
    m, x, meta = r18
    s = _scale(m, T * B)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    xr, mr, ds = x.repeat(T, 1, 1, 1), meta.repeat(T, 1, 1, 1), s.view(T * B, -1, 1, 1)
    want, _ = emulated_fp16_storage(sd, xr, mr, "resnet18", dropout_scale=ds, emulate=False)
    emu, _ = emulated_fp16_storage(sd, xr, mr, "resnet18", dropout_scale=ds, emulate=True)
    return s, want, emu


def test_broadcast_decoder_equals_the_decoder_on_the_repeated_pyramid(cuda, r18, f16):
    m, x, meta = r18
    s = _scale(m, T * B).to(cuda)
    with torch.no_grad():
        f1, ups = m._pyramid_h8(*m._check_inputs(x.to(cuda), meta.to(cuda)))
        shared = m._decoder_h8(f1, ups, s, passes=T)
        repeated = m._decoder_h8(f1.repeat(T, 1, 1, 1, 1), ups.repeat(T, 1, 1, 1, 1), s)
        raw = m._decoder_h8(f1, ups, s, passes=T, raw_head_input=True)
        raw_repeated = m._decoder_h8(f1.repeat(T, 1, 1, 1, 1), ups.repeat(T, 1, 1, 1, 1), s, raw_head_input=True)
    assert shared.shape == (T * B, 20, 32, 64) and shared.dtype == torch.float32
    assert torch.equal(shared, repeated)
    assert raw.dtype == torch.float16 and tuple(raw.shape) == (T * B, 2, 32, 64, 8) and torch.equal(raw, raw_repeated)


def test_shared_and_stacked_each_meet_the_emulated_bar(cuda, r18, f16, reference):
    m, x, meta = r18
    s, want, emu = reference
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        shared = m.forward_mc(xd, md, T, s.to(cuda))
        stacked = m.forward_with_dropout_scale(xd.repeat(T, 1, 1, 1), md.repeat(T, 1, 1, 1), s.to(cuda))
    check_against_emulated_bar("forward_mc (shared pyramid)", shared.cpu(), want, emu)
    check_against_emulated_bar("stacked forward", stacked.cpu(), want, emu)
    print(f"shared vs stacked: {float((shared - stacked).abs().max()):.2e}")
    g5 = shared.view(T, B, *shared.shape[1:])
    assert float((g5[0] - g5[1]).abs().max()) > 1e-3 and float((g5[1] - g5[2]).abs().max()) > 1e-3      # the passes differ


def _check_reduction(got, want, tag):
    """the bars of tests/test_gpu_head_mc.py"""
    d = [float((got[i] - want[i]).abs().max()) for i in range(3)]
    n_arg = int((got[3] != want[3]).sum())
    print(f"{tag}: p_bar {d[0]:.2e} H {d[1]:.2e} MI {d[2]:.2e} argmax {n_arg}")
    assert all(g.shape == w.shape and g.dtype == w.dtype for g, w in zip(got, want))
    assert d[0] <= 2e-6 and d[1] <= 2e-5 and d[2] <= 2e-5 and n_arg <= 2


def test_fused_head_agrees_with_the_reduction_of_the_logits(cuda, r18, f16):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        assert m.mc_fused_ok(xd, md, T)
    torch.manual_seed(5)
    want = ops.mc_reduce(mc_forward(m, [xd, md], T=T, share_prefix=True).contiguous())
    torch.manual_seed(5)
    got = mc_predict(m, [xd, md], T=T, share_prefix=True)
    _check_reduction(got, want, "fused head")
    assert not m.dropout_pyramid.training and not m.training


def test_launch_counts(cuda, r18, f16):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    s = _scale(m, T * B).to(cuda)
    ops.TIMING, ops.TIMING_TAGS[:] = [], []
    try:
        with torch.no_grad():
            m(xd, md)
        plain = list(ops.TIMING_TAGS)
        ops.TIMING, ops.TIMING_TAGS[:] = [], []
        with torch.no_grad():
            m.forward_mc(xd, md, T, s)
        tags = list(ops.TIMING_TAGS)
        ops.TIMING, ops.TIMING_TAGS[:] = [], []
        torch.manual_seed(5)
        mc_predict(m, [xd, md], T=T, share_prefix=True)
        names, fused_tags = [e[0] for e in ops.TIMING], list(ops.TIMING_TAGS)
    finally:
        ops.TIMING, ops.TIMING_TAGS[:] = None, []
    # the pyramid's layers appear once, at N = B; the decoder from its first conv on at N = T B; otherwise the launch list of a plain forward
    d0 = m.decoder_semantic[0]
    # (an UpsampleBlock's conv has the same channels as the first decoder conv: the decoder's is the last of them)
    dec0 = [i for i, tg in enumerate(tags) if f" {d0.in_channels}->{d0.out_channels} k3d1 " in tg][-1:]
    assert len(dec0) == 1 and len(tags) == len(plain) > 30, tags
    assert all(tg.startswith(f"N{B} ") for tg in tags[:dec0[0]]), tags
    assert all(tg.startswith(f"N{T * B} ") for tg in tags[dec0[0]:]), tags
    assert [tg.split(" ", 1)[1] for tg in tags] == [tg.split(" ", 1)[1] for tg in plain]
    # the fused step: one head + reduction launch, no head conv on its own, the same pyramid
    assert sum("head_mc_h8" in n for n in names) == 1, names
    assert not any("->20 k1" in tg and "head + MC" not in tg for tg in fused_tags), fused_tags
    assert not any("f16x3" in n or "conv_kernel<" in n or "head_mc_f32" in n for n in names), names
    assert [tg.split(" ", 1)[1] for tg in fused_tags[:dec0[0]]] == [tg.split(" ", 1)[1] for tg in plain[:dec0[0]]]


def test_unfused_fallback_where_the_fused_head_does_not_fit(cuda, r18, f16, monkeypatch):
    """slu_head_mc_h8 needs H W % 32 == 0.  A scan whose pixel count is not such a multiple (20 x 44 = 880) cannot reach the head: the model
    takes H and W that are multiples of 16 only, so H W at the head is a multiple of 256, and its other conditions (16 head input channels,
    at most 32 classes, which ops.mc_reduce shares) hold for every resnet18 / resnet34 model.  The fallback arm of mc_predict_fused (head conv
    to fp32 logits + ops.mc_reduce) is therefore entered here by switching the fit test off, and held to the fused result at the same bars."""
    from semanticlidarunc_amd import fpn_opt
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    with pytest.raises(RuntimeError, match="divisible by 16"):
        m(xd[:, :, :20, :44].contiguous(), md[:, :, :20, :44].contiguous())
    assert fpn_opt._head_mc_h8_fits(2, 20, 32 * 64) and not fpn_opt._head_mc_h8_fits(2, 20, 20 * 44) and not fpn_opt._head_mc_h8_fits(2, 33, 32 * 64)
    s = _scale(m, T * B).to(cuda)
    with torch.no_grad():
        fused = m.mc_predict_fused(xd, md, T, scale=s)
        definition = ops.mc_reduce(m.forward_mc(xd, md, T, s).view(T, B, 20, 32, 64))
        monkeypatch.setattr(fpn_opt, "_head_mc_h8_fits", lambda *a: False)
        ops.TIMING, ops.TIMING_TAGS[:] = [], []
        try:
            unfused = m.mc_predict_fused(xd, md, T, scale=s)
            names = [e[0] for e in ops.TIMING]
        finally:
            ops.TIMING, ops.TIMING_TAGS[:] = None, []
    assert not any("head_mc" in n for n in names), names
    _check_reduction(unfused, definition, "unfused fallback vs the reduction of forward_mc's logits")
    _check_reduction(unfused, fused, "unfused fallback vs fused")


def test_model_state_is_restored(cuda, r18, f16):
    m, x, meta = r18
    xd, md = x.to(cuda), meta.to(cuda)
    with torch.no_grad():
        before = m(xd, md)
    torch.manual_seed(5)
    shared = mc_forward(m, [xd, md], T=T, share_prefix=True)
    assert shared.shape == (T, B, 20, 32, 64)
    assert float((shared[0] - shared[1]).abs().max()) > 1e-3 and float((shared[1] - shared[2]).abs().max()) > 1e-3
    assert not m.dropout_pyramid.training and not m.training
    with torch.no_grad():
        assert torch.equal(m(xd, md), before)
    assert mc_dropout.MAX_STACK >= T
