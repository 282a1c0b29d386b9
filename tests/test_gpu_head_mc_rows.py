"""GPU: head_mc_h8_kernel<NKS, NQ> (csrc/head_mc_h8.hip) keeps only the 4 NQ accumulator rows per lane that can hold a class, masks the
dead rows of the last group by value (logit -inf) and loads one pass ahead.  Against the two-launch form (conv2d_h8 writing fp32 logits +
ops.mc_reduce) on the same fp16 features, at the bars of test_gpu_head_mc.py (p_bar 2e-6, entropies 2e-5, at most 2 argmax
differences), over every NQ with full and partly dead last groups in both lane halves, T with no prefetch / an even / an odd last pass,
one block and five blocks of 32 pixels, every NKS, with and without bias, and an eps large enough that real probabilities lie under the
clamp (the path where a dead row, whose p = 0 is also under it, could be counted as a class).

With C = 1 the normaliser ln C is 0, so h_norm is 0 / 0 = NaN in both forms (mi_norm is max(NaN, 0) = 0): positions where both are NaN
count as equal, a NaN in one only does not."""
import itertools

import pytest
import torch

from semanticlidarunc_amd import h8, ops

pytestmark = pytest.mark.gpu

CLASSES = [1, 8, 9, 16, 17, 20, 24, 25, 32]
PASSES = [1, 2, 3, 8]
BATCH = [1, 3]
CIN = [16, 32, 64]
SIZES = [(1, 32), (4, 40)]
EPS = [1e-12, 1e-3]


def _maxdiff(a, b):
    d = (a - b).abs()
    both = torch.isnan(a) & torch.isnan(b)
    return float(torch.where(both, torch.zeros_like(d), d).max())      # a NaN in one only stays NaN and fails every <=


def _head_and_reference(feats, wp, bias, cin, classes, t, b, hh, ww, eps):
    logits = h8.conv2d_h8([h8.H8Source(feats)], wp, cin, classes, 1, 1, 0, bias=bias, out_f32_nchw=True)
    want = ops.mc_reduce(logits.reshape(t, b, classes, hh, ww).contiguous(), eps)
    return h8.head_mc_h8(feats, wp, bias, classes, t, b, eps), want


@pytest.mark.parametrize("classes", CLASSES)
def test_head_rows_match_head_then_reduce(cuda, classes):
    g = torch.Generator(device=cuda).manual_seed(100 + classes)
    packed = {}
    for cin in CIN:
        w = torch.randn(classes, cin, 1, 1, device=cuda, generator=g) * 0.4
        packed[cin] = (h8.pack_conv_weight_h8(w), torch.randn(classes, device=cuda, generator=g))
    feats = {}
    for t, b, cin, (hh, ww) in itertools.product(PASSES, BATCH, CIN, SIZES):
        feats[(t, b, cin, hh, ww)] = h8.to_h8(torch.randn(t * b, cin, hh, ww, device=cuda, generator=g) * 2.0)
    worst = [0.0, 0.0, 0.0, 0]
    for (t, b, cin, hh, ww), x in feats.items():
        wp, bias = packed[cin]
        for use_bias, eps in itertools.product((True, False), EPS):
            got, want = _head_and_reference(x, wp, bias if use_bias else None, cin, classes, t, b, hh, ww, eps)
            case = f"C={classes} T={t} B={b} cin={cin} {hh}x{ww} bias={use_bias} eps={eps}"
            d = [_maxdiff(got[0], want[0]), _maxdiff(got[1], want[1]), _maxdiff(got[2], want[2]), int((got[3] != want[3]).sum())]
            worst = [max(p, q) for p, q in zip(worst, d)]
            assert d[0] <= 2e-6, case
            assert d[1] <= 2e-5 and d[2] <= 2e-5, case
            assert d[3] <= 2, case
            assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any()), case
    print(f"C={classes}: worst p_bar {worst[0]:.2e} h_norm {worst[1]:.2e} mi_norm {worst[2]:.2e} argmax flips {worst[3]}")


def test_argmax_ties_take_the_lower_class(cuda):
    """Classes 3 and 4 (lane half 0 row 3, lane half 1 row 0) and 17 and 19 share weight rows and bias, so they are exactly equal in
    every pass and in p_bar; a raised bias makes them the maximum at many pixels.  preds holds the lower index of each pair."""
    g = torch.Generator(device=cuda).manual_seed(7)
    t, b, cin, classes, hh, ww = 3, 2, 32, 20, 4, 40
    w = torch.randn(classes, cin, 1, 1, device=cuda, generator=g) * 0.4
    bias = torch.randn(classes, device=cuda, generator=g)
    bias[3] += 3.0
    bias[17] += 3.0
    w[4], bias[4] = w[3], bias[3]
    w[19], bias[19] = w[17], bias[17]
    feats = h8.to_h8(torch.randn(t * b, cin, hh, ww, device=cuda, generator=g) * 2.0)
    p_bar, _, _, preds = h8.head_mc_h8(feats, h8.pack_conv_weight_h8(w), bias, classes, t, b, 1e-12)
    assert torch.equal(p_bar[:, 3], p_bar[:, 4]) and torch.equal(p_bar[:, 17], p_bar[:, 19])
    assert int((preds == 4).sum()) == 0 and int((preds == 19).sum()) == 0
    assert int((preds == 3).sum()) > 0 and int((preds == 17).sum()) > 0
    assert torch.equal(preds.cpu(), p_bar.cpu().argmax(dim=1))             # the CPU argmax returns the first maximum


@pytest.mark.parametrize("eps", EPS)
def test_dead_rows_add_nothing(cuda, eps):
    """C = 20 leaves rows 8 .. 11 of the upper lane half dead.  Inputs scaled x30 saturate the softmax, so most live classes have p = 0
    like a dead row: p_bar still sums to 1 and both entropies stay in [0, 1].  T = 8 keeps 1 / T exact, so p_bar <= 1 holds exactly."""
    g = torch.Generator(device=cuda).manual_seed(11)
    t, b, cin, classes, hh, ww = 8, 3, 32, 20, 4, 40
    w = torch.randn(classes, cin, 1, 1, device=cuda, generator=g) * 0.4
    bias = torch.randn(classes, device=cuda, generator=g)
    feats = h8.to_h8(torch.randn(t * b, cin, hh, ww, device=cuda, generator=g) * 2.0 * 30.0)
    p_bar, hn, mi, preds = h8.head_mc_h8(feats, h8.pack_conv_weight_h8(w), bias, classes, t, b, eps)
    assert float((p_bar.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    assert float(p_bar.min()) >= 0.0
    assert float(hn.min()) >= 0.0 and float(hn.max()) <= 1.0 + 1e-6
    assert float(mi.min()) >= 0.0 and float(mi.max()) <= 1.0 + 1e-6
    assert int(preds.min()) >= 0 and int(preds.max()) < classes
