"""GPU: slu_head_mc_f32 (csrc/head_mc_f32.hip) -- GroupNorm apply + ReLU + 1x1 head + softmax + MC-dropout reduction in one launch -- against
the chain it replaces (ops.groupnorm(relu=True) -> 1x1 ops.conv2d_fused -> ops.mc_reduce, the same fp32 operations per pixel) and against
fp64 torch on the CPU.  Bars as tests/test_gpu_head_mc.py holds them for the h8 kernel: against the chain p_bar 2e-6, entropies 2e-5, at
most 2 differing argmax pixels; against fp64 p_bar 1e-5, MI 1e-4.  The argmax cap is a condition on the inputs: the seeds are chosen so that
the fp64 reference's two largest p_bar differ by more than 1e-4 on all but at most 2 pixels of a case (asserted before the comparison)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import uncertainty as ounc
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.ops import ConvSource

pytestmark = pytest.mark.gpu
EPS = 1e-12
# (Cin, C, T, B, H, W, GroupNorm groups or None)
CASES = [(16, 20, 3, 2, 8, 64, 8),          # resnet18 / 34 head
         (64, 5, 2, 1, 4, 32, 32),          # resnet50 head
         (84, 21, 4, 1, 5, 13, 4),          # efficientnet_v2 head; HW = 65: scalar path + masked tail
         (16, 32, 1, 2, 2, 48, None),       # T = 1: MI must vanish
         (2, 3, 5, 3, 3, 100, 1),
         (128, 32, 2, 1, 1, 36, None)]
IDS = ["-".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    """CPU inputs and the fp64 reference, computed once per case and never modified."""
    cin, c, t, b, h, w, groups = case
    g = torch.Generator().manual_seed(1000 + 7 * cin + c)
    x = torch.randn(t * b, cin, h, w, generator=g) * 3.0 + 1.0
    wt = torch.randn(c, cin, 1, 1, generator=g) / math.sqrt(cin)
    bias = torch.randn(c, generator=g)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    v = x.double()
    if groups is not None:
        v = F.relu(F.group_norm(v, groups, gamma.double(), beta.double(), 1e-5))
    logits = F.conv2d(v, wt.double(), bias.double())
    ref = ounc.mc_reduce(logits.reshape(t, b, c, h, w), EPS)
    return x, wt, bias, gamma, beta, ref


def _decided(p_bar):
    """number of pixels whose two largest p_bar are closer than 1e-4: only there may an argmax legitimately differ"""
    top = p_bar.topk(2, dim=1).values
    return int(((top[:, 0] - top[:, 1]) <= 1e-4).sum())


def _chain(x, wt, bias, gamma, beta, case):
    cin, c, t, b, h, w, groups = case
    y, stats = x, None
    if groups is not None:
        y, stats = ops.groupnorm(x, groups, gamma, beta, 1e-5, relu=True, return_stats=True)
    logits = ops.conv2d_fused([ConvSource(y)], ops.pack_conv_weight(wt), c, 1, 1, 0, bias=bias, act="none")
    return ops.mc_reduce(logits.reshape(t, b, c, h, w), EPS), stats


def _fused(x, wt, bias, gamma, beta, case):
    cin, c, t, b, h, w, groups = case
    if groups is None:
        return ops.head_mc_f32(x, wt, bias, t, b, EPS), None
    stats = ops.groupnorm_stats(x, groups, 1e-5)
    return ops.head_mc_f32(x, wt, bias, t, b, EPS, gn_stats=stats, gn_groups=groups, gn_gamma=gamma, gn_beta=beta, relu=True), stats


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_unfused_chain_and_fp64(cuda, case):
    cin, c, t, b, h, w, groups = case
    x, wt, bias, gamma, beta, ref = _case(case)
    assert _decided(ref[0]) <= 2, "seed: the fp64 reference has more than 2 undecided pixels"
    dev = [a.to(cuda) for a in (x, wt, bias, gamma, beta)]
    want, wstats = _chain(*dev, case)
    got, gstats = _fused(*dev, case)
    if groups is not None:
        assert torch.equal(gstats, wstats)                   # slu_groupnorm_stats: the numbers the unfused path normalises with
    d_p = float((got[0] - want[0]).abs().max())
    d_h, d_mi = float((got[1] - want[1]).abs().max()), float((got[2] - want[2]).abs().max())
    n_arg = int((got[3] != want[3]).sum())
    r_p, r_mi = float((got[0].cpu().double() - ref[0]).abs().max()), float((got[2].cpu().double() - ref[2]).abs().max())
    print(f"{case}: vs chain p_bar {d_p:.2e} H {d_h:.2e} MI {d_mi:.2e} argmax {n_arg}; vs fp64 p_bar {r_p:.2e} MI {r_mi:.2e}")
    assert got[3].dtype == torch.int64 and got[0].shape == (b, c, h, w) and got[1].shape == got[2].shape == got[3].shape == (b, h, w)
    assert d_p <= 2e-6
    assert d_h <= 2e-5 and d_mi <= 2e-5
    assert n_arg <= 2
    assert int((got[3].cpu() != ref[3]).sum()) <= 2
    assert r_p <= 1e-5 and r_mi <= 1e-4
    assert float((got[0].sum(1) - 1.0).abs().max()) <= 1e-5
    assert float(got[2].min()) >= 0.0 and float((got[2] - got[1]).max()) <= 1e-5 and float(got[1].max()) <= 1.0 + 1e-5
    if t == 1:
        assert float(got[2].max()) <= 1e-5


# T a power of two: the mean over passes of equal probabilities is exact.  C = 32: 1 / C is exact as well.
@pytest.mark.parametrize("case", [(16, 20, 2, 2, 8, 64, 8), (16, 32, 1, 2, 2, 48, None), (2, 3, 4, 3, 3, 100, 1)], ids=["c20", "c32", "c3"])
def test_ties_take_the_first_class(cuda, case):
    cin, c, t, b, h, w, groups = case
    x, _, _, gamma, beta, _ = _case((cin, c, t, b, h, w, groups))
    wt, bias = torch.zeros(c, cin, 1, 1), torch.zeros(c)
    got, _ = _fused(*[a.to(cuda) for a in (x, wt, bias, gamma, beta)], case)
    print(f"{case}: ties H-1 {float((got[1] - 1.0).abs().max()):.2e} MI max {float(got[2].max()):.2e}")
    assert float((got[0] - 1.0 / c).abs().max()) <= 1e-7
    assert int((got[3] != 0).sum()) == 0
    assert float((got[1] - 1.0).abs().max()) <= 1e-6
    assert float(got[2].abs().max()) == 0.0


def test_outputs_stay_inside_their_allocations(cuda):
    """HW = 65 (scalar path, masked tail): the four outputs carved from one buffer, each followed by sentinels that must survive."""
    case = CASES[2]
    cin, c, t, b, h, w, groups = case
    x, wt, bias, gamma, beta, _ = _case(case)
    x, wt, bias, gamma, beta = [a.to(cuda) for a in (x, wt, bias, gamma, beta)]
    hw, guard, mark = h * w, 64, -12345.0
    sizes = [b * c * hw, b * hw, b * hw, 2 * b * hw]              # floats; preds is int64 = 2 floats per pixel
    buf = torch.full((sum(s + guard + 1 for s in sizes),), mark, dtype=torch.float32, device=cuda)
    views, guards, off = [], [], 0
    for s in sizes:
        off += off % 2                                           # 8-byte alignment for the int64 view
        views.append(buf[off:off + s])
        guards.append((off + s, off + s + guard))
        off += s + guard
    p_bar, hn, mi = views[0].view(b, c, h, w), views[1].view(b, h, w), views[2].view(b, h, w)
    preds = views[3].view(torch.int64).view(b, h, w)
    stats = ops.groupnorm_stats(x, groups, 1e-5)
    ops.head_mc_f32_out(x, wt, bias, t, b, EPS, stats[0], stats[1], groups, gamma, beta, True, p_bar, hn, mi, preds)
    want = ops.head_mc_f32(x, wt, bias, t, b, EPS, gn_stats=stats, gn_groups=groups, gn_gamma=gamma, gn_beta=beta, relu=True)
    for lo, hi in guards:
        assert bool((buf[lo:hi] == mark).all()), f"sentinels {lo}:{hi} overwritten"
    assert torch.equal(p_bar, want[0]) and torch.equal(hn, want[1]) and torch.equal(mi, want[2]) and torch.equal(preds, want[3])
    assert int(preds.min()) >= 0 and int(preds.max()) < c


def test_wrapper_contracts(cuda):
    x, wt, bias, gamma, beta, _ = _case(CASES[0])
    x, wt, bias, gamma, beta = [a.to(cuda) for a in (x, wt, bias, gamma, beta)]
    with pytest.raises(RuntimeError):
        ops.head_mc_f32(x, wt, bias, 4, 2)                                       # T * B != N
    with pytest.raises(RuntimeError):
        ops.head_mc_f32(x.cpu(), wt, bias, 3, 2)
    with pytest.raises(RuntimeError):
        ops.head_mc_f32(x, wt[:, :8].contiguous(), bias, 3, 2)
    with pytest.raises(RuntimeError):
        ops.head_mc_f32(x, wt, bias, 3, 2, gn_gamma=gamma)                        # affine without statistics
    with pytest.raises(RuntimeError):
        ops.groupnorm_stats(x, 5)
