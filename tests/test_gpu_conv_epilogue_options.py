"""GPU: every epilogue option of the fp32-storage conv kernels -- bias -> activation (none / leaky / ReLU / tanh / SiLU) -> folded BatchNorm ->
[+ residual] -> [activation after the residual] -- at the three places the epilogue is written: the fp32 tiled kernel (conv_epilogue), the
split-fp16 tiled kernel and the split-fp16 streaming 1x1 kernel.  Reference: the same formula in float64 torch on the CPU.  Bars: those of
test_gpu_conv.py / test_gpu_f16x3.py -- 1e-4 * max(1, |want|max) against the reference and, for f16x3, 2e-5 * the same scale against the
exact-fp32 kernel on the same descriptor.  Every case prints its figure before it asserts (pytest -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from semanticlidarunc_amd import ops
from semanticlidarunc_amd.ops import ConvSource

pytestmark = pytest.mark.gpu
N, COUT = 2, 40          # 40 output channels: a partial second channel block
# site: precision, (ksize, dil, pad), channels of the concatenated sources, H, the widths it runs at, the kernel it must launch (or None)
SITES = {
    "fp32_tiled": ("fp32", (3, 1, 1), [8], 5, (36, 33), None),                 # W = 33: not a multiple of 4, the element-wise staging path
    "f16x3_tiled": ("f16x3", (3, 2, 2), [21], 5, (36, 33), None),
    "f16x3_stream1x1": ("f16x3", (1, 1, 0), [16, 16, 5], 4, (24,), "conv1x1_f16x3_kernel<2, 1>"),     # H * W = 96: pixel blocks stay inside one image
}
# act: keyword arguments of ops.conv2d_fused, the activation in float64, applied after the residual?
ACTS = {
    "none": ({}, lambda y: y, False),
    "leaky": ({"slope": 0.01}, lambda y: F.leaky_relu(y, 0.01), False),
    "relu": ({"act": "relu"}, torch.relu, False),
    "tanh": ({"act": "tanh"}, torch.tanh, False),
    "silu": ({"act": "silu"}, F.silu, False),
    "relu_late": ({"act": "relu", "act_after_resid": True}, torch.relu, True),
}


@functools.lru_cache(maxsize=None)
def _site(site, w):
    """inputs of one site at one width and conv(cat(srcs)) + bias in float64: computed once, shared by every case, never modified"""
    _, (k, dil, pad), parts, h, _, _ = SITES[site]
    g = torch.Generator().manual_seed(1000 * len(site) + w)
    srcs = [torch.randn(N, c, h, w, generator=g) for c in parts]
    cin = sum(parts)
    wgt = torch.randn(COUT, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias, bn_a, bn_b = torch.randn(COUT, generator=g) * 0.1, torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g) * 0.1
    res = torch.randn(N, COUT, h, w, generator=g)
    pre = F.conv2d(torch.cat(srcs, 1).double(), wgt.double(), bias.double(), padding=pad, dilation=dil)
    return srcs, wgt, bias, bn_a, bn_b, res, pre


def _want(site, w, act, resid):
    _, _, bias, bn_a, bn_b, res, pre = _site(site, w)
    _, fn, late = ACTS[act]
    y = pre if late else fn(pre)
    y = y * bn_a.double()[None, :, None, None] + bn_b.double()[None, :, None, None]
    if resid:
        y = y + res.double()
    return fn(y) if late else y


def _launch(dev, site, w, act, resid, precision, stats=None, record=False):
    _, (k, dil, pad), _, _, _, _ = SITES[site]
    srcs, wgt, bias, bn_a, bn_b, res, _ = _site(site, w)
    d = lambda t: t.to(dev).contiguous()
    wpack = ops.pack_conv_weight_f16x3(d(wgt)) if precision == "f16x3" else ops.pack_conv_weight(d(wgt))
    if record:
        ops.TIMING, ops.TIMING_TAGS = [], []              # measurement mode records the instantiation slu_conv2d_kernel_name reports
    try:
        got = ops.conv2d_fused([ConvSource(d(t)) for t in srcs], wpack, COUT, k, dil, pad, bias=d(bias), bn_a=d(bn_a), bn_b=d(bn_b),
                               resid=d(res) if resid else None, precision=precision, stats=stats, **ACTS[act][0])
        launched = [t[0] for t in ops.TIMING] if record else None
    finally:
        if record:
            ops.TIMING, ops.TIMING_TAGS = None, []
    torch.cuda.synchronize()
    return got, launched


@pytest.mark.parametrize("resid", [True, False], ids=["resid", "noresid"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("site", list(SITES))
def test_epilogue_option(cuda, site, act, resid):
    precision, _, _, _, widths, kernel = SITES[site]
    for w in widths:
        want = _want(site, w, act, resid)
        got, launched = _launch(cuda, site, w, act, resid, precision, record=kernel is not None)
        if kernel is not None:
            assert launched == [kernel], (site, w, launched)
        scale = max(1.0, float(want.abs().max()))
        err = float((got.cpu().double() - want).abs().max())
        print(f"{site} W={w} {act} resid={resid}: max abs err {err:.3e} (bar {1e-4 * scale:.3e})")
        assert err <= 1e-4 * scale, (site, w, act, resid, err)
        if precision == "f16x3":
            exact, _ = _launch(cuda, site, w, act, resid, "fp32")
            err = float((got - exact).abs().max())
            print(f"{site} W={w} {act} resid={resid}: max abs difference to the fp32 kernel {err:.3e} (bar {2e-5 * scale:.3e})")
            assert err <= 2e-5 * scale, (site, w, act, resid, err)


def test_statistics_with_late_relu_and_residual(cuda):
    """the fused batch statistics are those of the STORED output: after the residual and the late activation"""
    for w in SITES["fp32_tiled"][4]:
        st = torch.zeros((2, COUT), dtype=torch.float64, device=cuda)
        got, _ = _launch(cuda, "fp32_tiled", w, "relu_late", True, "fp32", stats=st)
        want = _want("fp32_tiled", w, "relu_late", True)
        assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
        s, q = ops.bn_stats(got)
        e1, e2 = float(((st[0] - s).abs() / (s.abs() + 1.0)).max()), float(((st[1] - q).abs() / q).max())
        print(f"W={w}: statistics relative error {e1:.3e} (sum), {e2:.3e} (sum of squares), bar 1e-5")
        assert e1 <= 1e-5 and e2 <= 1e-5
