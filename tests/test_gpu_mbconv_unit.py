"""GPU: the fused middle of an EfficientNetV2 MBConv block (csrc/mbconv_unit.hip) -- slu_dwconv3x3_se_fwd, slu_se_gate_psum -- and one block end to
end through effnet.block_forward, against fp64.

Bars: depthwise conv and its plane mean -- the project's exact-fp32 bar, err <= 1e-4 max(1, max|want|), against fp64 F.conv2d(groups=C) -> SiLU;
gate -- 1e-5 absolute (outputs lie in (0, 1); the bar of test_gpu_regnet.py::test_gate_kernel); one block -- 1e-4 max(1, max|want|) under 'fp32'."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import effnet_plain_restatement as R
from semanticlidarunc_amd import _lib, effnet as eff, ops, salsanext as sn

pytestmark = pytest.mark.gpu

# (N, C, H, W, stride).  A tile is a run of whole output rows of about 2048 outputs; 16-byte loads need W % 4 == 0, 16-byte stores Wo % 4 == 0.
DW_SHAPES = [
    (1, 1, 1, 1, 1),          # one pixel: every tap but the centre is padding
    (1, 3, 1, 7, 2),          # one row, stride 2: 1 x 4 outputs from an odd width (16-byte stores from scalar loads)
    (2, 5, 7, 9, 1),          # odd sizes, two images: the scalar route
    (2, 5, 7, 9, 2),
    (1, 2, 8, 256, 1),        # one full tile of the judged stride-1 shape: the vector route
    (1, 2, 16, 512, 2),       # the judged stride-2 shape: one tile
    (1, 2, 37, 132, 1),       # three tiles of 15 rows, the last with 7: vector route
    (2, 3, 33, 257, 2),       # 17 x 129 outputs: two tiles of 15 and 2 rows: scalar route
]
MULTI_TILE = {(1, 2, 37, 132, 1), (2, 3, 33, 257, 2)}


def _dw_problem(n, c, h, w, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * amp
    wt = torch.randn(c, 1, 3, 3, generator=g) * (2.0 / 9) ** 0.5
    b = torch.randn(c, generator=g) * 0.1
    return x, wt, b


def _check_dw(cuda, n, c, h, w, stride, x, wt, b):
    want = F.silu(F.conv2d(x.double(), wt.double(), b.double(), stride, 1, 1, c))
    count = want.shape[2] * want.shape[3]
    want_mean = want.mean((2, 3))
    xd, wd, bd = x.to(cuda), wt.reshape(c, 9).contiguous().to(cuda), b.to(cuda)
    y, psum = ops.dwconv3x3_se(xd, wd, bd, stride)
    tiles = _lib.load().slu_dwconv3x3_se_tiles(h, w, stride)
    assert y.shape == want.shape and psum.shape == (n, c, tiles) and tiles >= 1
    if (n, c, h, w, stride) in MULTI_TILE:
        assert tiles > 1
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((y.cpu().double() - want).abs().max())
    err_mean = float((psum.cpu().double().sum(-1) / count - want_mean).abs().max())
    print(f"{(n, c, h, w, stride)}: err {err:.2e}, mean err {err_mean:.2e} (bar {bar:.2e}), max|want| {float(want.abs().max()):.3g}, tiles {tiles}")
    assert err <= bar and err_mean <= bar                      # NaN anywhere fails both
    y2, psum2 = ops.dwconv3x3_se(xd, wd, bd, stride)
    assert torch.equal(y2, y) and torch.equal(psum2, psum)     # bit-identical run to run
    return y, xd, wd, bd


@pytest.mark.parametrize("n,c,h,w,stride", DW_SHAPES, ids=[f"N{s[0]}_C{s[1]}_{s[2]}x{s[3]}_s{s[4]}" for s in DW_SHAPES])
def test_depthwise_conv_and_its_mean(cuda, n, c, h, w, stride):
    x, wt, b = _dw_problem(n, c, h, w, 100 + c + h + w + stride)
    y, xd, wd, bd = _check_dw(cuda, n, c, h, w, stride, x, wt, b)
    # the kernel it replaces computes the same fmaf chain and the same SiLU
    assert torch.equal(ops.dwconv3x3(xd, wd, bd, stride, "silu"), y)


@pytest.mark.parametrize("n,c,h,w,stride", [(2, 5, 7, 9, 1), (1, 2, 16, 512, 2)], ids=["scalar", "vector"])
def test_depthwise_conv_on_the_tails_of_silu(cuda, n, c, h, w, stride):
    """Inputs in +-30: the conv's output reaches the range where SiLU is x (right tail) and a denormal-small negative (left tail)."""
    g = torch.Generator().manual_seed(5)
    x, wt, b = _dw_problem(n, c, h, w, 17)
    x = (torch.rand(x.shape, generator=g) * 60.0 - 30.0)
    want = F.conv2d(x.double(), wt.double(), b.double(), stride, 1, 1, c)
    assert float(want.max()) > 20.0 and float(want.min()) < -20.0
    _check_dw(cuda, n, c, h, w, stride, x, wt, b)


def test_wrapper_refusals(cuda):
    x, wt, b = _dw_problem(1, 4, 4, 8, 3)
    xd, wd, bd = x.to(cuda), wt.reshape(4, 9).contiguous().to(cuda), b.to(cuda)
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_se(x, wd, bd, 1)                          # CPU tensor
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_se(xd.transpose(2, 3), wd, bd, 1)         # non-contiguous
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_se(xd, wd[:3].contiguous(), bd, 1)
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_se(xd, wd, bd, 3)
    _, psum = ops.dwconv3x3_se(xd, wd, bd, 1)
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ops.se_gate_psum(psum, 32, z(2, 5, device=cuda), z(2, device=cuda), z(4, 2, device=cuda), z(4, device=cuda))
    with pytest.raises(RuntimeError):
        ops.se_gate_psum(psum, 0, z(2, 4, device=cuda), z(2, device=cuda), z(4, 2, device=cuda), z(4, device=cuda))
    with pytest.raises(RuntimeError):
        ops.se_gate_psum(z(1, 1537, 1, device=cuda), 1, z(2, 1537, device=cuda), z(2, device=cuda), z(1537, 2, device=cuda), z(1537, device=cuda))


# ---------------- the gate ----------------
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("s,c", [(1, 8), (24, 384), (48, 768), (96, 1536)])
def test_gate_kernel(cuda, s, c, t):
    n = 2
    g = torch.Generator().manual_seed(1000 * t + s + c)
    mean = torch.randn(n, c, generator=g)                                              # the mean of a SiLU output: either sign
    w1 = torch.randn(s, c, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, s, generator=g) * (2.0 / s) ** 0.5
    b1, b2 = torch.randn(s, generator=g) * 0.5, torch.randn(c, generator=g) * 0.5
    count = 1 if t == 1 else 7
    if t == 1:
        psum = mean.unsqueeze(2).clone()
    else:                                                                              # the same means as t partial sums over 7 pixels
        parts = torch.rand(n, c, t, generator=g) + 0.5
        psum = parts / parts.sum(2, keepdim=True) * (mean * 7.0).unsqueeze(2)
    real_mean = psum.double().sum(2) / count
    want = torch.sigmoid(F.linear(F.silu(F.linear(real_mean, w1.double(), b1.double())), w2.double(), b2.double()))
    d = [x.to(cuda) for x in (w1, b1, w2, b2)]
    got = ops.se_gate_psum(psum.to(cuda), count, *d)
    err = float((got.cpu().double() - want).abs().max())
    print(f"S {s}, C {c}, T {t}: err {err:.2e}, gates {float(want.mean()):.2f} +- {float(want.std()):.2f}")
    assert got.shape == (n, c) and err <= 1e-5
    assert float(want.std()) > 0.05                                                    # the gates are spread: the weights matter
    assert torch.equal(ops.se_gate_psum(psum.to(cuda), count, *d), got)
    if t == 1:                                                                         # [N, C] is taken as [N, C, 1]; the composed gate agrees
        assert torch.equal(ops.se_gate_psum(mean.to(cuda), 1, *d), got)
        composed = ops.se_scale(mean.view(n, c, 1, 1).to(cuda).contiguous(), *d)
        assert torch.equal(composed, got)                                              # one kernel behind both entry points (csrc/se_gate.hip)


# ---------------- one MBConv block end to end ----------------
# (input width, output width, expand ratio, stride, meta channels injected): a later block of a stage (residual) and a stage entry (stride 2, meta)
BLOCKS = [(128, 128, 4, 1, 0), (64, 128, 4, 2, 6), (48, 96, 6, 2, 3)]
_HOST = {}


def _host():
    """An FPN model as the owner of the packed-weight caches block_forward uses (its own parameters stay on the CPU and are not used)."""
    if "m" not in _HOST:
        _HOST["m"] = R.package_class()(backbone="efficientnet_v2_s").eval()
    return _HOST["m"]


@pytest.mark.parametrize("h,w", [(6, 33), (16, 16)])
@pytest.mark.parametrize("cin,cout,expand,stride,m", BLOCKS, ids=[f"{b[0]}to{b[1]}_x{b[2]}_s{b[3]}" + (f"_meta{b[4]}" if b[4] else "") for b in BLOCKS])
def test_one_block_against_the_fp64_restatement(cuda, cin, cout, expand, stride, m, h, w):
    torch.manual_seed(cin + cout)
    wrap = nn.Module()
    wrap.backbone = nn.Module()
    wrap.backbone.features = nn.Sequential(nn.Sequential(eff.MBConv(expand, 3, stride, cin, cout, 0.0)))
    R.he_fixture_(wrap, last_bn=1.0).eval()
    blk = wrap.backbone.features[0][0]
    assert blk.use_res_connect == (stride == 1 and cin == cout)
    sd = {k: v.double() for k, v in blk.state_dict().items()}
    g = torch.Generator().manual_seed(7 * h + w)
    x = torch.randn(2, cin, h, w, generator=g)
    meta = torch.randn(2, m, h, w, generator=g) if m else None
    xin = x.double() if m == 0 else torch.cat([x[:, :-m].double(), meta.double()], 1)
    want = R.mbconv(xin, sd, expand, stride, cin, cout)
    host = _host()
    name = f"test.{cin}.{cout}.{stride}.{h}.{w}"
    sn.set_conv_precision("fp32")
    with torch.no_grad():
        got = eff.block_forward(host, name, blk.to(cuda), x.to(cuda), None if m == 0 else meta.to(cuda)).cpu()
    assert got.shape == want.shape == (2, cout, (h + stride - 1) // stride, (w + stride - 1) // stride)
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f"err {err:.2e} (bar {bar:.2e}), max|want| {float(want.abs().max()):.3g}")
    assert err <= bar
    for cache in (host._packed, host._dw_cache):
        for key in [k for k in cache if k.startswith(name)]:
            cache.pop(key)
