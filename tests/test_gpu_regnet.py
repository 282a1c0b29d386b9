"""GPU: the RegNetY kernels (slu_regnet_gconv_fwd, slu_regnet_se_gate, slu_regnet_sample2), one Y block end to end, and both FPN classes on the
regnet_y_1_6gf / regnet_y_3_2gf encoders against the fp64 restatement (tests/regnet_restatement.py) and the goldens of the reference's own classes.

Bars: grouped conv and its pooled mean -- the exact-fp32 conv bar of test_gpu_conv.py, err <= 1e-4 max(1, max|want|), against fp64
F.conv2d(groups=...); gate -- 1e-5 absolute (outputs lie in (0, 1)); one block -- 1e-4 max(1, max|want|) under 'fp32'; models -- err <= 1e-3 S
and at most 1e-3 of the pixels with another argmax, S = max(1, max|want|), under 'fp32' and 'f16x3' (the CPU fp32 run of the restatement is
within 2e-6 S and flips no pixel on these fixtures: test_regnet_cpu.py::test_fixture_conditions)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import regnet_restatement as R
from conftest import golden
from semanticlidarunc_amd import _lib, ops, regnet as rgn, salsanext as sn
from semanticlidarunc_amd.utils.mc_dropout import mc_forward, mc_predict

pytestmark = pytest.mark.gpu

CASES = R.model_cases()
NAN = float("nan")


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ---------------- 1. the grouped conv ----------------
# (N, C, gw, H, W).  The kernel's constants: 256 lanes = one 8 x 32 output tile, or 4 x 64 when the output has at most four rows; input chunks of
# 8 channels through LDS (gw / 8 = 1, 2, 3 chunks); one workgroup per (tile, group, image); four waves per tile sum.
GCONV_SHAPES = [
    (1, 24, 24, 1, 1),        # the smallest map: every tap but the centre is padding; one group, three chunks; the 4 x 64 tile holds one pixel
    (2, 48, 24, 5, 7),        # two groups, two images (batch stride); stride 1 takes the 8 x 32 tile (5 rows), stride 2 the 4 x 64 one (3 rows)
    (1, 104, 8, 9, 70),       # gw 8 (one chunk), 13 groups; 9 x 70 crosses the 8 x 32 tile both ways (2 x 3 tiles), no multiple of it; stride 2: 5 x 35
    (2, 144, 16, 6, 33),      # gw 16 (two chunks); W = 32 + 1: a tile column of one pixel; stride 2: 3 x 17 on the 4 x 64 tile
    (1, 888, 24, 4, 16),      # 37 groups on a map smaller than the 4 x 64 tile (regnet_y_1_6gf's last stage at 64 x 256)
    (1, 72, 24, 2, 1024),     # a long row: 16 tile columns of 64, half of each tile's rows outside; stride 2: 1 x 512
    (1, 1512, 24, 2, 4),      # 63 groups, the widest model's last stage; stride 2: 1 x 2
    (1, 32, 16, 17, 65),      # H and W one more than a multiple of the tile at both strides: 17 x 65 = (2 x 8 + 1) x (2 x 32 + 1), stride 2: 9 x 33
]


def _gconv_problem(n, c, gw, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(c, gw, 3, 3, generator=g) * (2.0 / (9 * gw)) ** 0.5
    b = torch.randn(c, generator=g) * 0.1
    return x, wt, b


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n,c,gw,h,w", GCONV_SHAPES, ids=[f"N{s[0]}_C{s[1]}_gw{s[2]}_{s[3]}x{s[4]}" for s in GCONV_SHAPES])
def test_grouped_conv_and_its_mean(cuda, n, c, gw, h, w, stride):
    x, wt, b = _gconv_problem(n, c, gw, h, w, 100 + c + h + stride)
    want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride, 1, 1, c // gw))
    want_mean = want.mean((2, 3))
    # the input is channels [2, 2 + C) of a wider tensor whose other channels are NaN; the output buffer is NaN before the launch
    wide = torch.cat([torch.full((n, 2, h, w), NAN), x, torch.full((n, 3, h, w), NAN)], 1).to(cuda)
    wg = ops.pack_regnet_gconv_weight(wt.to(cuda), gw)
    bd = b.to(cuda)
    out = torch.full(want.shape, NAN, device=cuda)
    got, psum = ops.regnet_gconv(wide, wg, bd, stride, coff=2, cuse=c, out=out)
    assert got.shape == want.shape and psum.shape[:2] == (n, c)
    s1 = max(8, c // 4)
    gw1, gb1, gw2, gb2 = (torch.zeros(s1, c, device=cuda), torch.zeros(s1, device=cuda), torch.zeros(c, s1, device=cuda), torch.zeros(c, device=cuda))
    gate, mean = ops.regnet_se_gate(psum, want.shape[2] * want.shape[3], gw1, gb1, gw2, gb2, want_mean=True)
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got.cpu().double() - want).abs().max())
    err_mean = float((mean.cpu().double() - want_mean).abs().max())
    print(f"stride {stride}: err {err:.2e}, mean err {err_mean:.2e} (bar {bar:.2e}), max|want| {float(want.abs().max()):.3g}, tiles {psum.shape[2]}")
    assert err <= bar and err_mean <= bar                      # NaN anywhere fails both
    assert bool((gate == 0.5).all())                           # sigmoid(0)
    again, psum2 = ops.regnet_gconv(wide, wg, bd, stride, coff=2, cuse=c)
    _, mean2 = ops.regnet_se_gate(psum2, want.shape[2] * want.shape[3], gw1, gb1, gw2, gb2, want_mean=True)
    assert torch.equal(again, got) and torch.equal(psum2, psum) and torch.equal(mean2, mean)      # bit-identical run to run


def test_grouped_conv_refusals(cuda):
    x, wt, b = (t.to(cuda) for t in _gconv_problem(1, 48, 24, 4, 8, 3))
    wg = ops.pack_regnet_gconv_weight(wt, 24)
    y, psum = ops.regnet_gconv(x, wg, b, 1)
    assert y.shape == (1, 48, 4, 8) and psum.shape == (1, 48, 1)
    lib = _lib.load()
    out = torch.full((1, 48, 4, 8), 7.0, device=cuda)
    args = (x.data_ptr(), 48, 0, wg.data_ptr(), b.data_ptr(), out.data_ptr(), psum.data_ptr(), 1, 48)
    assert lib.slu_regnet_gconv_fwd(*args, 12, 4, 8, 1, None) == -2                         # a group width that is not instantiated
    assert lib.slu_regnet_gconv_fwd(*args, 24, 4, 8, 3, None) == -1                         # stride 3
    assert lib.slu_regnet_gconv_fwd(None, 48, 0, wg.data_ptr(), b.data_ptr(), out.data_ptr(), psum.data_ptr(), 1, 48, 24, 4, 8, 1, None) == -1
    assert lib.slu_regnet_gconv_fwd(x.data_ptr(), 48, 0, wg.data_ptr(), b.data_ptr(), out.data_ptr(), None, 1, 48, 24, 4, 8, 1, None) == -1
    assert lib.slu_regnet_gconv_fwd(x.data_ptr(), 48, 8, wg.data_ptr(), b.data_ptr(), out.data_ptr(), psum.data_ptr(), 1, 48, 24, 4, 8, 1, None) == -1
    assert lib.slu_regnet_se_gate(None, 1, 1.0, wg.data_ptr(), b.data_ptr(), wg.data_ptr(), b.data_ptr(), out.data_ptr(), None, 1, 48, 8, None) == -1
    assert lib.slu_regnet_sample2(ctypes.byref(_lib.Cat2(None, None, 48, 0, 48, 0, 0)), out.data_ptr(), 1, 4, 8, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                         # nothing was launched
    with pytest.raises(RuntimeError):
        ops.pack_regnet_gconv_weight(torch.zeros(48, 12, 3, 3, device=cuda), 12)
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x.cpu(), wg, b, 1)                                                 # CPU tensor
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x.transpose(2, 3), wg, b, 1)                                       # non-contiguous
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x.double(), wg, b, 1)                                              # dtype
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x, wg[:1].contiguous(), b, 1)                                      # one group for 48 channels
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x, wg, b[:24].contiguous(), 1)
    with pytest.raises(RuntimeError):
        ops.regnet_gconv(x, wg, b, 3)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.regnet_gconv(x, wg, b, 1, out=x)
    with pytest.raises(RuntimeError):
        ops.regnet_se_gate(psum, 32, torch.zeros(8, 47, device=cuda), torch.zeros(8, device=cuda), torch.zeros(48, 8, device=cuda), torch.zeros(48, device=cuda))


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (5, 7), (6, 33), (16, 16)])
def test_sample2_is_exact(cuda, h, w):
    g = torch.Generator().manual_seed(h * 10 + w)
    x = torch.randn(2, 7, h, w, generator=g)
    want = x[:, :, ::2, ::2]
    assert torch.equal(ops.regnet_sample2(x.to(cuda)).cpu(), want)
    first = torch.cat([x[:, :4], torch.full((2, 3, h, w), NAN)], 1)
    got = ops.regnet_sample2(first.to(cuda), 0, 4, x[:, 4:].contiguous().to(cuda)).cpu()
    assert torch.equal(got, want)


# ---------------- 2. the gate ----------------
SQUEEZE_WIDTHS = [8, 12, 18, 30, 54, 84, 144, 222]      # round(0.25 * block input width) over the four models


@pytest.mark.parametrize("c", [48, 120, 888, 1512])
@pytest.mark.parametrize("s", SQUEEZE_WIDTHS)
def test_gate_kernel(cuda, s, c):
    for n in (1, 3):
        g = torch.Generator().manual_seed(1000 * n + s + c)
        mean = torch.rand(n, c, generator=g) * 2.0                                         # the mean of a ReLU output
        w1 = torch.randn(s, c, generator=g) * (2.0 / c) ** 0.5
        w2 = torch.randn(c, s, generator=g) * (2.0 / s) ** 0.5
        b1, b2 = torch.randn(s, generator=g) * 0.5, torch.randn(c, generator=g) * 0.5
        want = torch.sigmoid(F.linear(F.relu(F.linear(mean.double(), w1.double(), b1.double())), w2.double(), b2.double()))
        d = [t.to(cuda) for t in (w1, b1, w2, b2)]
        got = ops.regnet_se_gate(mean.to(cuda), 1, *d)
        err = float((got.cpu().double() - want).abs().max())
        assert got.shape == (n, c) and err <= 1e-5, (n, err)
        assert 0.05 < float(want.std())                                                    # the gates are spread: the weights matter
        # the same means as five partial sums over 7 pixels
        parts = torch.rand(n, c, 5, generator=g)
        parts = parts / parts.sum(2, keepdim=True) * (mean * 7.0).unsqueeze(2)
        got5, mean5 = ops.regnet_se_gate(parts.to(cuda), 7, *d, want_mean=True)
        assert float((mean5.cpu().double() - mean.double()).abs().max()) <= 1e-5 and float((got5.cpu().double() - want).abs().max()) <= 1e-5
        assert torch.equal(ops.regnet_se_gate(parts.to(cuda), 7, *d), got5)
    # the SiLU gate of EfficientNet is another operator and keeps its behaviour
    x = mean.view(n, c, 1, 1).to(cuda).contiguous()
    silu = torch.sigmoid(F.linear(F.silu(F.linear(mean.double(), w1.double(), b1.double())), w2.double(), b2.double()))
    assert float((ops.se_scale(x, *d).cpu().double() - silu).abs().max()) <= 1e-5
    assert float((silu - want).abs().max()) > 1e-3


# ---------------- 3. one Y block end to end ----------------
# (width in, width out, stride, group width, meta channels injected): the first and a later block of a stage for every group width
BLOCKS = [(32, 48, 2, 8, 0), (104, 104, 1, 8, 0), (64, 144, 2, 16, 6), (336, 336, 1, 24, 0), (576, 1512, 2, 24, 3)]
_HOST = {}


def _host():
    """An FPN model as the owner of the packed-weight caches y_block_forward uses (its own parameters stay on the CPU and are not used)."""
    if "m" not in _HOST:
        _HOST["m"] = R.package_class("plain")(backbone="regnet_y_1_6gf").eval()
    return _HOST["m"]


@pytest.mark.parametrize("h,w", [(6, 33), (16, 16)])
@pytest.mark.parametrize("win,wout,stride,gw,m", BLOCKS, ids=[f"{b[0]}to{b[1]}_s{b[2]}_gw{b[3]}" + (f"_meta{b[4]}" if b[4] else "") for b in BLOCKS])
def test_one_block_against_the_fp64_restatement(cuda, win, wout, stride, gw, m, h, w):
    torch.manual_seed(win + wout)
    wrap = nn.Module()
    wrap.backbone = nn.Module()
    wrap.backbone.blk = rgn.YBlock(win, wout, stride, gw)
    R.he_fixture_(wrap, last_bn=1.0).eval()
    blk = wrap.backbone.blk
    sd = {k: v.double() for k, v in blk.state_dict().items()}
    g = torch.Generator().manual_seed(7 * h + w)
    x = torch.randn(2, win, h, w, generator=g).abs()                                       # a block's input is a ReLU output
    meta = torch.randn(2, m, h, w, generator=g) if m else None
    xin = x.double() if m == 0 else torch.cat([x[:, :-m].double(), meta.double()], 1)
    with torch.no_grad():
        want = R.y_block(xin, {"b." + k: v for k, v in sd.items()}, "b")
        gates = R.se_gate(F.relu(R._bn(F.conv2d(F.relu(R._bn(F.conv2d(xin, sd["f.a.0.weight"]), sd, "f.a.1")), sd["f.b.0.weight"], None, stride, 1, 1,
                                                         wout // gw), sd, "f.b.1")), sd, "f.se")
    host = _host()
    name = f"test.{win}.{wout}.{h}.{w}"
    sn.set_conv_precision("fp32")
    with torch.no_grad():
        got = rgn.y_block_forward(host, name, blk.to(cuda), x.to(cuda), None if m == 0 else meta.to(cuda)).cpu()
    assert got.shape == want.shape == (2, wout, (h + stride - 1) // stride, (w + stride - 1) // stride)
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f"err {err:.2e} (bar {bar:.2e}), max|want| {float(want.abs().max()):.3g}, gates {float(gates.mean()):.2f} +- {float(gates.std()):.2f}")
    assert err <= bar
    assert float(gates.std()) > 0.02                                                       # the SE is not a constant on this fixture
    for key in [k for k in host._packed if k.startswith(name)] + [k for k in host._regnet_cache if k.startswith(name)]:
        host._packed.pop(key, None)
        host._regnet_cache.pop(key, None)


# ---------------- 4. the models ----------------
_REFERENCE = {}


def _case(case):
    """(model on the CPU, x, meta, fp64 restatement output), computed once per case."""
    if case[0] not in _REFERENCE:
        _, kind, backbone, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(kind), backbone, config, classes)
        if gname is None:
            x, meta = R.inputs(config, b, h, w, seed)
        else:
            g = golden(gname)
            assert np.allclose(R.sd_digest(model.state_dict()), g["sd_digest"], rtol=1e-10)
            x, meta = _t(g["x"]), _t(g["meta"])
        want = R.forward(kind, model.state_dict(), x, meta, config, dtype=torch.float64)
        if gname is not None:      # the reference's own class produced the golden; the restatement agrees with it (test_regnet_cpu.py)
            assert float((want - _t(golden(gname)["out"]).double()).abs().max()) <= 1e-6 * R.scale_of(want)
        _REFERENCE[case[0]] = (model, x, meta, want)
    return _REFERENCE[case[0]]


def _compare(y, want, tag):
    s = R.scale_of(want)
    err = float((y.double() - want).abs().max())
    fl = R.flips(y, want)
    print(f"{tag}: S = {s:.3g}, err = {err / s:.2e} S, flips = {fl:.2e}")
    return err / s, fl


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_models_against_the_fp64_restatement(cuda, case, prec):
    """'f16x3': split-fp16 products in the dense convs (stem, the blocks' 1x1 convs, FPN blocks, head); the grouped convs stay exact fp32.  The
    same bar."""
    model, x, meta, want = _case(case)
    m = copy.deepcopy(model).to(cuda)
    sn.set_conv_precision(prec)
    try:
        with torch.no_grad():
            y = m(x.to(cuda), meta.to(cuda)).cpu()
    finally:
        sn.set_conv_precision("fp32")
    assert y.shape == want.shape
    err, fl = _compare(y, want, f"{case[0]} {prec}")
    assert err <= 1e-3 and fl <= 1e-3


# ---------------- 5. it runs on the new path ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_block_kernels_are_the_path_and_follow_the_parameters(cuda, kind, monkeypatch):
    case = next(c for c in CASES if c[1] == kind and c[9] is not None)
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    lib = _lib.load()
    counts = {"gconv": 0, "gate": 0, "sample": 0}
    real = {"gconv": lib.slu_regnet_gconv_fwd, "gate": lib.slu_regnet_se_gate, "sample": lib.slu_regnet_sample2}

    def counted(key):
        def f(*a):
            counts[key] += 1
            return real[key](*a)
        return f

    def boom(*a, **k):
        raise AssertionError("the composed path was taken")
    monkeypatch.setattr(lib, "slu_regnet_gconv_fwd", counted("gconv"))
    monkeypatch.setattr(lib, "slu_regnet_se_gate", counted("gate"))
    monkeypatch.setattr(lib, "slu_regnet_sample2", counted("sample"))
    monkeypatch.setattr(ops, "global_avgpool", boom)
    monkeypatch.setattr(ops, "se_scale", boom)
    monkeypatch.setattr(ops, "space_to_depth2", boom)
    monkeypatch.setattr(ops, "space_to_depth2_cat", boom)
    blocks = sum(R.DEPTHS[case[2]])
    with torch.no_grad():
        y0 = m(xd, md)
        assert counts == {"gconv": blocks, "gate": blocks, "sample": 4}
        m.layer3[1].f.se.fc2.bias.add_(0.5)                                 # read in place: no cache to follow
        y1 = m(xd, md)
        m.layer2[0].f.b[1].weight.mul_(1.5)                                 # in place: the folded f.b cache must notice
        y2 = m(xd, md)
        m.layer1[1].f.c[0].weight.mul_(1.25)                                # ... and the packed 1x1 cache
        y3 = m(xd, md)
    assert counts == {"gconv": 4 * blocks, "gate": 4 * blocks, "sample": 16}
    assert min(float((b - a).abs().max()) for a, b in ((y0, y1), (y1, y2), (y2, y3))) > 1e-4
    fresh = copy.deepcopy(m)
    for name in ("_packed", "_regnet_cache"):
        fresh.__dict__.pop(name, None)
    with torch.no_grad():
        assert torch.equal(fresh(xd, md), y3)


# ---------------- 6. precisions and modes ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_precisions_and_modes(cuda, kind):
    case = next(c for c in CASES if c[1] == kind and c[9] is not None)
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="resnet18 / resnet34"):
            m(xd, md)
    finally:
        sn.set_conv_precision("fp32")
    with pytest.raises(NotImplementedError, match=case[2]):
        m(xd, md)                                            # gradients enabled, parameters require them
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=case[2]):
        m(xd, md)                                            # train mode
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(x, meta)                                           # CPU tensors: no fallback
    with torch.no_grad():
        assert m(xd, md).shape == (1, 5, 32, 64)


# ---------------- 7. MC dropout on the _opt model ----------------
def test_mc_dropout_on_the_opt_model(cuda):
    """T = 4 stacked passes: they differ, match the fp64 restatement given the multipliers the stacked pass draws, and mc_predict reduces exactly
    what mc_forward stacks.  share_prefix=True is refused."""
    case = next(c for c in CASES if c[1] == "opt" and c[9] is None)
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    x1, meta1 = x[:1], meta[:1]
    xd, md = x1.to(cuda), meta1.to(cuda)
    t = 4
    c = m.decoder_semantic[0].in_channels
    torch.manual_seed(5)
    s = torch.nn.functional.dropout2d(torch.ones((t, c, 1, 1), dtype=torch.float32, device=cuda), 0.1, True).reshape(t, c)
    assert int((s == 0).sum()) > 0
    torch.manual_seed(5)
    logits = mc_forward(m, [xd, md], T=t)                                                   # [T, 1, classes, H, W]
    assert not m.dropout_pyramid.training and not m.training
    assert logits.shape[:2] == (t, 1)
    assert float((logits[0] - logits[1]).abs().max()) > 1e-3                                # the passes differ
    sd = model.state_dict()
    want = torch.stack([R.forward("opt", sd, x1, meta1, case[3], dtype=torch.float64, dropout_scale=s[i:i + 1].cpu()) for i in range(t)])
    scale = R.scale_of(want)
    err_pass = float((logits.cpu().double() - want).abs().max()) / scale
    print(f"S = {scale:.3g}: passes {err_pass:.2e} S")
    assert err_pass <= 1e-3
    torch.manual_seed(5)
    pred = mc_predict(m, [xd, md], T=t)
    stacked = ops.mc_reduce(logits.contiguous())
    assert len(pred) == len(stacked) and all(torch.equal(a, b) for a, b in zip(pred, stacked))
    with pytest.raises(RuntimeError, match="stacked schedule"):
        mc_predict(m, [xd, md], T=t, share_prefix=True)
    with pytest.raises(RuntimeError, match="stacked schedule"):
        m.forward_mc(xd, md, t)
    assert not m.dropout_pyramid.training
