"""GPU: the Fire module kernel (slu_fire_fwd), the ceil-mode max-pool (slu_maxpool3s2_ceil_fwd) and both FPN classes on the SqueezeNet 1.0 encoder
against the fp64 restatement (tests/squeezenet_restatement.py) and the goldens of the reference's own classes.

Bars: Fire kernel -- the exact-fp32 conv bar of test_gpu_conv.py, err <= 1e-4 max(1, max|want|), against an fp64 composition of F.conv2d; pool --
exact equality; models -- err <= 1e-3 S and at most 1e-3 of the pixels with another argmax, S = max(1, max|want|), under 'fp32' and 'f16x3' (the
CPU fp32 run of the restatement is within 2e-6 S and flips no pixel on these fixtures: test_squeezenet_cpu.py::test_fixture_conditions)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import squeezenet_restatement as R
from conftest import golden
from semanticlidarunc_amd import _lib, ops, salsanext as sn
from semanticlidarunc_amd.utils.mc_dropout import mc_forward, mc_predict

pytestmark = pytest.mark.gpu

CASES = R.model_cases()


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ---------------- 1. the Fire kernel ----------------
def _fire_problem(n, cin, s, e1, e3, h, w, seed):
    """He-drawn weights, N(0, 0.1) biases."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wsq = torch.randn(s, cin, generator=g) * (2.0 / cin) ** 0.5
    w1 = torch.randn(e1, s, generator=g) * (2.0 / s) ** 0.5
    w3 = torch.randn(e3, s, 3, 3, generator=g) * (2.0 / (9 * s)) ** 0.5
    bsq, b1, b3 = (torch.randn(c, generator=g) * 0.1 for c in (s, e1, e3))
    return x, wsq, w1, w3, bsq, b1, b3


def _fire_want(x, wsq, w1, w3, bsq, b1, b3):
    s, cin = wsq.shape
    sq = F.relu(F.conv2d(x.double(), wsq.double().view(s, cin, 1, 1), bsq.double()))
    return torch.cat([F.relu(F.conv2d(sq, w1.double().view(-1, s, 1, 1), b1.double())), F.relu(F.conv2d(sq, w3.double(), b3.double(), padding=1))], 1)


def _fire_run(cuda, x, wsq, w1, w3, bsq, b1, b3, **kw):
    d = [t.to(cuda) for t in (wsq, w1, w3, bsq, b1, b3)]
    return ops.fire(x.to(cuda) if isinstance(x, torch.Tensor) and not x.is_cuda else x, ops.pack_fire_weight(d[0], d[1], d[2]), d[3], d[4], d[5], **kw)


# (N, Cin, S, E1, E3, H, W, channels of the second source)
FIRE_SHAPES = [(1, 96, 16, 64, 64, 1, 1, 0), (2, 13, 10, 20, 36, 5, 7, 0), (1, 128, 32, 128, 128, 9, 70, 0), (2, 256, 48, 192, 192, 6, 33, 6),
               (1, 512, 64, 256, 256, 4, 16, 0), (1, 96, 16, 64, 64, 2, 1024, 0)]


@pytest.mark.parametrize("n,cin,s,e1,e3,h,w,m", FIRE_SHAPES, ids=[f"N{c[0]}_{c[1]}_s{c[2]}_e{c[3]}+{c[4]}_{c[5]}x{c[6]}" + (f"_meta{c[7]}" if c[7] else "")
                                                                 for c in FIRE_SHAPES])
def test_fire_kernel(cuda, n, cin, s, e1, e3, h, w, m):
    """The kernel's constants: 4 x 32 output tile, 6 x 34 squeeze halo in LDS, K chunks of 32 input channels in the squeeze and of 16 squeeze
    channels in the expand convs (the packed weights zero-pad Cin to a multiple of 32 and S to a multiple of 16), 32-channel output blocks,
    output blocks split over up to 4 workgroups when there are fewer than 256 tiles.  The tile does not exceed 8 x 64.
      1 x 1           the smallest map: every halo position but the centre is outside the image
      2 x 13.. 5 x 7  ragged everything (Cin 13, S 10, E1 20, E3 36: no multiple of 16 or 32, odd S), batch stride
      9 x 70          crosses tile edges both ways (3 tile rows, 3 tile columns), neither a multiple of the tile: interior halos from real input
      250 + 6         two sources, coff0 = 0, ct0 = 256: the first tensor's last 6 channels are NaN and must not be read
      512 / 64 / 256  the LDS (52 224 B) and channel maxima, two squeeze row blocks, 8 + 8 output blocks split over 4 workgroups
      2 x 1024        a long row: 32 tile columns, a tile row with two of its four rows outside the image"""
    x, wsq, w1, w3, bsq, b1, b3 = _fire_problem(n, cin, s, e1, e3, h, w, 100 + cin + h)
    want = _fire_want(x, wsq, w1, w3, bsq, b1, b3)
    kw = {}
    first = x
    if m:
        first = torch.cat([x[:, :cin - m], torch.full((n, m, h, w), float("nan"))], 1)
        kw = dict(cuse=cin - m, src2=x[:, cin - m:].contiguous().to(cuda))
    got = _fire_run(cuda, first, wsq, w1, w3, bsq, b1, b3, **kw)
    assert got.shape == want.shape
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    err = float((got.cpu().double() - want).abs().max())
    print(f"err {err:.2e} (bar {bar:.2e}), max|want| {float(want.abs().max()):.3g}")
    assert err <= bar
    again = _fire_run(cuda, first, wsq, w1, w3, bsq, b1, b3, **kw)
    assert torch.equal(again, got)                                                           # bit-identical run to run


def test_fire_leaky_halo_would_be_seen(cuda):
    """The wrong kernel the bar must catch: relu(bsq) instead of 0 outside the image moves a 5 x 7 Fire by far more than the bar."""
    x, wsq, w1, w3, bsq, b1, b3 = _fire_problem(2, 13, 10, 20, 36, 5, 7, 118)
    want = _fire_want(x, wsq, w1, w3, bsq, b1, b3)
    sd = {"f.squeeze.weight": wsq.double().view(10, 13, 1, 1), "f.squeeze.bias": bsq.double(), "f.expand1x1.weight": w1.double().view(20, 10, 1, 1),
          "f.expand1x1.bias": b1.double(), "f.expand3x3.weight": w3.double(), "f.expand3x3.bias": b3.double()}
    assert float((R.fire(x.double(), sd, "f") - want).abs().max()) <= 1e-12
    leaky = float((R.fire(x.double(), sd, "f", leaky_halo=True) - want).abs().max())
    got = _fire_run(cuda, x, wsq, w1, w3, bsq, b1, b3).cpu().double()
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    print(f"leaky halo moves the output by {leaky:.3g}, bar {bar:.2e}")
    assert leaky > 100 * bar and float((got - want).abs().max()) <= bar


def test_fire_reads_a_channel_range(cuda):
    """src[:, coff:coff + cuse] (+) src2 with coff > 0: what a caller with a wider tensor passes."""
    n, cin, s, e1, e3, h, w = 2, 20, 12, 24, 40, 7, 37
    x, wsq, w1, w3, bsq, b1, b3 = _fire_problem(n, cin, s, e1, e3, h, w, 7)
    want = _fire_want(x, wsq, w1, w3, bsq, b1, b3)
    wide = torch.cat([torch.full((n, 5, h, w), float("nan")), x[:, :16], torch.full((n, 2, h, w), float("nan"))], 1)
    got = _fire_run(cuda, wide, wsq, w1, w3, bsq, b1, b3, coff=5, cuse=16, src2=x[:, 16:].contiguous().to(cuda)).cpu()
    assert float((got.double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_fire_refusals(cuda):
    n, cin, s, e1, e3, h, w = 1, 24, 16, 32, 32, 4, 8
    x, wsq, w1, w3, bsq, b1, b3 = (t.to(cuda) for t in _fire_problem(n, cin, s, e1, e3, h, w, 3))
    wpack = ops.pack_fire_weight(wsq, w1, w3)
    assert ops.fire(x, wpack, bsq, b1, b3).shape == (n, e1 + e3, h, w)
    lib = _lib.load()
    # S = 65 and E3 = 257: the library's "not instantiated" code from every entry point, never a launch
    assert lib.slu_fire_packed_floats(cin, 65, e1, e3) == 0 and lib.slu_fire_packed_floats(cin, s, e1, 257) == 0
    assert lib.slu_fire_packed_floats(cin, 64, 256, 256) > 0
    with pytest.raises(_lib.SluError, match="-2"):
        ops.pack_fire_weight(torch.zeros(65, cin, device=cuda), torch.zeros(e1, 65, device=cuda), torch.zeros(e3, 65, 3, 3, device=cuda))
    with pytest.raises(_lib.SluError, match="-2"):
        ops.pack_fire_weight(wsq, w1, torch.zeros(257, s, 3, 3, device=cuda))
    with pytest.raises(RuntimeError):
        ops.fire(x, wpack, torch.zeros(65, device=cuda), b1, b3)
    with pytest.raises(RuntimeError):
        ops.fire(x, wpack, bsq, b1, torch.zeros(257, device=cuda))
    d = _lib.FireDesc()
    out = torch.full((n, e1 + 257, h, w), 7.0, device=cuda)
    d.src0, d.ct0, d.c0, d.N, d.H, d.W = x.data_ptr(), cin, cin, n, h, w
    d.wpack, d.bsq, d.b1, d.b3, d.out = wpack.data_ptr(), bsq.data_ptr(), b1.data_ptr(), b3.data_ptr(), out.data_ptr()
    d.S, d.E1, d.E3 = s, e1, 257
    assert lib.slu_fire_fwd(ctypes.byref(d), None) == -2
    d.S, d.E3 = 65, e3
    assert lib.slu_fire_fwd(ctypes.byref(d), None) == -2
    # out aliasing src0: SLU_EINVAL from the library, RuntimeError from the wrapper
    big = torch.full((n, e1 + e3, h, w), 7.0, device=cuda)
    d.S, d.src0, d.ct0, d.out = s, big.data_ptr(), e1 + e3, big.data_ptr()
    assert lib.slu_fire_fwd(ctypes.byref(d), None) == -1
    with pytest.raises(RuntimeError, match="overlap"):
        ops.fire(big, wpack, bsq, b1, b3, out=big, cuse=cin)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((big == 7.0).all())                             # nothing was launched
    with pytest.raises(RuntimeError):
        ops.fire(x.cpu(), wpack, bsq, b1, b3)                                                # CPU tensor
    with pytest.raises(RuntimeError):
        ops.fire(x.transpose(2, 3), wpack, bsq, b1, b3)                                      # non-contiguous
    with pytest.raises(RuntimeError):
        ops.fire(x, wpack[:-64].contiguous(), bsq, b1, b3)                                   # mis-sized packed weight
    with pytest.raises(RuntimeError):
        ops.fire(x, wpack, bsq, b1, b3, out=torch.empty(n, e1 + e3, h, w + 1, device=cuda))


# ---------------- 2. the ceil-mode pool ----------------
@pytest.mark.parametrize("h", [3, 4, 5, 7, 8])
@pytest.mark.parametrize("w", [3, 4, 5, 7, 8])
def test_ceil_pool_is_exact(cuda, h, w):
    x = torch.randn(2, 5, h, w, generator=torch.Generator().manual_seed(h * 10 + w))
    want = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    got = ops.maxpool3s2_ceil(x.to(cuda)).cpu()
    assert got.shape == want.shape and torch.equal(got, want)


def test_ceil_pool_two_sources_and_refusals(cuda):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 16, 48, generator=g)
    want = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    first = torch.cat([x[:, :3], torch.full((2, 2, 16, 48), float("nan"))], 1)
    got = ops.maxpool3s2_ceil(first.to(cuda), cuse=3, src2=x[:, 3:].contiguous().to(cuda)).cpu()
    assert got.shape == (2, 5, 8, 24) and torch.equal(got, want)
    assert not torch.equal(want, F.max_pool2d(x, 3, 2, 1))                                   # same size, other windows: another operator
    with pytest.raises(RuntimeError):
        ops.maxpool3s2_ceil(torch.zeros(1, 2, 2, 8, device=cuda))                            # H = 2
    xd = x.to(cuda)
    assert _lib.load().slu_maxpool3s2_ceil_fwd(ctypes.byref(_lib.Cat2(xd.data_ptr(), None, 5, 0, 5, 0, 0)), xd.data_ptr(), 2, 2, 48, None) == -1


# ---------------- 3. the models ----------------
_REFERENCE = {}


def _case(case):
    """(model on the CPU, x, meta, fp64 restatement output), computed once per case."""
    if case[0] not in _REFERENCE:
        _, kind, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(kind), config, classes)
        if gname is None:
            x, meta = R.inputs(config, b, h, w, seed)
        else:
            g = golden(gname)
            assert np.allclose(R.sd_digest(model.state_dict()), g["sd_digest"], rtol=1e-10)
            x, meta = _t(g["x"]), _t(g["meta"])
        want = R.forward(kind, model.state_dict(), x, meta, config, dtype=torch.float64)
        if gname is not None:      # the reference's own class produced the golden; the restatement agrees with it (test_squeezenet_cpu.py)
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
    """'f16x3': split-fp16 products in the dense convs (stem, FPN blocks, head); the Fires stay exact fp32.  The same bar."""
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


# ---------------- 4. it runs on the new path ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_fused_fire_is_the_path_and_follows_the_parameters(cuda, kind, monkeypatch):
    case = next(c for c in CASES if c[1] == kind and c[2] == "m6_att_msm" and c[8] is None and c[4:6] == (32, 64))
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    lib = _lib.load()
    counts = {"fire": 0, "pool": 0}
    real_fire, real_pool = lib.slu_fire_fwd, lib.slu_maxpool3s2_ceil_fwd

    def fire(*a):
        counts["fire"] += 1
        return real_fire(*a)

    def pool(*a):
        counts["pool"] += 1
        return real_pool(*a)

    def boom(*a, **k):
        raise AssertionError("the composed path was taken")
    monkeypatch.setattr(lib, "slu_fire_fwd", fire)
    monkeypatch.setattr(lib, "slu_maxpool3s2_ceil_fwd", pool)
    monkeypatch.setattr(ops, "maxpool3s2", boom)
    monkeypatch.setattr(torch, "cat", boom)
    with torch.no_grad():
        y0 = m(xd, md)
        assert counts == {"fire": 8, "pool": 3}
        m.layer3[0].squeeze.bias.add_(0.5)                               # in place: the cache must notice
        y1 = m(xd, md)
        m.layer1[1].expand3x3.weight.mul_(1.5)
        y2 = m(xd, md)
    assert counts == {"fire": 24, "pool": 9}
    assert float((y1 - y0).abs().max()) > 1e-3 and float((y2 - y1).abs().max()) > 1e-3
    fresh = copy.deepcopy(m)
    for name in ("_packed", "_fire_cache"):
        fresh.__dict__.pop(name, None)
    with torch.no_grad():
        assert torch.equal(fresh(xd, md), y2)


# ---------------- 5. precisions and modes ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_precisions_and_modes(cuda, kind):
    case = next(c for c in CASES if c[1] == kind and c[2] == "m3_plain" and c[8] is None)
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="resnet18 / resnet34"):
            m(xd, md)
    finally:
        sn.set_conv_precision("fp32")
    with pytest.raises(NotImplementedError, match="squeezenet1_0"):
        m(xd, md)                                            # gradients enabled, parameters require them
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="squeezenet1_0"):
        m(xd, md)                                            # train mode
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(x, meta)                                           # CPU tensors: no fallback
    with torch.no_grad():
        assert m(xd, md).shape == (x.shape[0], 20, 32, 64)


# ---------------- 6. MC dropout on the _opt model ----------------
def test_mc_dropout_on_the_opt_model(cuda):
    """T = 4 stacked passes: they differ, and their mean matches the fp64 restatement given the multipliers the stacked pass draws.
    share_prefix=True is refused."""
    case = next(c for c in CASES if c[1] == "opt" and c[2] == "m6_att_msm" and c[8] is None and c[4:6] == (32, 64))
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
    logits = mc_forward(m, [xd, md], T=t).cpu()                                             # [T, 1, classes, H, W]
    assert not m.dropout_pyramid.training and not m.training
    assert logits.shape[:2] == (t, 1)
    assert float((logits[0] - logits[1]).abs().max()) > 1e-3                                # the passes differ
    sd = model.state_dict()
    want = torch.stack([R.forward("opt", sd, x1, meta1, "m6_att_msm", dtype=torch.float64, dropout_scale=s[i:i + 1].cpu()) for i in range(t)])
    scale = R.scale_of(want)
    err_pass = float((logits.double() - want).abs().max()) / scale
    err_mean = float((logits.double().mean(0) - want.mean(0)).abs().max()) / scale
    print(f"S = {scale:.3g}: passes {err_pass:.2e} S, mean {err_mean:.2e} S")
    assert err_pass <= 1e-3 and err_mean <= 1e-3
    with torch.no_grad():
        single = m.forward_with_dropout_scale(xd, md, s[2:3].contiguous()).cpu()
    assert float((single.double() - want[2]).abs().max()) <= 1e-3 * scale
    with pytest.raises(RuntimeError, match="stacked schedule"):
        mc_predict(m, [xd, md], T=t, share_prefix=True)
    with pytest.raises(RuntimeError, match="stacked schedule"):
        m.forward_mc(xd, md, t)
    assert not m.dropout_pyramid.training
