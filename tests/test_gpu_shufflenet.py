"""GPU: the ShuffleNetV2 unit tail kernel (slu_shuffle_tail_fwd), the channel-offset source of the fused conv, and both FPN classes on the four
ShuffleNetV2 encoders against the fp64 restatement (tests/shufflenet_restatement.py) and the goldens of the reference's own classes.

Bars: kernels -- the exact-fp32 conv bar of test_gpu_conv.py, err <= 1e-4 max(1, max|want|), against an fp64 composition of F.conv2d; models --
err <= 1e-3 S and at most 1e-3 of the pixels with another argmax, S = max(1, max|want|) (the CPU fp32 run of the restatement is within 1.1e-5 S
and flips no pixel on these fixtures: test_shufflenet_cpu.py::test_fixture_conditions)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shufflenet_restatement as R
from conftest import golden
from semanticlidarunc_amd import _lib, ops, salsanext as sn
from semanticlidarunc_amd.ops import ConvSource
from semanticlidarunc_amd.utils.mc_dropout import mc_predict

pytestmark = pytest.mark.gpu

CASES = R.model_cases()


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ---------------- 1. the tail kernel ----------------
def _tail_problem(n, c, co, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    wdw = torch.randn(c, 9, generator=g) / 3
    bdw = torch.randn(c, generator=g) * 0.1
    wpw = torch.randn(co, c, generator=g) / c ** 0.5
    bpw = torch.randn(co, generator=g) * 0.1
    return x, wdw, bdw, wpw, bpw


def _tail_want(x, wdw, bdw, wpw, bpw, stride):
    c, co = wdw.shape[0], wpw.shape[0]
    d = F.conv2d(x.double(), wdw.double().view(c, 1, 3, 3), bdw.double(), stride=stride, padding=1, groups=c)
    return F.relu(F.conv2d(d, wpw.double().view(co, c, 1, 1), bpw.double()))


TAIL_SHAPES = [(2, 24, 24, 9, 70, 1, None), (2, 24, 24, 9, 37, 2, None), (3, 58, 58, 5, 33, 1, None), (2, 116, 116, 6, 20, 2, 6),
               (2, 116, 116, 6, 20, 2, 3), (1, 122, 122, 1, 1, 1, None), (1, 488, 488, 4, 8, 1, None), (1, 488, 488, 4, 8, 2, None),
               (1, 48, 96, 8, 16, 2, None), (1, 58, 58, 32, 1024, 1, None)]


@pytest.mark.parametrize("n,c,co,h,w,stride,m", TAIL_SHAPES, ids=[f"N{s[0]}_{s[1]}to{s[2]}_{s[3]}x{s[4]}_s{s[5]}" + (f"_meta{s[6]}" if s[6] else "") for s in TAIL_SHAPES])
def test_tail_kernel(cuda, n, c, co, h, w, stride, m):
    x, wdw, bdw, wpw, bpw = _tail_problem(n, c, co, h, w, 100 + c + h)
    want = _tail_want(x, wdw, bdw, wpw, bpw, stride)
    ho, wo = want.shape[2:]
    assert (ho, wo) == ((h + stride - 1) // stride, (w + stride - 1) // stride)
    dev = [t.to(cuda) for t in (wdw, bdw, wpw, bpw)]
    wpack = ops.pack_shuffle_tail_weight(dev[2])
    g = torch.Generator().manual_seed(5)
    pattern = torch.randn(n, 2 * co, ho, wo, generator=g)
    if m:      # two-source input x[:, :c - m] (+) meta: the first tensor keeps its c channels, the last m are not read
        first = torch.cat([x[:, :c - m], torch.full((n, m, h, w), float("nan"))], 1).to(cuda)
        kw = dict(cuse=c - m, src2=x[:, c - m:].contiguous().to(cuda))
    else:
        first, kw = x.to(cuda), {}
    bar = 1e-4 * max(1.0, float(want.abs().max()))
    for parity in (0, 1):
        out = pattern.clone().to(cuda)
        got = ops.shuffle_tail(first, dev[0], dev[1], wpack, dev[3], co, stride, out=out, parity=parity, **kw)
        assert got is out
        got = got.cpu()
        err = float((got[:, parity::2].double() - want).abs().max())
        print(f"parity {parity}: err {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        assert torch.equal(got[:, 1 - parity::2], pattern[:, 1 - parity::2])              # the other parity is untouched
        again = ops.shuffle_tail(first, dev[0], dev[1], wpack, dev[3], co, stride, out=pattern.clone().to(cuda), parity=parity, **kw).cpu()
        assert torch.equal(again, got)                                                       # bit-identical run to run
    # the pass-through half in the same launch (wider than co: only its first co channels are copied)
    p = torch.randn(n, co + 3, ho, wo, generator=g)
    got = ops.shuffle_tail(first, dev[0], dev[1], wpack, dev[3], co, stride, passthrough=p.to(cuda), **kw).cpu()
    assert torch.equal(got[:, 0::2], p[:, :co])
    assert float((got[:, 1::2].double() - want).abs().max()) <= bar


def test_tail_reads_a_channel_range(cuda):
    """src[:, coff:coff + cuse] (+) src2: what a caller with a wider tensor passes."""
    n, c, co, h, w = 2, 20, 24, 7, 19
    x, wdw, bdw, wpw, bpw = _tail_problem(n, c, co, h, w, 7)
    want = _tail_want(x, wdw, bdw, wpw, bpw, 1)
    wide = torch.cat([torch.full((n, 5, h, w), float("nan")), x[:, :16], torch.full((n, 2, h, w), float("nan"))], 1)
    dev = [t.to(cuda) for t in (wdw, bdw, wpw, bpw)]
    got = ops.shuffle_tail(wide.to(cuda), dev[0], dev[1], ops.pack_shuffle_tail_weight(dev[2]), dev[3], co, 1, coff=5, cuse=16,
                           src2=x[:, 16:].contiguous().to(cuda), passthrough=torch.zeros(n, co, h, w, device=cuda)).cpu()
    assert float((got[:, 1::2].double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert not bool(got[:, 0::2].any())


def test_tail_refusals(cuda):
    n, c, co, h, w = 1, 24, 24, 4, 8
    x, wdw, bdw, wpw, bpw = (t.to(cuda) for t in _tail_problem(n, c, co, h, w, 3))
    wpack = ops.pack_shuffle_tail_weight(wpw)
    ok = ops.shuffle_tail(x, wdw, bdw, wpack, bpw, co, 1, passthrough=x)
    assert ok.shape == (n, 2 * co, h, w)
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x.cpu(), wdw, bdw, wpack, bpw, co, 1)                              # CPU tensor
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x.double(), wdw, bdw, wpack, bpw, co, 1)                           # wrong dtype
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x.transpose(2, 3), wdw, bdw, wpack, bpw, co, 1)                    # non-contiguous
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw[:-1].contiguous(), bdw, wpack, bpw, co, 1)                  # mis-sized depthwise weight
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw, bdw, wpack[:-64].contiguous(), bpw, co, 1)                 # mis-sized packed weight
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw, bdw, wpack, bpw[:-1].contiguous(), co, 1)                  # mis-sized bias
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw, bdw, wpack, bpw, co, 3)                                    # stride
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw, bdw, wpack, bpw, co, 1, out=torch.empty(n, 2 * co, h, w + 1, device=cuda))
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(x, wdw, bdw, wpack, bpw, co, 1, parity=0, passthrough=x)           # the pass-through half owns the even channels
    # more output channels than the library instantiates: its "not instantiated" code, never a silent wrong answer
    assert _lib.load().slu_shuffle_tail_packed_floats(520, 24) == 0
    with pytest.raises(_lib.SluError, match="-2"):
        ops.pack_shuffle_tail_weight(torch.zeros(520, 24, device=cuda))
    d = _lib.ShuffleTailDesc()
    out = torch.empty(n, 2 * 520, h, w, device=cuda)
    d.src0, d.ct0, d.c0, d.N, d.H, d.W, d.stride, d.Co, d.parity = x.data_ptr(), c, c, n, h, w, 1, 520, 1
    d.wdw, d.bdw, d.wpack, d.bpw, d.out = wdw.data_ptr(), bdw.data_ptr(), wpack.data_ptr(), bpw.data_ptr(), out.data_ptr()
    import ctypes
    assert _lib.load().slu_shuffle_tail_fwd(ctypes.byref(d), None) == -2


# ---------------- 2. channel-offset source of the 1x1 conv ----------------
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_conv_reads_the_second_half_of_its_source(cuda, prec):
    """x[:, C/2:] as the source of the 1x1 conv: the range ends with the last image's last channel, i.e. where the tensor ends (it is exactly as
    large as the kernel's last legal access, odd H W so the ragged last K-chunk is on the unaligned path), and the half in front of the range is
    NaN so that a read before it poisons the result."""
    n, c, h, w = 3, 116, 5, 33
    half = c // 2
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(half, half, 1, 1, generator=g) / half ** 0.5
    b = torch.randn(half, generator=g) * 0.1
    want = F.relu(F.conv2d(x[:, half:].double(), wt.double(), b.double()))
    xd = x.to(cuda)
    xd[:, :half] = float("nan")                                                              # the half that must not be read
    pack = ops.pack_conv_weight_f16x3(wt.to(cuda)) if prec == "f16x3" else ops.pack_conv_weight(wt.to(cuda))
    got = ops.conv2d_fused([ConvSource(xd, None, False, 0, half, half)], pack, half, 1, 1, 0, bias=b.to(cuda), precision=prec, act="relu").cpu()
    err = float((got.double() - want).abs().max())
    assert err <= 1e-4 * max(1.0, float(want.abs().max())), err
    with pytest.raises(RuntimeError):
        ops.conv2d_fused([ConvSource(xd, None, False, 0, half, half + 1)], pack, half, 1, 1, 0)       # range past the last channel
    with pytest.raises(RuntimeError):
        ops.conv2d_fused([ConvSource(xd, None, False, 0, 0, half)], pack, half, 1, 1, 0)              # an offset needs a count


# ---------------- 3. the models ----------------
_REFERENCE = {}


def _case(case):
    """(model on the CPU, x, meta, fp64 restatement output), computed once per case."""
    if case[0] not in _REFERENCE:
        _, kind, width, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(kind), width, config, classes)
        if gname is None:
            x, meta = R.inputs(config, b, h, w, seed)
        else:
            g = golden(gname)
            assert np.allclose(R.sd_digest(model.state_dict()), g["sd_digest"], rtol=1e-10)
            x, meta = _t(g["x"]), _t(g["meta"])
        want = R.forward(kind, model.state_dict(), x, meta, config, dtype=torch.float64)
        if gname is not None:      # the reference's own class produced the golden; the restatement agrees with it (test_shufflenet_cpu.py)
            assert float((want - _t(golden(gname)["out"]).double()).abs().max()) <= 1e-6 * R.scale_of(want)
        _REFERENCE[case[0]] = (model, x, meta, want)
    return _REFERENCE[case[0]]


def _compare(y, want, tag):
    s = R.scale_of(want)
    err = float((y.double() - want).abs().max())
    fl = R.flips(y, want)
    print(f"{tag}: S = {s:.3g}, err = {err / s:.2e} S, flips = {fl:.2e}")
    return err / s, fl


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_models_against_the_fp64_restatement(cuda, case):
    model, x, meta, want = _case(case)
    m = copy.deepcopy(model).to(cuda)
    with torch.no_grad():
        y = m(x.to(cuda), meta.to(cuda)).cpu()
    assert y.shape == want.shape
    err, fl = _compare(y, want, case[0])
    assert err <= 1e-3 and fl <= 1e-3


@pytest.mark.parametrize("case", CASES[:16], ids=[c[0] for c in CASES[:16]])
def test_models_under_f16x3(cuda, case):
    """Split-fp16 products in the dense convs (the unit tails stay exact fp32): the fp32 bar."""
    model, x, meta, want = _case(case)
    m = copy.deepcopy(model).to(cuda)
    sn.set_conv_precision("f16x3")
    try:
        with torch.no_grad():
            y = m(x.to(cuda), meta.to(cuda)).cpu()
    finally:
        sn.set_conv_precision("fp32")
    err, fl = _compare(y, want, case[0] + " f16x3")
    assert err <= 1e-3 and fl <= 1e-3


# ---------------- 4. it runs on the new path ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_fused_tail_is_the_path_and_follows_the_parameters(cuda, kind, monkeypatch):
    case = next(c for c in CASES if c[1] == kind and c[2] == R.WIDTHS[0] and c[3] == "m6_att_msm" and c[9] is None and c[5:7] == (32, 64))
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)

    def boom(*a, **k):
        raise AssertionError("the composed path was taken")
    monkeypatch.setattr(ops, "dwconv3x3", boom)
    monkeypatch.setattr(torch, "cat", boom)
    with torch.no_grad():
        y0 = m(xd, md)
        with torch.no_grad():
            m.layer2[1].branch2[3].weight.mul_(1.5)
        y1 = m(xd, md)
        m.layer1[0].branch1[1].running_var.add_(0.5)
        y2 = m(xd, md)
    assert float((y1 - y0).abs().max()) > 1e-3 and float((y2 - y1).abs().max()) > 1e-3
    fresh = copy.deepcopy(m)
    for name in ("_packed", "_shf_cache", "_dw_cache"):
        fresh.__dict__.pop(name, None)
    with torch.no_grad():
        assert torch.equal(fresh(xd, md), y2)


# ---------------- 5. precisions and modes ----------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_precisions_and_modes(cuda, kind):
    case = next(c for c in CASES if c[1] == kind and c[2] == R.WIDTHS[0] and c[3] == "m3_plain" and c[9] is None)
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x.to(cuda), meta.to(cuda)
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="resnet18 / resnet34"):
            m(xd, md)
    finally:
        sn.set_conv_precision("fp32")
    with pytest.raises(NotImplementedError, match="shufflenet_v2_x0_5"):
        m(xd, md)                                            # gradients enabled, parameters require them
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="shufflenet_v2_x0_5"):
        m(xd, md)                                            # train-mode BatchNorm
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(x, meta)                                           # CPU tensors: no fallback
    with torch.no_grad():
        assert m(xd, md).shape == (x.shape[0], 20, 32, 64)


# ---------------- 6. MC dropout on the _opt model ----------------
def test_mc_dropout_on_the_opt_model(cuda):
    """mc_predict (stacked schedule) against three single forwards with the multipliers the stacked pass draws.  The passes are the same
    arithmetic per image; the conv tile choice may differ between N = 3 and N = 1, so the bars are those of test_gpu_fpn_opt_mc.py."""
    case = next(c for c in CASES if c[1] == "opt" and c[2] == R.WIDTHS[0] and c[3] == "m6_att_msm" and c[9] is None and c[5:7] == (32, 64))
    model, x, meta, _ = _case(case)
    m = copy.deepcopy(model).to(cuda)
    xd, md = x[:1].to(cuda), meta[:1].to(cuda)
    t = 3
    c = m.decoder_semantic[0].in_channels
    torch.manual_seed(5)
    s = torch.nn.functional.dropout2d(torch.ones((t, c, 1, 1), dtype=torch.float32, device=cuda), 0.1, True).reshape(t, c)
    assert int((s == 0).sum()) > 0
    with torch.no_grad():
        logits = torch.stack([m.forward_with_dropout_scale(xd, md, s[i:i + 1].contiguous()) for i in range(t)])
    want = ops.mc_reduce(logits.contiguous())
    torch.manual_seed(5)
    got = mc_predict(m, [xd, md], T=t)
    assert not m.dropout_pyramid.training and not m.training
    d = [float((got[i] - want[i]).abs().max()) for i in range(3)]
    top = want[0].topk(2, dim=1).values
    undecided = (top[:, 0] - top[:, 1]) <= 1e-4
    print(f"p_bar {d[0]:.2e} H {d[1]:.2e} MI {d[2]:.2e}")
    assert d[0] <= 2e-6 and d[1] <= 2e-5 and d[2] <= 2e-5
    assert not bool(((got[3] != want[3]) & ~undecided).any())
    assert float((logits[0] - logits[1]).abs().max()) > 1e-3                                # the passes differ
    # the shared-prefix schedule is identical to the strict one or refused, never silently different
    torch.manual_seed(5)
    try:
        shared = mc_predict(m, [xd, md], T=t, share_prefix=True)
    except RuntimeError:
        shared = None
    if shared is not None:
        assert all(torch.equal(a, b) for a, b in zip(shared, got))
    assert not m.dropout_pyramid.training
