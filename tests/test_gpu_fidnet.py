"""GPU: the fused point-MLP stem and bilinear_ac_sum against fp64 on the CPU, FIDNet's commuted head against the reference order, and the
ResNet34_point model against the fp64 restatement and the outputs the reference's own class produced (tests/golden/fidnet_point_*.npz,
tools/gen_golden_fidnet.py).

Bars.  Every fp32 kernel comparison against fp64 uses  bar = max(4 e_fp32, 1e-6 max|want|)  with e_fp32 the error of the SAME computation done by
torch on the CPU in fp32, in the reference's order, against fp64: a measurement of the reference arithmetic, never of the code under test (both
numbers are printed).  point_mlp sums each dot product as one k-ordered fmaf chain, torch's CPU conv in blocks: both are a few ulp of the sum of
magnitudes.  bilinear_ac_sum: 1e-6 sum_k max|src_k| -- each term is two nested fp32 lerps with correctly rounded weights, a few ulp of its
source's magnitude, as in bilinear_ac_cat.  The commuted head is NOT bit-equal to the reference order: the reference interpolates 384 channels and
takes one 1024-term dot product per output, the model takes three 128-term dot products on the low-resolution maps, interpolates and adds them to
the 640-term one; the same real number (the four interpolation weights sum to 1) rounded along another route.  Under f16x3 its bar is 1e-5 of the
output scale, as for CENet's commuted aux head.
Model parity: 1e-3 max|logit| (the project's bar) against the restatement in fp64 and against the stored fp32 reference; the backend's
1024-channel map (ResNet_34_point.forward) is held per channel slice to 1e-3 of that slice's maximum, because the logits alone move by less than
the bar when a deep BatchNorm bias is dropped (fidnet_restatement.py).

Measured on MI355X (maxima over the cases of each test):
    point_mlp            1.11e-05 at the model's widths, where the bars are 1.7e-05 .. 5.6e-05 (e_fp32 4.3e-06 .. 1.4e-05, max|want| 8 .. 18);
                         9.3e-06 on the 32-pixel-tile chain (bars 1.1e-05 .. 3.6e-05); two runs equal bit for bit
    bilinear_ac_sum      1.46e-06 with three sources of 128 channels (bar 2.56e-05); 0 for one source at the output size
    commuted head        fp32 3.12e-06 (bar 6.34e-06 = 4 e_fp32; the composed form 5.16e-06), f16x3 5.00e-06 (bar 3.46e-05; composed 6.05e-06)
    model, of max|logit| against fp64 / against the stored reference:   fp32 2.74e-06 / 3.49e-06,   f16x3 1.48e-05 / 1.47e-05
    backend slices, of each slice's maximum:   fp32 2.42e-06,   f16x3 1.17e-05;   SemanticHead(backend(x)) against the fast route 1.46e-06"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fidnet_restatement as R
from conftest import golden
from semanticlidarunc_amd import fidnet, ops, salsanext as sn
from test_gpu_cenet import PAIR_IDS, PAIRS

pytestmark = pytest.mark.gpu

SLOPE = 0.01
# name, C0, widths
CHAINS = (("model_c3", 3, (64, 128, 256, 512)), ("model_c4", 4, (64, 128, 256, 512)), ("model_c5", 5, (64, 128, 256, 512)),
          ("model_c8", 8, (64, 128, 256, 512)), ("three_5_32_96_64", 5, (32, 96, 64)), ("one_5_64", 5, (64,)),
          ("one_32_512", 32, (512,)),                    # two full K-chunks of input channels
          ("wide_5_512_512_64", 5, (512, 512, 64)))      # two 512-channel maps of 64 pixels exceed the LDS: the 32-pixel tile
PIXELS = ((1, 1), (7, 9), (8, 8), (5, 13), (7, 13))      # 1, 63, 64, 65 and 91 pixels: below, at and above the 64-pixel tile, two tiles
N = 3
_CHAIN = {}


def _chain(ci, pi):
    """(x, weights, biases, fp64 and CPU-fp32 results with and without the last activation): built once per case and left unchanged."""
    if (ci, pi) not in _CHAIN:
        _, c0, widths = CHAINS[ci]
        g = torch.Generator().manual_seed(1000 * ci + pi)
        x = torch.randn(N, c0, *PIXELS[pi], generator=g) - 1.0                         # negative-heavy: the slope shows
        ws, bs, cin = [], [], c0
        for co in widths:
            ws.append(torch.randn(co, cin, generator=g) * (2.0 / cin) ** 0.5)
            bs.append((2.0 * torch.randint(0, 2, (co,), generator=g) - 1.0) * (0.75 + 0.5 * torch.rand(co, generator=g)))      # |b| ~ 1
            cin = co

        def run(dtype, act_last):
            t = x.to(dtype)
            for i, (w, b) in enumerate(zip(ws, bs)):
                t = F.conv2d(t, w.to(dtype)[:, :, None, None], b.to(dtype))
                if act_last or i + 1 < len(ws):
                    t = F.leaky_relu(t, SLOPE)
            return t
        _CHAIN[(ci, pi)] = (x, ws, bs, {a: (run(torch.float64, a), run(torch.float32, a)) for a in (True, False)})
    return _CHAIN[(ci, pi)]


def _bar(want64, cpu32):
    e32 = float((cpu32.double() - want64).abs().max())
    return max(4.0 * e32, 1e-6 * float(want64.abs().max())), e32


@pytest.mark.parametrize("pi", range(len(PIXELS)), ids=["%dx%d" % p for p in PIXELS])
@pytest.mark.parametrize("ci", range(len(CHAINS)), ids=[c[0] for c in CHAINS])
def test_point_mlp_matches_the_fp64_chain(cuda, ci, pi):
    x, ws, bs, ref = _chain(ci, pi)
    widths = CHAINS[ci][2]
    packed = ops.pack_point_mlp([w.to(cuda) for w in ws])
    bias = torch.cat(bs).to(cuda)
    xd = x.to(cuda)
    for act_last in (True, False):
        got = ops.point_mlp(xd, packed, bias, widths, SLOPE, act_last=act_last)
        again = ops.point_mlp(xd, packed, [b.to(cuda) for b in bs], widths, SLOPE, act_last=act_last)      # the biases as a sequence
        want, cpu32 = ref[act_last]
        bar, e32 = _bar(want, cpu32)
        err = float((got.cpu().double() - want).abs().max())
        print(f"{CHAINS[ci][0]} {PIXELS[pi]} act_last={act_last}: err {err:.2e}, e_fp32 {e32:.2e}, bar {bar:.2e}, max|want| {float(want.abs().max()):.3g}")
        assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert err <= bar
        assert torch.equal(got, again)                                                 # no atomics: bit-identical run to run
    assert not torch.equal(ref[True][0], ref[False][0])                                # the last activation is no no-op on this data


def test_point_mlp_refusals(cuda):
    x = torch.zeros(1, 5, 2, 2, device=cuda)
    w1, w2 = torch.zeros(64, 5, device=cuda), torch.zeros(32, 64, device=cuda)
    packed, bias = ops.pack_point_mlp([w1, w2]), torch.zeros(96, device=cuda)
    assert packed.numel() == ops.point_mlp_packed_floats(64, 5) + ops.point_mlp_packed_floats(32, 64)
    assert ops.pack_point_mlp([w1[:, :, None, None]]).numel() == ops.point_mlp_packed_floats(64, 5)
    with pytest.raises(RuntimeError, match="1..4 layers"):
        ops.pack_point_mlp([])
    with pytest.raises(RuntimeError, match="1..4 layers"):
        ops.pack_point_mlp([torch.zeros(32, 5, device=cuda)] + [torch.zeros(32, 32, device=cuda)] * 4)
    with pytest.raises(RuntimeError, match="do not follow"):
        ops.pack_point_mlp([w1, torch.zeros(32, 32, device=cuda)])
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.pack_point_mlp([torch.zeros(48, 5, device=cuda)])
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.pack_point_mlp([torch.zeros(544, 5, device=cuda)])
    with pytest.raises(RuntimeError, match="input channels"):
        ops.pack_point_mlp([torch.zeros(32, 33, device=cuda)])
    with pytest.raises(RuntimeError, match="does not match"):
        ops.point_mlp(x, packed, torch.zeros(128, device=cuda), [64, 64], SLOPE)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.point_mlp(torch.zeros(1, 20, 2, 2, device=cuda), packed, bias, [64, 32], SLOPE)      # two K-chunks of input channels, packed for one
    with pytest.raises(RuntimeError, match="biases"):
        ops.point_mlp(x, packed, bias[:-1], [64, 32], SLOPE)
    with pytest.raises(RuntimeError, match="biases"):
        ops.point_mlp(x, packed, [bias[:64], bias[:32], bias[:1]], [64, 32], SLOPE)
    with pytest.raises(RuntimeError, match="N, C0, H, W"):
        ops.point_mlp(x[0], packed, bias, [64, 32], SLOPE)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.point_mlp(x.permute(0, 1, 3, 2)[:, :, :, ::2], packed, bias, [64, 32], SLOPE)


# ---- bilinear_ac_sum ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (1, 3, 128))
@pytest.mark.parametrize("nsrc", (1, 2, 3))
@pytest.mark.parametrize("pi", range(len(PAIRS)), ids=PAIR_IDS)
def test_bilinear_ac_sum_matches_fp64(cuda, pi, nsrc, c):
    """Source k takes the input size of pair (pi + k): every launch with more than one source mixes input sizes, as the model's does."""
    size = PAIRS[pi][1]
    g = torch.Generator().manual_seed(100 * pi + 10 * nsrc + c)
    srcs = [torch.randn(N, c, *PAIRS[(pi + k) % len(PAIRS)][0], generator=g) * (1.0 + k) for k in range(nsrc)]
    want = sum(F.interpolate(s.double(), size=size, mode="bilinear", align_corners=True) for s in srcs)
    dev = [s.to(cuda) for s in srcs]
    got = ops.bilinear_ac_sum(dev, size)
    err, bar = float((got.cpu().double() - want).abs().max()), 1e-6 * sum(float(s.abs().max()) for s in srcs)
    print(f"{PAIR_IDS[pi]} {nsrc} sources C = {c}: err {err:.2e}, bar {bar:.2e}")
    assert got.shape == (N, c) + size and err <= bar
    assert torch.equal(got, ops.bilinear_ac_sum(dev, size))
    if nsrc == 1 and tuple(srcs[0].shape[2:]) == size:
        assert torch.equal(got.cpu(), srcs[0])                                         # the identity size gives the input back bit for bit
    if nsrc == 1:
        assert torch.equal(got, ops.bilinear_ac_cat(dev, size))                        # one term: the kernel it is derived from, bit for bit


def test_bilinear_ac_sum_refusals(cuda):
    a, b = torch.zeros(1, 2, 2, 2, device=cuda), torch.zeros(1, 2, 4, 4, device=cuda)
    with pytest.raises(RuntimeError, match="1..3 sources"):
        ops.bilinear_ac_sum([a, a, a, a], (4, 4))
    with pytest.raises(RuntimeError, match="1..3 sources"):
        ops.bilinear_ac_sum([], (4, 4))
    with pytest.raises(RuntimeError, match="batch"):
        ops.bilinear_ac_sum([a, torch.zeros(2, 2, 2, 2, device=cuda)], (4, 4))
    with pytest.raises(RuntimeError, match="channels"):
        ops.bilinear_ac_sum([a, torch.zeros(1, 3, 2, 2, device=cuda)], (4, 4))
    with pytest.raises(RuntimeError, match="size must be positive"):
        ops.bilinear_ac_sum([a, b], (0, 4))
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.bilinear_ac_sum([torch.zeros(1, 1, 1, 1 << 22, device=cuda)], (1, 1))      # a source axis of 2^22: the coordinate quotient's limit


# ---- the commuted head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ("fp32", "f16x3"))
def test_commuted_head_matches_the_reference_order(cuda, precision):
    """conv_1 + bn1 + LeakyReLU over 640 full-resolution + 3 x 128 interpolated channels (4 x 16 -> 16 x 64) into 512: three low-resolution convs +
    bilinear_ac_sum + the residual conv, against interpolate -> cat -> conv -> BatchNorm -> LeakyReLU in fp64; the composed form on the same bar."""
    torch.manual_seed(21)
    head = R.randomise_bn(fidnet.SemanticHead(20, 1024), 20, 1.0).eval()
    g = torch.Generator().manual_seed(22)
    x, x_1 = torch.randn(1, 512, 16, 64, generator=g), torch.randn(1, 128, 16, 64, generator=g)
    lows = [torch.randn(1, 128, 4, 16, generator=g) for _ in range(3)]

    def ref(dtype):
        cat = torch.cat([x.to(dtype), x_1.to(dtype)] + [F.interpolate(t.to(dtype), size=(16, 64), mode="bilinear", align_corners=True) for t in lows], 1)
        y = F.conv2d(cat, head.conv_1.weight.detach().to(dtype), head.conv_1.bias.detach().to(dtype))
        bn = head.bn1
        return F.leaky_relu(F.batch_norm(y, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                                         bn.bias.detach().to(dtype), False, 0.0, bn.eps), SLOPE)
    want = ref(torch.float64)
    scale = float(want.abs().max())
    bar, e32 = _bar(want, ref(torch.float32))
    if precision == "f16x3":
        bar = 1e-5 * scale
    head.to(cuda)
    sn.set_conv_precision(precision)
    try:
        with torch.no_grad():
            for commuted in (True, False):
                got = head._conv_1_from_pyramid(x.to(cuda), x_1.to(cuda), [t.to(cuda) for t in lows], (16, 64), commuted).cpu()
                err = float((got.double() - want).abs().max())
                print(f"head conv_1 ({precision}, commuted={commuted}): err {err:.2e}, e_fp32 {e32:.2e}, bar {bar:.2e}, scale {scale:.3g}")
                assert got.shape == want.shape and err <= bar
    finally:
        sn.set_conv_precision("fp32")


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _case(name, cuda):
    """(case, golden, model on the device, fp64 restatement logits and backend map): built once per golden and left unchanged."""
    if name not in _BUILT:
        case = R.CASES[R.CASE_IDS.index(name)]
        g = golden(name)
        m = R.randomise_bn(R.package_model(case).eval(), case[-1], float(g["gain"]))
        want64, mid64 = R.forward(m.state_dict(), torch.from_numpy(g["x"]), dtype=torch.float64, want_backend=True)
        _BUILT[name] = (case, g, m.to(cuda), want64, mid64)
    return _BUILT[name]


def _run(f, x, precision):
    sn.set_conv_precision(precision)
    try:
        with torch.no_grad():
            return f(x).cpu()
    finally:
        sn.set_conv_precision("fp32")


@pytest.mark.parametrize("precision", ("fp32", "f16x3"))
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_model_matches_restatement_and_reference(cuda, name, precision):
    case, g, m, want64, mid64 = _case(name, cuda)
    x = torch.from_numpy(g["x"]).to(cuda)
    ref = torch.from_numpy(g["logits"])
    scale = float(ref.abs().max())
    got = _run(m, x, precision)
    e64, eref = float((got.double() - want64).abs().max()), float((got - ref).abs().max())
    print(f"{name} {precision}: scale {scale:.3g}; fast route vs fp64 restatement {e64 / scale:.2e}, vs stored reference {eref / scale:.2e} (of the scale)")
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert e64 <= 1e-3 * scale and eref <= 1e-3 * scale
    # every combination of the composed and the fused forms: the same bar (whichever a precision does not take by default stays tested)
    for fs, ch in ((False, False), (True, False), (False, True), (True, True)):
        alt = _run(lambda t: m.model._forward(t, fused_stem=fs, commuted_head=ch), x, precision)
        ealt = float((alt.double() - want64).abs().max())
        print(f"    fused_stem={fs} commuted_head={ch}: vs fp64 restatement {ealt / scale:.2e}")
        assert ealt <= 1e-3 * scale
    # the backend's own contract, slice by slice (the logits alone do not hold the deep layers), and the head's own contract on top of it
    mid = _run(m.model.backend, x, precision)
    assert mid.shape == mid64.shape
    sums, _ = R.backend_digest(mid)
    for i, (sname, lo, hi) in enumerate(R.SLICES):
        smax = float(mid64[:, lo:hi].abs().max())
        es = float((mid[:, lo:hi].double() - mid64[:, lo:hi]).abs().max())
        print(f"    backend slice {sname}: max {smax:.3g}, err / max {es / smax:.2e}")
        assert es <= 1e-3 * smax
        assert abs(sums[i, 1] - g["backend_sums"][i, 1]) <= 1e-3 * g["backend_sums"][i, 1]      # and the reference's own digest
    slow = _run(m.model.semantic_head, mid.to(cuda), precision)
    eslow = float((slow - got).abs().max())
    print(f"    SemanticHead(backend(x)) vs the fast route {eslow / scale:.2e}")
    assert eslow <= 1e-3 * scale


# precision, fused_stem, commuted_head (None: the precision's default).  The defaults of both precisions (f16x3 runs slu_point_mlp), and both
# fused routes forced under both: the stem pack (`_stem_cache`) and the sliced conv_1 packs (`conv_1.low*`, `conv_1.full_res`) are only built there
ROUTES = (("fp32", None, None), ("f16x3", None, None), ("fp32", True, True), ("f16x3", True, True))


def test_second_forward_is_bit_identical_and_the_cache_follows_the_weights(cuda):
    case, g, m, _, _ = _case(R.CASE_IDS[1], cuda)
    x = torch.from_numpy(g["x"]).to(cuda)

    def run(route):
        return _run(lambda t: m.model._forward(t, fused_stem=route[1], commuted_head=route[2]), x, route[0])
    first = [run(r) for r in ROUTES]                                                   # every cache of every route is filled from here on
    assert torch.equal(_run(m, x, "fp32"), first[0]) and torch.equal(_run(m, x, "f16x3"), first[1])      # forward(x) is the default route
    for r, f in zip(ROUTES, first):
        assert torch.equal(run(r), f), r                                               # a second forward repeats the first bit for bit
    assert not torch.equal(first[0], first[2])                                         # the forced forms are other arithmetic, not the default again
    # in place: same storage, new version.  Per cache at least one parameter: the stem (the fused pack and the four composed convs), a block
    # conv and BatchNorm, conv_1 (whole and sliced) with its BatchNorm, the last conv's bias
    backend, head = m.model.backend, m.model.semantic_head
    for p in (backend.conv1.bias, backend.conv3.weight, backend.bn_1.running_var, backend.layer4[2].bn2.bias, backend.layer2[0].conv1.weight,
              head.conv_1.weight, head.conv_1.bias, head.bn1.running_mean, head.semantic_output.bias):
        keep = p.detach().clone()
        with torch.no_grad():
            p.mul_(-1.0) if p is not backend.bn_1.running_var else p.mul_(4.0)
        try:
            changed = [run(r) for r in ROUTES]
            want = R.forward({k: v.cpu() for k, v in m.state_dict().items()}, x.cpu(), dtype=torch.float64)
        finally:
            with torch.no_grad():
                p.copy_(keep)
        bar = 1e-3 * float(want.abs().max())
        for r, c, f in zip(ROUTES, changed, first):
            assert not torch.equal(c, f), r                                            # a stale pack would repeat the first result ..
            assert float((c.double() - want).abs().max()) <= bar, r                    # .. and the new one is the edited model's
    for r, f in zip(ROUTES, first):
        assert torch.equal(run(r), f), r                                               # the restoring copy_ is picked up as well


def test_gpu_side_refusals(cuda):
    case, g, m, _, _ = _case(R.CASE_IDS[1], cuda)
    x = torch.from_numpy(g["x"]).to(cuda)
    for f in (m, m.model.backend):
        sn.set_conv_precision("f16")
        try:
            with torch.no_grad(), pytest.raises(RuntimeError, match="'f16'"):
                f(x)
        finally:
            sn.set_conv_precision("fp32")
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f(x.cpu())
            with pytest.raises(RuntimeError, match="divisible by 8"):
                f(x[:, :, :4].contiguous())
            with pytest.raises(RuntimeError, match="divisible by 8"):
                f(x[:, :, :, :36].contiguous())
        with pytest.raises(NotImplementedError, match="inference only"):
            f(x)
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="inference only"):
            m(x)
    finally:
        m.eval()
    big = fidnet.FIDNet(40, "ResNet34_point").eval().to(cuda)                          # more than 32 classes: the head is a plain conv
    with torch.no_grad():
        assert big(x).shape == (1, 40, 8, 40)
