"""GPU: the two CENet decoder kernels against fp64 on the CPU, the commuted aux head, and the ResNet-34 model against the fp64 restatement and
the outputs the reference's own classes produced (tests/golden/cenet_resnet34_*.npz, tools/gen_golden_cenet.py).

Bars.  bilinear_ac_cat: 1e-6 max|x| -- two nested fp32 lerps with correctly rounded fp32 weights are a few ulp of max|x|, and the coordinate is an
exact integer ratio.  bilinear_ac_softmax: 1e-6 on probabilities; the kernel interpolates in fp64 up to the subtraction of the column maximum, so
the bar holds for logits of +-80 too.  Commuted aux head: 1e-5 on probabilities.  It is NOT bit-equal to the reference order: the reference
interpolates the 128 channels and then takes the 128-term dot product per class, the model takes the dot product on the low-resolution map
(fp32 MFMA sums) and interpolates the C logits; both are the same real number (the four weights sum to 1, so the bias passes through), rounded
along different routes -- a logit of magnitude ~1 differs by ~1e-6, a probability by a quarter of that at most.
Model parity: 1e-3 absolute on probabilities (the project's north-star bar) against the restatement in fp64 and against the stored fp32 reference.

Measured on MI355X (max over the three goldens and every returned map), against fp64 / against the stored reference:
    fp32   8.2e-06 / 9.8e-06
    f16x3  2.3e-05 / 2.3e-05"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cenet_restatement as R
from conftest import golden
from semanticlidarunc_amd import ops, salsanext as sn

pytestmark = pytest.mark.gpu

PAIRS = (((1, 5), (8, 40)), ((2, 8), (16, 64)), ((3, 5), (7, 13)), ((4, 16), (4, 16)))      # (in, out): the last is the identity
PAIR_IDS = ["1x5-8x40", "2x8-16x64", "3x5-7x13", "4x16-4x16"]
# name, N, channels per source, explicit channel offsets in a C_tot-channel buffer (None: packed from 0, buffer made by the wrapper)
ARRANGEMENTS = (("one_c3", 1, (3,), None, None), ("two_c1_c128_offsets_n3", 3, (1, 128), (5, 140), 270), ("three_c128_c3_c1", 1, (128, 3, 1), None, None),
                ("three_reversed_offsets_n3", 3, (3, 1, 3), (8, 4, 0), 12))
SENTINEL = -12345.0


def _ref_interp(x, size):
    return F.interpolate(x.double(), size=size, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("arr", ARRANGEMENTS, ids=[a[0] for a in ARRANGEMENTS])
@pytest.mark.parametrize("pi", range(len(PAIRS)), ids=PAIR_IDS)
def test_bilinear_ac_cat_matches_fp64(cuda, pi, arr):
    """Source k takes the input size of pair (pi + k): every launch mixes input sizes, as the model's does."""
    _, n, chans, offs, ctot = arr
    size = PAIRS[pi][1]
    g = torch.Generator().manual_seed(100 * pi + len(chans))
    srcs = [torch.randn(n, c, *PAIRS[(pi + k) % len(PAIRS)][0], generator=g) * (1.0 + k) for k, c in enumerate(chans)]
    if offs is None:
        out = ops.bilinear_ac_cat([s.to(cuda) for s in srcs], size).cpu()
        offs = np.cumsum([0] + list(chans))[:-1].tolist()
        assert out.shape == (n, sum(chans)) + size
        written = torch.ones(out.shape[1], dtype=torch.bool)
    else:
        buf = torch.full((n, ctot) + size, SENTINEL, device=cuda)
        assert ops.bilinear_ac_cat([s.to(cuda) for s in srcs], size, out=buf, c_offs=offs) is buf
        out = buf.cpu()
        written = torch.zeros(ctot, dtype=torch.bool)
    for s, o in zip(srcs, offs):
        want = _ref_interp(s, size)
        got = out[:, o:o + s.shape[1]].double()
        err, bar = float((got - want).abs().max()), 1e-6 * float(s.abs().max())
        print(f"{arr[0]} {PAIR_IDS[pi]} source {tuple(s.shape)} -> channels [{o}, {o + s.shape[1]}): err {err:.2e}, bar {bar:.2e}")
        assert err <= bar
        if tuple(s.shape[2:]) == size:
            assert torch.equal(out[:, o:o + s.shape[1]], s)           # identity sizes give the input back bit for bit
        written[o:o + s.shape[1]] = True
    assert bool((out[:, ~written] == SENTINEL).all())                 # channels outside the slices are untouched


def test_bilinear_ac_cat_refusals(cuda):
    a, b = torch.zeros(1, 2, 2, 2, device=cuda), torch.zeros(1, 2, 4, 4, device=cuda)
    with pytest.raises(RuntimeError, match="1..3 sources"):
        ops.bilinear_ac_cat([a, a, a, a], (4, 4))
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.bilinear_ac_cat([a, b], (4, 4), out=torch.zeros(1, 4, 4, 4, device=cuda), c_offs=(0, 1))
    with pytest.raises(RuntimeError, match="leave"):
        ops.bilinear_ac_cat([a, b], (4, 4), out=torch.zeros(1, 3, 4, 4, device=cuda))
    with pytest.raises(RuntimeError, match="batch"):
        ops.bilinear_ac_cat([a, torch.zeros(2, 2, 2, 2, device=cuda)], (4, 4))
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.bilinear_ac_cat([b], (4, 4), out=b)


def _ref_softmax(x, size):
    return F.softmax(_ref_interp(x, size), 1)


@pytest.mark.parametrize("c", (1, 3, 20, 32))
@pytest.mark.parametrize("pi", range(len(PAIRS)), ids=PAIR_IDS)
def test_bilinear_ac_softmax_matches_fp64(cuda, pi, c):
    (h, w), size = PAIRS[pi]
    g = torch.Generator().manual_seed(7 * pi + c)
    x = 3.0 * torch.randn(3, c, h, w, generator=g)
    big = 80.0 * (2.0 * torch.randint(0, 2, (3, c, h, w), generator=g) - 1.0)      # +-80, a sign per element
    flat = torch.full((3, c, h, w), 1.25) * torch.randn(3, 1, h, w, generator=g)   # all classes equal at every pixel
    for name, t in (("randn x 3", x), ("+-80", big), ("equal", flat)):
        got = ops.bilinear_ac_softmax(t.to(cuda), size).cpu()
        assert got.shape == (3, c) + size and bool(torch.isfinite(got).all())
        err = float((got.double() - _ref_softmax(t, size)).abs().max())
        print(f"C = {c} {PAIR_IDS[pi]} {name}: err {err:.2e}")
        assert err <= 1e-6
        if name == "equal":
            assert bool((got == torch.tensor(1.0 / c, dtype=torch.float32)).all())          # exactly 1 / C
    if (h, w) == size:
        assert torch.equal(ops.bilinear_ac_softmax(x.to(cuda)).cpu(), ops.bilinear_ac_softmax(x.to(cuda), size).cpu())


def test_bilinear_ac_softmax_refuses_33_classes(cuda):
    with pytest.raises(RuntimeError, match="at most 32 classes"):
        ops.bilinear_ac_softmax(torch.zeros(1, 33, 2, 2, device=cuda), (4, 4))


@pytest.mark.parametrize("precision", ("fp32", "f16x3"))
def test_commuted_aux_head_matches_the_reference_order(cuda, precision):
    """1x1 conv at low resolution + bilinear_ac_softmax against interpolate -> conv -> softmax in fp64 (see the module header)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 128, 4, 16, generator=g)
    wgt, bias = torch.randn(20, 128, 1, 1, generator=g) / 128 ** 0.5, 0.1 * torch.randn(20, generator=g)
    want = F.softmax(F.conv2d(_ref_interp(x, (16, 64)), wgt.double(), bias.double()), 1)
    wd = wgt.to(cuda)
    wpack = ops.pack_conv_weight_f16x3(wd) if precision == "f16x3" else ops.pack_conv_weight(wd)
    logits = ops.conv2d_fused([ops.ConvSource(x.to(cuda))], wpack, 20, 1, 1, 0, bias=bias.to(cuda), precision=precision)
    got = ops.bilinear_ac_softmax(logits, (16, 64)).cpu()
    err = float((got.double() - want).abs().max())
    print(f"commuted aux head ({precision}): err {err:.2e}")
    assert err <= 1e-5


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _case(name, cuda):
    """(case, golden, model on the device, fp64 restatement outputs): built once per golden and left unchanged."""
    if name not in _BUILT:
        case = R.CASES[R.CASE_IDS.index(name)]
        g = golden(name)
        m = R.randomise_bn(R.package_model(case).eval(), case[-1], float(g["gain"]))
        want64 = R.as_list(R.forward(m.state_dict(), torch.from_numpy(g["x"]), case[4], R.prefix_of(case), dtype=torch.float64))
        _BUILT[name] = (case, g, m.to(cuda), want64)
    return _BUILT[name]


def _run(m, x, precision):
    sn.set_conv_precision(precision)
    try:
        with torch.no_grad():
            return [t.cpu() for t in R.as_list(m(x))]
    finally:
        sn.set_conv_precision("fp32")


@pytest.mark.parametrize("precision", ("fp32", "f16x3"))
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_model_matches_restatement_and_reference(cuda, name, precision):
    case, g, m, want64 = _case(name, cuda)
    got = _run(m, torch.from_numpy(g["x"]).to(cuda), precision)
    ref = R.load_outputs(g)
    assert len(got) == len(want64) == len(ref) == (4 if case[4] else 1)
    for i, (a, w64, r) in enumerate(zip(got, want64, ref)):
        e64, eref = float((a.double() - w64).abs().max()), float((a - r).abs().max())
        print(f"{name} {precision} map {i}: vs fp64 restatement {e64:.2e}, vs stored reference {eref:.2e}")
        assert a.shape == r.shape and a.dtype == torch.float32
        assert e64 <= 1e-3 and eref <= 1e-3
        assert float((a.sum(1) - 1).abs().max()) <= 1e-5


def test_aux_off_is_element_zero_of_aux_on_and_the_cache_follows_the_weights(cuda):
    case, g, m, _ = _case(R.CASE_IDS[1], cuda)
    x = torch.from_numpy(g["x"]).to(cuda)
    with_aux = _run(m, x, "fp32")
    m.aux = m.model.aux = False
    try:
        alone = _run(m, x, "fp32")
    finally:
        m.aux = m.model.aux = True
    assert len(alone) == 1 and torch.equal(alone[0], with_aux[0])
    assert all(torch.equal(a, b) for a, b in zip(_run(m, x, "fp32"), with_aux))      # a second forward repeats the first bit for bit
    w = m.model.conv_2.conv.weight
    keep = w.detach().clone()
    with torch.no_grad():
        w.mul_(-1.0)                                                                   # in place: same storage, new version
    try:
        changed = _run(m, x, "fp32")
    finally:
        with torch.no_grad():
            w.copy_(keep)
    assert float((changed[0] - with_aux[0]).abs().max()) > 1e-3
    assert all(torch.equal(a, b) for a, b in zip(changed[1:], with_aux[1:]))          # the aux heads do not read conv_2
    assert all(torch.equal(a, b) for a, b in zip(_run(m, x, "fp32"), with_aux))


def test_gpu_side_refusals(cuda):
    case, g, m, _ = _case(R.CASE_IDS[1], cuda)
    x = torch.from_numpy(g["x"]).to(cuda)
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="'f16'"):
            m(x)
    finally:
        sn.set_conv_precision("fp32")
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x.cpu())
        with pytest.raises(RuntimeError, match="divisible by 8"):
            m(x[:, :, :4].contiguous())
        with pytest.raises(RuntimeError, match="divisible by 8"):
            m(x[:, :, :, :36].contiguous())
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="inference only"):
            m(x)
    finally:
        m.eval()
