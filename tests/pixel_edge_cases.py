"""Edge-shape cases for the fp32 per-pixel kernels that share csrc/pixel_common.h (fpn_ops.hip, fpn_train.hip, effnet_ops.hip,
pointwise.hip): the case tables, the seeded input builders and the references, written with plain torch on the CPU and evaluated in
fp64 (the yardstick) and in fp32 (the conditioning check).  No GPU here; ``tests/test_pixel_edge_cases_cpu.py`` shows that every
input is fair for its bar and ``tests/test_gpu_pixel_kernel_edges.py`` holds the kernels to the fp64 results.

A *family* is one kernel (or a forward / backward pair) with
  cases   the shapes and input kinds, each a ``Case`` with an id that names the kernel and the shape,
  build   case -> dict of fp32 CPU inputs from a ``torch.Generator`` seeded by the case id,
  ref     (case, inputs, dtype) -> dict of results in that dtype; every backward is ``torch.autograd.grad`` of the forward,
  bars    case -> {result: (coefficient, mode)}.
Modes: ``exact`` torch.equal; ``abs`` the coefficient itself; ``rel`` coefficient * max(1, max|want|); ``elem`` the difference of each
element divided by max(1, |want|) of that element against the coefficient; ``gap4`` four times the distance of the fp32 torch result
from the fp64 one (the two GroupNorm offset inputs only, the ``_bar`` convention of test_gpu_fpn_train.py).  ``ulp16`` / ``h16_worst`` /
``same_bits`` are the half-ulp bar and the bit-pattern equality of the fp16-storing kernels' table (tests/h8_pixel_edge_cases.py).  The coefficients are
those of the tests the project already has for the same ops (test_gpu_fpn.py, test_gpu_conv.py, test_gpu_fpn_train.py,
test_gpu_fpn_opt.py, test_gpu_effnet.py).  A result key ``name#elem`` is a second look at result ``name``.

Conditioning rule: for every result that is not exact the fp32 torch evaluation must lie within a quarter of the bar of the fp64 one.
An input that fails it gets another seed or scale, never another bar.

Bilinear: the 1e-6 bar holds for power-of-two scales only -- torch's own fp32 path is 1.2e-5 to 2.4e-5 from fp64 at scales 3, 5, 6.
Max-pool: a window of -inf only is left out (ATen sends its gradient to the window's first element, window_argmax to none).
"""
from __future__ import annotations

import zlib
from typing import Callable, Dict, List, NamedTuple, Optional

import torch
import torch.nn.functional as F

EPS = 1e-5
SENTINEL = -7.0
WINDOW_HW = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (2, 7), (7, 9), (13, 37)]
COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 4097]          # values per 1024-thread workgroup
FIXED = [0.0, -0.0] + [s * v for v in (1e-30, 1e-8, 0.5, 20.0, 87.0, 88.5, 89.0, 100.0, 104.0, 1e4) for s in (1.0, -1.0)]
# the cap slu_grid_1d puts on the forward launch of each family with a `round2` case
GRID_CAP = dict(maxpool=16384, avgpool=16384, nearest=16384, s2d=16384, d2s=16384, bilinear=65535, pointwise=65536, replace_tail=65536, groupnorm=65535,
                gate=65535)


class Case(NamedTuple):
    family: str
    id: str
    p: dict
    big: bool = False          # second round of a grid-stride loop: forward only unless the table names the backward


class Family(NamedTuple):
    cases: List[Case]
    build: Callable
    ref: Callable
    bars: Callable


# inputs whose first seed failed the conditioning rule (fp32 torch further than a quarter of the bar from fp64) and the seed offset that
# replaced it.  The wgrad case: torch's fp32 sum of 98304 products is 0.13 to 0.33 of the bar away, depending on the seed.  The GroupNorm
# case: groups of two values, whose dx is 0 up to rounding times rstd, and one pair of the first seed lay close together.
SALTS = {"dwconv3x3_wgrad 3x5x64x512": 5, "groupnorm bwd relu 3x6x1x1 g3": 3}


def gen(case: Case) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + SALTS.get(case.id, 0))


def _leaf(t, dt):
    return None if t is None else t.detach().to(dt).requires_grad_(True)


def _to(t, dt):
    return None if t is None else t.to(dt)


def _grad(out, ins, cot):
    return [None if g is None else g.detach() for g in torch.autograd.grad(out, ins, cot.to(out.dtype), allow_unused=True)]


def _hw(hw):
    return f"{hw[0]}x{hw[1]}"


def _shape(s):
    return "x".join(str(v) for v in s)


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def bar_of(spec, want64, want32):
    """(bar, denominator | None) of one result."""
    coef, mode = spec[:2]
    if mode == "abs":
        return coef, None
    if mode == "rel":
        return coef * max(1.0, float(want64.abs().max())), None
    if mode == "elem":
        return coef, want64.abs().clamp_min(1.0)
    if mode == "gap4":
        return 4.0 * float((want32.double() - want64).abs().max()), None
    raise ValueError(mode)


def cmp(tag, got, want64, want32, bar):
    """_cmp of tests/test_gpu_loss_class_counts.py: prints device-fp64, fp32 torch-fp64 and the bar, then asserts the conditioning rule and the bar"""
    want64 = want64.detach().double().cpu()
    gap = None if want32 is None else float((want32.detach().double().cpu() - want64).abs().max())
    diff = float((got.detach().double().cpu() - want64).abs().max())
    print(f"{tag}: device-fp64 {diff:.3e}, fp32 torch-fp64 {'n/a' if gap is None else format(gap, '.3e')}, bar {bar:.3e}")
    if gap is not None:
        assert gap <= bar / 4, f"{tag}: the inputs are ill-conditioned for this bar (fp32 torch is {gap:.3e} from fp64, bar {bar:.3e})"
    assert diff <= bar, f"{tag}: {diff:.3e} > {bar:.3e}"


# the bar mode of the fp16-storing kernels (tests/h8_pixel_edge_cases.py): |got - want64| <= ulp16(want64) / 2 + tol, an overflowing reference
# value must come back as the infinity; and equality by bit pattern, which tells -0 from +0
def ulp16(v):
    a = v.double().abs()
    a = torch.where(torch.isfinite(a) & (a > 0), a, torch.full_like(a, 2.0 ** -14))
    e = torch.frexp(a)[1].double() - 1.0
    return torch.exp2(e.clamp_min(-14.0) - 10.0)


def h16_worst(got, want64, tol):
    """(ok, worst error / allowed over the finite part, elements that should be an infinity and are not)"""
    got, want64 = got.double(), want64.double()
    over = want64.abs() >= 65520.0
    allowed = ulp16(want64) / 2 + tol
    err = torch.where(over, torch.zeros_like(want64), (got - want64).abs())
    ratio = torch.where(over, torch.zeros_like(want64), err / allowed)
    fine = bool((ratio <= 1.0).all())          # a NaN fails
    bad_inf = int((over & (got != torch.sign(want64) * float("inf"))).sum())
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
    return fine and bad_inf == 0, worst, bad_inf


def same_bits(a, b):
    """equality of two fp32 tensors of fp16 or fp32 values including the sign of zero"""
    a, b = a.float().contiguous(), b.float().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check(case: Case, got: Dict[str, torch.Tensor], want64, want32):
    """Every result of `got` against the references.  A key ``name@variant`` of `got` is held to reference ``name``."""
    seen = set()
    for bkey, spec in FAMILIES[case.family].bars(case).items():
        base = bkey.split("#")[0]
        for gkey, g in got.items():
            if gkey.split("@")[0] != base:
                continue
            seen.add(gkey)
            tag = f"{case.id} {gkey}{bkey[len(base):]}"
            w64, w32 = want64[base], want32[base]
            g = g.detach().cpu()
            assert tuple(g.shape) == tuple(w64.shape), f"{tag}: shape {tuple(g.shape)}, expected {tuple(w64.shape)}"
            assert bool(torch.isfinite(g).all()), f"{tag}: not finite"
            if spec[1] == "exact":
                same = torch.equal(g.double(), w64)
                print(f"{tag}: exact {'ok' if same else 'DIFFERS'}")
                assert same, f"{tag}: differs from the reference in {int((g.double() != w64).sum())} of {g.numel()} elements"
                continue
            bar, den = bar_of(spec, w64, w32)
            if spec[2:] == ("unconditioned",):
                w32 = None
            if den is not None:
                cmp(tag, g.double() / den, w64 / den, None if w32 is None else w32.double() / den, bar)
            else:
                cmp(tag, g, w64, w32, bar)
    assert seen == set(got), f"{case.id}: results without a bar: {sorted(set(got) - seen)}"


def conditioning(case: Case, want64, want32):
    """[(result, fp32 torch - fp64, bar)] of the results that are not exact; the exact ones must agree between the two dtypes."""
    out = []
    for bkey, spec in FAMILIES[case.family].bars(case).items():
        base = bkey.split("#")[0]
        w64, w32 = want64[base], want32[base]
        assert w64.dtype == torch.float64 and w32.dtype == torch.float32, f"{case.id} {bkey}: reference dtypes"
        assert bool(torch.isfinite(w64).all()) and bool(torch.isfinite(w32).all()), f"{case.id} {bkey}: reference not finite"
        if spec[1] == "exact":
            assert torch.equal(w32.double(), w64), f"{case.id} {bkey}: exact result differs between fp32 and fp64 torch"
            continue
        bar, den = bar_of(spec, w64, w32)
        gap = (w32.double() - w64).abs()
        out.append((bkey, float((gap if den is None else gap / den).max()), bar, spec))
    return out


def evaluate(case: Case, families=None):
    """(inputs, fp64 results, fp32 results); families: another table than this module's"""
    fam = (FAMILIES if families is None else families)[case.family]
    inputs = fam.build(case)
    with torch.enable_grad():
        return inputs, fam.ref(case, inputs, torch.float64), fam.ref(case, inputs, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# max-pool 3x3 / s2 / p1 forward and backward: exact (the cotangent is integer-valued, so the <= 4-term sums are exact in any order)
# ---------------------------------------------------------------------------------------------------------------------
def _maxpool_cases():
    cs = [Case("maxpool", f"maxpool {kind} 2x3x{_hw(hw)}", dict(shape=(2, 3) + hw, kind=kind)) for hw in WINDOW_HW for kind in ("neg", "ties", "const")]
    # x [2, 9, 513, 1025] pools to 2 373 138 outputs, one round of the 16384 x 256 grid; 17 channels give 4 482 594, a second round
    return cs + [Case("maxpool", f"maxpool {tag} 2x{ch}x513x1025", dict(shape=(2, ch, 513, 1025), kind="randn"), True) for tag, ch in (("large", 9), ("round2", 17))]


def _maxpool_build(c):
    g, shape = gen(c), c.p["shape"]
    if c.p["kind"] == "neg":          # padding must never win
        x = -(torch.rand(shape, generator=g) + 0.125)
    elif c.p["kind"] == "ties":       # post-ReLU, values 0, 1, 2: most windows hold their maximum more than once
        x = torch.relu(torch.randint(-2, 3, shape, generator=g).float())
    elif c.p["kind"] == "const":
        x = torch.full(shape, 1.5)
    else:
        x = torch.randn(shape, generator=g)
    n, ch, h, w = shape
    return dict(x=x, dy=torch.randint(-3, 4, (n, ch, (h + 1) // 2, (w + 1) // 2), generator=g).float())


def _maxpool_ref(c, i, dt):
    x = _leaf(i["x"], dt)
    y = F.max_pool2d(x, 3, 2, 1)
    out = dict(y=y.detach())
    if not c.big:
        out["dx"] = _grad(y, [x], i["dy"])[0]
    return out


def _maxpool_bars(c):
    return dict(y=(None, "exact")) if c.big else dict(y=(None, "exact"), dx=(None, "exact"))


# ---------------------------------------------------------------------------------------------------------------------
# average pool 3x3 / s2 / p1 (divisor 9) of x[n % B] * scale[n]: 1e-6
# ---------------------------------------------------------------------------------------------------------------------
AVG_MODES = {"plain": (2, 2, False), "scaled": (2, 2, True), "bcast1to3": (1, 3, True), "bcast2to4": (2, 4, True)}      # in_batch, n_out, scale


def _avgpool_cases():
    cs = [Case("avgpool", f"avgpool {mode} 3x{_hw(hw)}", dict(hw=hw, c=3, mode=mode)) for hw in WINDOW_HW for mode in AVG_MODES]
    return cs + [Case("avgpool", f"avgpool {tag} 2x{ch}x513x1025", dict(hw=(513, 1025), c=ch, mode="scaled"), True) for tag, ch in (("large", 9), ("round2", 17))]


def _avgpool_build(c):
    g = gen(c)
    b, n_out, scaled = AVG_MODES[c.p["mode"]]
    x = torch.randn((b, c.p["c"]) + c.p["hw"], generator=g) * 0.25
    return dict(x=x, scale=0.5 + 0.5 * torch.rand(n_out, c.p["c"], generator=g) if scaled else None, n_out=n_out)


def _avgpool_ref(c, i, dt):
    x = i["x"].to(dt)[torch.arange(i["n_out"]) % i["x"].shape[0]]
    if i["scale"] is not None:
        x = x * i["scale"].to(dt)[:, :, None, None]
    return dict(y=F.avg_pool2d(x, 3, 2, 1, count_include_pad=True))


# ---------------------------------------------------------------------------------------------------------------------
# nearest down-sampling y[oy][ox] = x[oy f][ox f] and its backward: exact
# ---------------------------------------------------------------------------------------------------------------------
def _nearest_cases():
    cs = [Case("nearest", f"nearest f{f} 2x3x{f}x{3 * f}", dict(shape=(2, 3, f, 3 * f), f=f)) for f in (1, 2, 4, 8)]
    return cs + [Case("nearest", "nearest round2 f2 1x17x1024x1024", dict(shape=(1, 17, 1024, 1024), f=2), True)]


def _nearest_build(c):
    g, (n, ch, h, w), f = gen(c), c.p["shape"], c.p["f"]
    return dict(x=torch.randn(c.p["shape"], generator=g), dy=torch.randn(n, ch, h // f, w // f, generator=g))


def _nearest_ref(c, i, dt):
    x, f = _leaf(i["x"], dt), c.p["f"]
    y = F.interpolate(x, scale_factor=1.0 / f, mode="nearest") if f > 1 else x * 1
    assert torch.equal(y, x[:, :, ::f, ::f])
    out = dict(y=y.detach())
    if not c.big:
        out["dx"] = _grad(y, [x], i["dy"])[0]
    return out


def _nearest_bars(c):
    return dict(y=(None, "exact")) if c.big else dict(y=(None, "exact"), dx=(None, "exact"))


# ---------------------------------------------------------------------------------------------------------------------
# space-to-depth, phase-major: y[n, (2p+q) C + c, oy, ox] = x[n, c, 2oy+p, 2ox+q], alone and of cat(a[:, :ca], b): exact
# ---------------------------------------------------------------------------------------------------------------------
def _s2d_cases():
    cs = [Case("s2d", f"space_to_depth2 {_shape(s)}", dict(a=s, ca=s[1], cb=0)) for s in ((2, 3, 4, 6), (1, 1, 2, 2), (3, 5, 2, 10))]
    cs += [Case("s2d", f"space_to_depth2_cat Ca{ca_full} ca{ca} Cb{cb} 2x.x4x6", dict(a=(2, ca_full, 4, 6), ca=ca, cb=cb))
           for ca_full, ca, cb in ((3, 3, 2), (3, 1, 2), (2, 2, 1))]
    return cs + [Case("s2d", "space_to_depth2_cat round2 Ca3 ca2 Cb3 1x.x1024x1024", dict(a=(1, 3, 1024, 1024), ca=2, cb=3), True)]


def _s2d_build(c):
    g, a = gen(c), c.p["a"]
    return dict(a=torch.randn(a, generator=g), b=torch.randn((a[0], c.p["cb"]) + a[2:], generator=g) if c.p["cb"] else None)


def _s2d_ref(c, i, dt):
    x = i["a"].to(dt)[:, :c.p["ca"]]
    if i["b"] is not None:
        x = torch.cat([x, i["b"].to(dt)], 1)
    n, ch, h, w = x.shape
    y = F.pixel_unshuffle(x, 2)          # channel c * 4 + (2p + q)
    return dict(y=y.view(n, ch, 4, h // 2, w // 2).transpose(1, 2).reshape(n, 4 * ch, h // 2, w // 2).contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# depth-to-space (PixelShuffle) into a channel slice of a larger buffer [+ ELU + 1], and its backward
# ---------------------------------------------------------------------------------------------------------------------
def _d2s_cases():
    cs = [Case("d2s", f"depth_to_space r{r} {_hw(hw)}{' elu+1' if elu else ''} into 1:3 of 5", dict(n=2, cout=2, hw=hw, r=r, elu=elu, ctot=5, c_off=1))
          for r in (1, 2, 4, 8) for hw in ((1, 1), (3, 5)) for elu in (False, True)]
    cs.append(Case("d2s", "depth_to_space r2 3x5 own output", dict(n=2, cout=3, hw=(3, 5), r=2, elu=False, ctot=3, c_off=0, fresh=True)))
    return cs + [Case("d2s", "depth_to_space round2 r2 1x20x512x512 into 1:6 of 7", dict(n=1, cout=5, hw=(512, 512), r=2, elu=False, ctot=7, c_off=1), True)]


def _d2s_build(c):
    g, p = gen(c), c.p
    h, w = p["hw"]
    return dict(x=torch.randn(p["n"], p["cout"] * p["r"] ** 2, h, w, generator=g), dy=torch.randn(p["n"], p["ctot"], h * p["r"], w * p["r"], generator=g))


def _d2s_ref(c, i, dt):
    p, x = c.p, _leaf(i["x"], dt)
    ps = F.pixel_shuffle(x, p["r"])
    y = F.elu(ps) + 1 if p["elu"] else ps
    out = torch.full(i["dy"].shape, SENTINEL, dtype=dt)          # channels outside the slice keep the sentinel
    out[:, p["c_off"]:p["c_off"] + p["cout"]] = y.detach()
    res = dict(out=out)
    if not p["elu"] and not c.big:
        res["dx"] = _grad(ps, [x], i["dy"][:, p["c_off"]:p["c_off"] + p["cout"]])[0]
    return res


def _d2s_bars(c):
    if c.p["elu"]:
        return dict(out=(1e-6, "abs"))
    return dict(out=(None, "exact")) if c.big else dict(out=(None, "exact"), dx=(None, "exact"))


# ---------------------------------------------------------------------------------------------------------------------
# value * softmax(score over W) and its backward: forward 2e-6 of the scale, gradients 2e-5 of theirs
# ---------------------------------------------------------------------------------------------------------------------
ROW_W = [1, 2, 63, 64, 65, 255, 256, 257, 511, 4095, 4096]
ROW_KINDS = ("randn3", "wide", "const", "shift1000")


def _row_cases():
    # (3, 2, 2, 65): N, C and H all above 1 and N != H, where every wrong split of blockIdx.x into (n, y) reads another row
    shapes = [(2, 3, 2, w) for w in ROW_W] + [(3, 1, 1, 65), (1, 2, 5, 300), (3, 2, 2, 65)]
    return [Case("rowsoftmax", f"row_softmax_mul {kind} {_shape(s)}", dict(shape=s, kind=kind)) for s in shapes for kind in ROW_KINDS]


def _row_build(c):
    g, (n, ch, h, w), kind = gen(c), c.p["shape"], c.p["kind"]
    if kind == "const":
        score = torch.full((n, 1, h, w), 0.75)
    else:
        score = torch.randn(n, 1, h, w, generator=g) * (60.0 if kind == "wide" else 3.0) + (1000.0 if kind == "shift1000" else 0.0)
    return dict(score=score, value=torch.randn(n, ch, h, w, generator=g), dout=torch.randn(n, ch, h, w, generator=g))


def _row_ref(c, i, dt):
    s, v = _leaf(i["score"], dt), _leaf(i["value"], dt)
    out = v * torch.softmax(s, dim=-1)
    ds, dv = _grad(out, [s, v], i["dout"])
    return dict(out=out.detach(), dscore=ds, dvalue=dv)


# ---------------------------------------------------------------------------------------------------------------------
# bilinear up-sampling (align_corners = False), power-of-two scales: forward 1e-6, backward 1e-5 of its scale; scale 1 is the identity
# ---------------------------------------------------------------------------------------------------------------------
def _bilinear_cases():
    cs = [Case("bilinear", f"bilinear s{s} {_shape(shape)}", dict(shape=shape, s=s)) for s in (1, 2, 4, 8, 16) for shape in ((1, 2, 7, 37), (2, 1, 3, 5), (1, 1, 33, 129))]
    return cs + [Case("bilinear", "bilinear round2 s4 1x65x64x257", dict(shape=(1, 65, 64, 257), s=4), True)]


def _bilinear_build(c):
    g, (n, ch, h, w), s = gen(c), c.p["shape"], c.p["s"]
    return dict(x=torch.randn(c.p["shape"], generator=g) * 0.25, dy=torch.randn(n, ch, h * s, w * s, generator=g))


def _bilinear_ref(c, i, dt):
    x = _leaf(i["x"], dt)
    y = F.interpolate(x, scale_factor=c.p["s"], mode="bilinear", align_corners=False)
    out = dict(y=y.detach())
    if not c.big:
        out["dx"] = _grad(y, [x], i["dy"])[0]
    return out


def _bilinear_bars(c):
    if c.p["s"] == 1:
        return dict(y=(None, "exact"), dx=(None, "exact"))
    return dict(y=(1e-6, "abs")) if c.big else dict(y=(1e-6, "abs"), dx=(1e-5, "rel"))


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm [+ ReLU] with its statistics, and its backward
# ---------------------------------------------------------------------------------------------------------------------
def _gn_case(tag, shape, groups, kind="randn", affine=True, relu=False, bwd=False, want_affine=True, big=False):
    return Case("groupnorm", f"groupnorm {tag} {_shape(shape)} g{groups}", dict(shape=shape, groups=groups, kind=kind, affine=affine, relu=relu, bwd=bwd,
                                                                               want_affine=want_affine), big)


def _gn_cases():
    cs = []
    for count in COUNTS + [66, 1026, 4098]:          # the last three: ragged counts that C / groups = 2 and 6 divide (the listed ones are odd or powers of two)
        for groups in (6, 3, 1):
            cpg = 6 // groups
            if count % cpg == 0:
                cs.append(_gn_case(f"stats{count}", (2, 6, 1, count // cpg), groups))
    s = (2, 8, 5, 13)
    cs += [_gn_case("noaffine", s, 4, affine=False, bwd=True), _gn_case("noaffine relu", s, 4, affine=False, relu=True, bwd=True),
           _gn_case("const", s, 4, kind="const", bwd=True), _gn_case("const relu zeros", s, 4, kind="const", relu=True, bwd=True),
           _gn_case("offset100", s, 4, kind="offset100"), _gn_case("offset1000", s, 4, kind="offset1000")]
    for hw in (1, 63, 257):
        for groups in (6, 3):
            for relu in (False, True):
                for want_affine in (False, True):
                    cs.append(_gn_case(f"bwd{'' if want_affine else ' dx only'}{' relu' if relu else ''}", (3, 6, 1, hw), groups, relu=relu, bwd=True,
                                       want_affine=want_affine))
    return cs + [_gn_case("round2", (1, 66, 512, 513), 2, big=True)]


def _gn_build(c):
    g, p = gen(c), c.p
    n, ch, h, w = p["shape"]
    cpg = ch // p["groups"]
    x = torch.randn(p["shape"], generator=g)
    if p["kind"] == "offset100":
        x = x * 0.1 + 100.0
    elif p["kind"] == "offset1000":
        x = x * 0.01 + 1000.0
    else:
        x = x * 1.5 + 0.5
    gamma = 1.0 + 0.3 * torch.randn(ch, generator=g) if p["affine"] else None
    beta = 0.3 * torch.randn(ch, generator=g) if p["affine"] else None
    if cpg * h * w == 1:
        # a group of one value: y = beta.  ATen evaluates x a + b with a = rstd gamma = 316 gamma and b = beta - mean a, and rounding b at the
        # size of x a costs its fp32 result 316 |x gamma| 2^-24, 4e-5 at |x| = 2: the scale that keeps fp32 torch inside a quarter of the bar
        x = torch.randn(p["shape"], generator=g) * 0.03
    if p["kind"] == "const":          # group 0 of every sample: 2^-4 everywhere (sums, mean and x a exact, so y = beta in any precision; small as above)
        x[:, :cpg] = 0.0625
        if p["relu"]:
            beta[:cpg] = 0.0          # y is exactly 0 there; the backward masks with y > 0
    dy = torch.randn(p["shape"], generator=g)
    if cpg * h * w == 1:          # dx = 0 there, and fp32 torch leaves rstd |dy gamma| 2^-24 of it: 6e-5 with |dy| near 3
        dy = dy * 0.1
    return dict(x=x, gamma=gamma, beta=beta, dy=dy)


def _gn_ref(c, i, dt):
    p = c.p
    n, ch, h, w = p["shape"]
    x, gamma, beta = _leaf(i["x"], dt), _leaf(i["gamma"], dt), _leaf(i["beta"], dt)
    y = F.group_norm(x, p["groups"], gamma, beta, EPS)
    if p["relu"]:
        y = F.relu(y)
    xg = x.detach().view(n, p["groups"], -1)
    out = dict(y=y.detach(), mean=xg.mean(-1).reshape(-1), rstd=(xg.var(-1, unbiased=False) + EPS).rsqrt().reshape(-1))
    if p["bwd"]:
        gr = _grad(y, [x] + ([gamma, beta] if p["affine"] else []), i["dy"])
        out["dx"] = gr[0]
        if p["affine"]:
            out["dgamma"], out["dbeta"] = gr[1], gr[2]
        else:          # d/dgamma, d/dbeta at gamma = 1, beta = 0
            one, zero = torch.ones(ch, dtype=dt, requires_grad=True), torch.zeros(ch, dtype=dt, requires_grad=True)
            y1 = F.group_norm(x.detach(), p["groups"], one, zero, EPS)
            out["dgamma"], out["dbeta"] = _grad(F.relu(y1) if p["relu"] else y1, [one, zero], i["dy"])
    return out


def _gn_bars(c):
    offset = c.p["kind"].startswith("offset")
    # offset inputs: torch's own fp32 result is far from fp64, so the output's bar is 4x that gap and the fp32 statistics are no yardstick
    bars = dict(y=(None, "gap4") if offset else (2e-5, "abs"), mean=(2e-5, "elem") + (("unconditioned",) if offset else ()),
                rstd=(2e-5, "elem") + (("unconditioned",) if offset else ()))
    if c.p["bwd"]:
        bars.update(dx=(5e-5, "rel"), dgamma=(5e-5, "rel"), dbeta=(5e-5, "rel"))
    return bars


# ---------------------------------------------------------------------------------------------------------------------
# x * softmax(score over H W) + x with its statistics (max, 1 / sum exp), and its backward
# ---------------------------------------------------------------------------------------------------------------------
def _gate_cases():
    cs = [Case("gate", f"spatial_softmax_gate 3x{ch}x1x{hw}", dict(shape=(3, ch, 1, hw))) for hw in COUNTS for ch in (1, 5)]
    return cs + [Case("gate", "spatial_softmax_gate round2 1x65x512x513", dict(shape=(1, 65, 512, 513)), True)]


def _gate_build(c):
    g, (n, ch, h, w) = gen(c), c.p["shape"]
    offs = torch.tensor([-50.0, 0.0, 50.0])[:n] if n == 3 else torch.zeros(n)      # another sample's maximum or sum shows up
    score = 2.0 * torch.randn(n, 1, h, w, generator=g) + offs[:, None, None, None]
    return dict(x=torch.randn(c.p["shape"], generator=g), score=score, dout=torch.randn(c.p["shape"], generator=g))


def _gate_ref(c, i, dt):
    x, s = _leaf(i["x"], dt), _leaf(i["score"], dt)
    n = x.shape[0]
    out = x * torch.softmax(s.view(n, -1), dim=-1).view_as(s) + x
    flat = s.detach().view(n, -1)
    mx = flat.amax(-1)
    res = dict(out=out.detach(), smax=mx, sinv=1.0 / torch.exp(flat - mx[:, None]).sum(-1))
    if not c.big:
        res["dx"], res["dscore"] = _grad(out, [x, s], i["dout"])
    return res


def _gate_bars(c):
    # 1 / sum exp: the forward's coefficient on a value <= 1 (the sum holds the term exp(0) = 1)
    bars = dict(out=(2e-6, "rel"), smax=(None, "exact"), sinv=(2e-6, "elem"))
    if not c.big:
        bars.update(dx=(2e-5, "rel"), dscore=(2e-5, "rel"))
    return bars


# ---------------------------------------------------------------------------------------------------------------------
# activations, forward and backward.  `#elem` holds every element to the same coefficient at its own scale max(1, |want|): with
# 1e4 among the inputs the bar of the whole tensor alone would let an error of 0.02 on a value near 1 pass.
# ---------------------------------------------------------------------------------------------------------------------
POINTWISE = {"relu": ("leaky", 0.0), "leaky0.01": ("leaky", 0.01), "tanh": ("tanh", 0.0), "elu+1": ("elu+1", 0.0), "silu": ("silu", 0.0)}

GRAD_AT_ZERO = {"relu": 0.0, "leaky0.01": 0.01, "elu+1": 1.0}          # what ATen gives at x = 0 and x = -0


def pointwise_fn(name, x):
    op, slope = POINTWISE[name]
    if op == "leaky":
        return F.relu(x) if slope == 0.0 else F.leaky_relu(x, slope)
    return {"tanh": torch.tanh, "silu": F.silu, "elu+1": lambda v: F.elu(v) + 1}[op](x)


def _pw_cases():
    cs = [Case("pointwise", f"pointwise {name} n{n}", dict(name=name, n=n)) for name in POINTWISE for n in (1, 22, 255, 256, 257)]
    return cs + [Case("pointwise", "pointwise round2 elu+1 n16777473", dict(name="elu+1", n=16777216 + 257), True)]


def _pw_build(c):
    g, n = gen(c), c.p["n"]
    x = torch.randn(n, generator=g) * 2.0
    if not c.big:          # the fixed list first (n = 22: the list alone; n = 1: the 0 alone)
        k = min(n, len(FIXED))
        x[:k] = torch.tensor(FIXED[:k])
    return dict(x=x, dy=torch.randn(n, generator=g))


def _pw_ref(c, i, dt):
    x = _leaf(i["x"], dt)
    y = pointwise_fn(c.p["name"], x)
    return dict(y=y.detach(), dx=_grad(y, [x], i["dy"])[0])


def _pw_bars(c):
    fwd = 2e-6 if c.p["name"] == "silu" else 1e-5
    return {"y": (fwd, "rel"), "y#elem": (fwd, "elem"), "dx": (1e-5, "rel"), "dx#elem": (1e-5, "elem")}


def silu_as_kernel(x32):
    """fp32 emulation of pixel_common.h's silu and of pointwise_bwd_kernel's SiLU derivative: (v / (1 + exp(-v)), s (1 + v (1 - s)))"""
    e = torch.exp(-x32)
    sg = 1.0 / (1.0 + e)
    return x32 / (1.0 + e), sg * (1.0 + x32 * (1.0 - sg))


# ---------------------------------------------------------------------------------------------------------------------
# out = cat(x[:, :C-m], meta) and its backward: exact
# ---------------------------------------------------------------------------------------------------------------------
def _tail_cases():
    cs = [Case("replace_tail", f"replace_tail m{m} 2x4x3x5", dict(shape=(2, 4, 3, 5), m=m)) for m in (4, 1, 3)]
    return cs + [Case("replace_tail", "replace_tail round2 m3 1x65x512x513", dict(shape=(1, 65, 512, 513), m=3), True)]


def _tail_build(c):
    g, (n, ch, h, w) = gen(c), c.p["shape"]
    return dict(x=torch.randn(c.p["shape"], generator=g), meta=torch.randn(n, c.p["m"], h, w, generator=g), dout=torch.randn(c.p["shape"], generator=g))


def _tail_ref(c, i, dt):
    x, meta, m = _leaf(i["x"], dt), _leaf(i["meta"], dt), c.p["m"]
    out = torch.cat([x[:, :x.shape[1] - m], meta], 1)
    dx, dmeta = _grad(out, [x, meta], i["dout"])
    return dict(out=out.detach(), dx=dx, dmeta=dmeta)


# ---------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 (pad 1, stride 1 / 2) [+ bias] [+ SiLU]: 2e-6 of the scale; its weight gradient: 2e-5 of its scale
# ---------------------------------------------------------------------------------------------------------------------
def _dw_cases():
    return [Case("dwconv", f"dwconv3x3 s{st}{' bias' if bias else ''}{' silu' if act == 'silu' else ''} 2x3x{_hw(hw)}", dict(shape=(2, 3) + hw, stride=st, bias=bias, act=act))
            for hw in WINDOW_HW for st in (1, 2) for bias in (False, True) for act in ("none", "silu")]


def _dw_build(c):
    g, ch = gen(c), c.p["shape"][1]
    return dict(x=torch.randn(c.p["shape"], generator=g), w=torch.randn(ch, 9, generator=g) / 3.0, bias=0.5 * torch.randn(ch, generator=g) if c.p["bias"] else None)


def _dw_ref(c, i, dt):
    ch = c.p["shape"][1]
    y = F.conv2d(i["x"].to(dt), i["w"].to(dt).view(ch, 1, 3, 3), _to(i["bias"], dt), stride=c.p["stride"], padding=1, groups=ch)
    return dict(y=F.silu(y) if c.p["act"] == "silu" else y)


def _dwg_cases():
    shapes = [(2, 3) + hw for hw in WINDOW_HW] + [(1, 1, 7, 9), (3, 5, 64, 512)]      # the last: 128 fp32 terms per lane before the fp64 sum
    return [Case("dwwgrad", f"dwconv3x3_wgrad {_shape(s)}", dict(shape=s)) for s in shapes]


def _dwg_build(c):
    g = gen(c)
    return dict(x=torch.randn(c.p["shape"], generator=g), dy=torch.randn(c.p["shape"], generator=g))


def _dwg_ref(c, i, dt):
    ch = c.p["shape"][1]
    w = torch.zeros(ch, 1, 3, 3, dtype=dt, requires_grad=True)
    y = F.conv2d(i["x"].to(dt), w, None, stride=1, padding=1, groups=ch)
    return dict(dw=_grad(y, [w], i["dy"])[0].view(ch, 9))


# ---------------------------------------------------------------------------------------------------------------------
# SqueezeExcitation: the global average pool and the gate sigmoid(fc2(SiLU(fc1(mean)))): 2e-6
# ---------------------------------------------------------------------------------------------------------------------
def _gap_cases():
    return [Case("gap", f"global_avgpool {n}x{ch}x1x{hw}", dict(shape=(n, ch, 1, hw))) for hw in (1, 63, 64, 65, 4097) for n, ch in ((1, 1), (1, 5), (7, 1))]


def _gap_build(c):
    return dict(x=torch.randn(c.p["shape"], generator=gen(c)))


def _gap_ref(c, i, dt):
    return dict(avg=i["x"].to(dt).mean((2, 3)))


SE_MAX = (16000, 384)          # (C + S) * 4 bytes = 64 KB of LDS exactly; one more channel is refused


def _se_cases():
    cs = [Case("se", f"se_scale C{ch} S{s}", dict(c=ch, s=s, bias=True)) for ch, s in ((1, 1), (65, 3), (1536, 96), SE_MAX)]
    return cs + [Case("se", "se_scale C65 S3 no bias", dict(c=65, s=3, bias=False))]


def _se_build(c):
    g, ch, s = gen(c), c.p["c"], c.p["s"]
    b = c.p["bias"]
    return dict(x=torch.randn(2, ch, 2, 3, generator=g), w1=torch.randn(s, ch, generator=g) / ch ** 0.5, b1=0.2 * torch.randn(s, generator=g) if b else None,
                w2=torch.randn(ch, s, generator=g) / s ** 0.5, b2=0.2 * torch.randn(ch, generator=g) if b else None)


def _se_ref(c, i, dt):
    hid = F.silu(F.linear(i["x"].to(dt).mean((2, 3)), i["w1"].to(dt), _to(i["b1"], dt)))
    return dict(scale=torch.sigmoid(F.linear(hid, i["w2"].to(dt), _to(i["b2"], dt))))


def _const(bars):
    return lambda c: bars


FAMILIES: Dict[str, Family] = {
    "maxpool": Family(_maxpool_cases(), _maxpool_build, _maxpool_ref, _maxpool_bars),
    "avgpool": Family(_avgpool_cases(), _avgpool_build, _avgpool_ref, _const(dict(y=(1e-6, "abs")))),
    "nearest": Family(_nearest_cases(), _nearest_build, _nearest_ref, _nearest_bars),
    "s2d": Family(_s2d_cases(), _s2d_build, _s2d_ref, _const(dict(y=(None, "exact")))),
    "d2s": Family(_d2s_cases(), _d2s_build, _d2s_ref, _d2s_bars),
    "rowsoftmax": Family(_row_cases(), _row_build, _row_ref, _const(dict(out=(2e-6, "rel"), dscore=(2e-5, "rel"), dvalue=(2e-5, "rel")))),
    "bilinear": Family(_bilinear_cases(), _bilinear_build, _bilinear_ref, _bilinear_bars),
    "groupnorm": Family(_gn_cases(), _gn_build, _gn_ref, _gn_bars),
    "gate": Family(_gate_cases(), _gate_build, _gate_ref, _gate_bars),
    "pointwise": Family(_pw_cases(), _pw_build, _pw_ref, _pw_bars),
    "replace_tail": Family(_tail_cases(), _tail_build, _tail_ref, _const(dict(out=(None, "exact"), dx=(None, "exact"), dmeta=(None, "exact")))),
    "dwconv": Family(_dw_cases(), _dw_build, _dw_ref, _const(dict(y=(2e-6, "rel")))),
    "dwwgrad": Family(_dwg_cases(), _dwg_build, _dwg_ref, _const(dict(dw=(2e-5, "rel")))),
    "gap": Family(_gap_cases(), _gap_build, _gap_ref, _const(dict(avg=(2e-6, "abs")))),
    "se": Family(_se_cases(), _se_build, _se_ref, _const(dict(scale=(2e-6, "abs")))),
}
ALL_CASES = [c for fam in FAMILIES.values() for c in fam.cases]
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)


def case_id(c: Case) -> str:
    return c.id.replace(" ", "-")
