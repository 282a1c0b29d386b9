"""Edge-shape cases for the fp16-storage ("h8") per-pixel kernels of csrc/fpn_opt_h8.hip, csrc/fpn_h8.hip and csrc/layout_h8.hip: the case
tables, the seeded input builders and the references, in the shape of tests/pixel_edge_cases.py (whose ``Case``, ``Family``, ``gen``,
``case_id``, ``SENTINEL`` and ``SALTS`` are used here).  A reference is plain torch on the CPU, evaluated in fp64 (the yardstick) and in fp32 (the conditioning
check) on the fp16-valued inputs: every stored input is ``x.half().float()``.  No GPU here; tests/test_h8_pixel_edge_cases_cpu.py shows
that every input is fair for its bar and that the bars tell a subtly wrong kernel from a right one, and
tests/test_gpu_h8_pixel_kernel_edges.py holds the kernels to the fp64 results.

Tensors are NCHW here; ``pack_h8`` / ``unpack_h8`` are the layout [N, G, H, W, 8] in plain torch, so no kernel under test prepares or
reads back another one's data.

Bar modes
  exact     equality of the unpacked values, pad channels and the sentinel blocks around an output slice included; by bit pattern
            (signed zeros) except for the max-pool, where max(+0, -0) is either zero.
  h16(coef) |got - want64| <= ulp16(want64) / 2 + coef |want64|, ulp16(v) = 2^(max(floor(log2 |v|), -14) - 10): the one rounding to
            nearest even that h8_pack8 is entitled to, and the fp32 arithmetic ahead of it.  |want64| >= 65520 must come back as the
            infinity of that sign.  A reference may give the coefficient term itself, elementwise, as result ``name!tol``.
  rel       fp32 outputs: |got - want64| <= coef |want64| (GroupNorm mean and rstd);  elem: coef max(1, |want64|) (ELU + 1).

Family                         bar                where the coefficient comes from
  maxpool                      exact (values)     fp16 max is exact
  s2d (+ meta injection)       exact (bits)       data movement; meta is injected as meta.half()
  d2s                          exact (bits)       data movement, the whole destination buffer with its sentinel blocks
  from_h8, to_h8 (plain)       exact (bits)       fp16 -> fp32 is exact; fp32 -> fp16 is x.half().  (The -0 inputs of `to_h8 subnormal 2x8x3x5` found
                                                  nchw_to_h8_kernel storing +0 for -0: x * 1.0f and the conversion had fused into fma(x, 1, +0).)
  pixelshuffle (plain)         exact (bits)       data movement
  to_h8 / pixelshuffle scaled  h16(2^-23) each    one fp32 multiply (2^-24) per multiplier, doubled
  avgpool                      h16(4 * 2^-24)     nine exact adds, a multiply and a divide
  bilinear                     h16(1e-6)          the bar of the fp32 kernel in pixel_edge_cases.py, scales 2 / 4 / 8 only
  elu (ELU + 1, fp32 out)      elem 1e-6          the bar of the fp32 kernel
  gate                         h16(1e-5)          __expf carries about |arg| 2^-24 relative error, |arg| <= 88, twice (weight and sum)
  attention                    h16(1e-5 + 2e-7 sum|w_a|)   the expf term as the gate's; att_tanh is 1e-7 absolute (the kernel's own comment), so the
                                                  score is off by 1e-7 sum|w_a|, which the softmax turns into that much RELATIVE error of a weight,
                                                  once through its numerator and once through its sum
  groupnorm mean, rstd         rel 2^-22          fp64 sums of exact values rounded to fp32 once (2^-24); for |mean| / std <= 1e3
  groupnorm apply              h16, tol = GN_COEF ((|xhat| + |mean| rstd) |gamma| + |beta|)
      The first derivation, 2^-22 (1 + |mean| / std) |want|, does not fit: the rounding of the fp32 mean, 2^-24 |mean|, is an ABSOLUTE error of
      2^-24 |mean| rstd |gamma| whatever xhat is, and the last add rounds at the size of its operands |xhat gamma| and |beta|, so where the result
      cancels (y near 0, which 0.05 randn + 5 data and any beta give in every plane) a correct kernel misses a bar that shrinks with |want|.  The
      coefficient term is therefore taken of the operands, (|xhat| + |mean| rstd) |gamma| + |beta|, not of the result, and GN_COEF is four times
      the distance of torch's fp32 evaluation of the same formula from fp64 in those units (measured over every case of the table:
      3.245 * 2^-24 at most, on `3randn+1 slice 2x20x1x66563 g5`; five roundings of 2^-24 each are the worst case): 13 * 2^-24.  The CPU test
      asserts that no case's fp32 evaluation is further than a quarter of it.

Conditioning rule (the fp32 file's): for every non-exact result torch's fp32 evaluation, rounded to fp16 where the kernel stores fp16, lies
within the bar with a quarter of the coefficient term.  An input that fails gets another seed through ``SALTS`` or another scale, never
another bar.  No reference value is NaN or lies within the coefficient term of 65520.  No case leaves elements out.  To keep torch's fp32
evaluation inside a quarter of avgpool's four roundings, the avgpool data are multiples of 2^-10 below 4 and its multipliers multiples of
1/8, which makes the nine adds and the multiply exact in fp32 and leaves the divide as the only rounding, for torch and for the kernel.
GroupNorm's statistics are fp64 in the reference whatever the dtype (the kernel's documented design); the fp32 evaluation rounds them once.

Deliberate differences, left out of the tables: NaN inputs (the packed-half maximum and torch disagree by design); the gate of an image
whose scores are ALL -inf (torch gives NaN weights, and so does the kernel: exp(-inf - -inf)); +inf and -inf in one avgpool window.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

import pixel_edge_cases as pe
from pixel_edge_cases import Case, Family, SENTINEL, _const, _hw, case_id, gen, h16_worst, same_bits, ulp16  # noqa: F401  (case_id: for the test files)

EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # the kernels take eps as a float
U = 2.0 ** -24
GN_COEF = 13.0 * 2.0 ** -24          # 4 x 3.25 * 2^-24 (measured: torch fp32 against fp64 in operand units, see above)
INF = float("inf")
OUT_HW = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (2, 7), (7, 9)]
FIXED16 = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0]
ELU_FIXED = FIXED16 + [-17.0, -20.0, -INF]
ROW_CAP, LIN_CAP, TILE_CAP = 65535, 32768, 4096          # h8_row_grid's rows / images, slu_grid_1d's blocks, the gate's and GroupNorm apply's tiles

# inputs whose first seed failed the conditioning rule and the seed offset that replaced it (none so far: such an input has an element whose
# fp32 torch result lies within the coefficient term of a tie between two fp16 values, on the other side of it than the fp64 result)
SALTS: Dict[str, int] = {}
pe.SALTS.update(SALTS)


# ---------------------------------------------------------------------------------------------------------------------
# layout, roundings, comparison
# ---------------------------------------------------------------------------------------------------------------------
def r16(t):
    return t.half().float()


def rne(t):
    """fp32 -> fp16, to nearest even, as fp32 values"""
    return t.float().half().float()


def trunc16(t):
    """fp32 -> fp16 toward zero (a wrong kernel)"""
    t = t.float()
    h = t.half()
    bits = h.view(torch.int16).clone()
    bits -= (h.float().abs() > t.abs()).to(torch.int16)          # sign-magnitude: one step toward zero
    return bits.view(torch.float16).float()


def bf16_then_16(t):
    """fp32 -> 8 significant bits -> fp16 (a wrong kernel)"""
    return t.float().bfloat16().float().half().float()


def pack_h8(x):
    """NCHW (fp16-valued) -> [N, ceil(C / 8), H, W, 8] fp16, pad channels 0"""
    n, c, h, w = x.shape
    g = (c + 7) // 8
    y = torch.zeros(n, 8 * g, h, w, dtype=torch.float16)
    y[:, :c] = x.half()
    return y.view(n, g, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def unpack_h8(y):
    """[N, G, H, W, 8] fp16 -> NCHW fp32 with all 8 G channels"""
    n, g, h, w, _ = y.shape
    return y.permute(0, 1, 4, 2, 3).reshape(n, 8 * g, h, w).float()


def pad8(t, value=0.0):
    """NCHW with the channels padded to a multiple of 8"""
    c = t.shape[1]
    return t if c % 8 == 0 else F.pad(t, (0, 0, 0, 0, 0, 8 - c % 8), value=value)


def tol_of(spec, key, want64):
    """the coefficient term of an h16 bar, elementwise"""
    t = want64.get(key + "!tol")
    return t if t is not None else spec[0] * want64[key].double().abs()


def result_fails(case: Case, key: str, got, want64) -> bool:
    """does `got` (fp32 or fp64, CPU) miss the bar of result `key`?"""
    spec = FAMILIES[case.family].bars(case)[key]
    w = want64[key]
    if tuple(got.shape) != tuple(w.shape):
        return True
    if spec[1] == "exact":
        return not (same_bits(got, w) if spec[0] == "bits" else torch.equal(got.double(), w.double()))
    if spec[1] == "h16":
        return not h16_worst(got, w, tol_of(spec, key, want64))[0]
    d = (got.double() - w.double()).abs()
    den = w.double().abs() if spec[1] == "rel" else w.double().abs().clamp_min(1.0)
    return not bool((d <= spec[0] * den).all())


def check(case: Case, got: Dict[str, torch.Tensor], want64, want32):
    """Every result of `got` (CPU, NCHW) against the fp64 reference at the case's bar; prints the worst error next to the bar."""
    bars = FAMILIES[case.family].bars(case)
    assert set(got) == set(bars), f"{case.id}: results {sorted(got)}, bars for {sorted(bars)}"
    for key, spec in bars.items():
        g, w = got[key], want64[key]
        tag = f"{case.id} {key}"
        assert tuple(g.shape) == tuple(w.shape), f"{tag}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
        if spec[1] == "exact":
            same = same_bits(g, w) if spec[0] == "bits" else torch.equal(g.double(), w.double())
            print(f"{tag}: exact ({spec[0]}) {'ok' if same else 'DIFFERS'}")
            assert same, f"{tag}: differs from the reference in {int((g.double() != w.double()).sum())} of {g.numel()} elements"
        elif spec[1] == "h16":
            tol = tol_of(spec, key, want64)
            ok, worst, bad_inf = h16_worst(g, w, tol)
            fin = w.double().abs() < 65520.0
            tol = torch.as_tensor(tol).double().expand(w.shape)
            diff = (g.double() - w.double())[fin].abs().nan_to_num(nan=INF)
            err = float(diff.max()) if bool(fin.any()) else 0.0
            # what the error leaves of the coefficient term once the rounding's half ulp is taken off: the fp32 arithmetic ahead of the store
            pos = tol[fin] > 0
            used = float(((diff - ulp16(w)[fin] / 2)[pos] / tol[fin][pos]).clamp_min(0.0).max()) if bool(pos.any()) else 0.0
            print(f"{tag}: device-fp64 {err:.3e} worst, {worst:.3f} of the bar ulp16 / 2 + tol, {used:.3f} of tol beyond the half ulp (tol up to {float(tol.max()):.3e}), "
                  f"{int((~fin).sum())} overflowing, {bad_inf} of them not the infinity")
            assert ok, f"{tag}: {worst:.3f} of the bar, {bad_inf} overflows that are not the infinity"
        else:
            den = w.double().abs() if spec[1] == "rel" else w.double().abs().clamp_min(1.0)
            d = (g.double() - w.double()).abs()
            ratio = torch.where(d == 0, torch.zeros_like(d), d / den)
            gap = (want32[key].double() - w.double()).abs()
            print(f"{tag}: device-fp64 {float(ratio.max()):.3e} relative, fp32 torch-fp64 {float(torch.where(gap == 0, gap, gap / den).max()):.3e}, bar {spec[0]:.3e}")
            assert bool((d <= spec[0] * den).all()), f"{tag}: {float(ratio.max()):.3e} > {spec[0]:.3e}"


def conditioning(case: Case, want64, want32):
    """Asserts the conditioning rule and the overflow / NaN condition; [(result, fp32 torch's worst share of its quarter bar)]"""
    out = []
    for key, spec in FAMILIES[case.family].bars(case).items():
        w64, w32 = want64[key], want32[key]
        tag = f"{case.id} {key}"
        assert w64.dtype == torch.float64 and w32.dtype == torch.float32, f"{tag}: reference dtypes"
        assert not bool(torch.isnan(w64).any()) and not bool(torch.isnan(w32).any()), f"{tag}: NaN in a reference"
        if spec[1] == "exact":
            assert same_bits(w32, w64), f"{tag}: exact result differs between fp32 and fp64 torch"
            continue
        if spec[1] == "h16":
            tol = torch.as_tensor(tol_of(spec, key, want64)).double()
            near = torch.isfinite(w64) & ((w64.abs() - 65520.0).abs() <= tol)
            assert not bool(near.any()), f"{tag}: {int(near.sum())} reference values within the coefficient term of 65520"
            ok, worst, bad_inf = h16_worst(rne(w32), w64, tol / 4)
            assert ok, f"{tag}: fp32 torch rounded to fp16 is at {worst:.3f} of ulp16 / 2 + tol / 4 ({bad_inf} overflows differ): ill-conditioned input"
            out.append((key, worst))
        else:
            assert bool(torch.isfinite(w64).all()), f"{tag}: reference not finite"
            den = w64.abs() if spec[1] == "rel" else w64.abs().clamp_min(1.0)
            gap = (w32.double() - w64).abs()
            assert bool((gap <= spec[0] / 4 * den).all()), f"{tag}: fp32 torch is further than a quarter of the bar from fp64"
            out.append((key, float(torch.where(gap == 0, gap, gap / (spec[0] / 4 * den)).max())))
    return out


def evaluate(case: Case):
    """(inputs, fp64 results, fp32 results)"""
    return pe.evaluate(case, FAMILIES)


def pattern(shape):
    """an arithmetic pattern of fp16 values (multiples of 1/8 below 256), for the tensors too large for randn"""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.int64)
    return (((idx * 2654435761) % 4093 - 2046).float() / 8.0).view(shape)


def _sprinkle(x, g, values, share=0.4):
    """`share` of x replaced by the listed special values, in equal parts"""
    u = torch.rand(x.shape, generator=g)
    for k, v in enumerate(values):
        lo = share * k / len(values)
        x[(u >= lo) & (u < lo + share / len(values))] = v
    return x


def _pool_shapes():
    """(input H x W, C, N): every output size of OUT_HW from odd and from even inputs, 255 / 256 / 257 output columns in two blocks"""
    out = []
    for k, (oh, ow) in enumerate(OUT_HW):
        pars = [(1, 1), (0, 0)] + ([(1, 0), (0, 1)] if (oh, ow) in ((3, 3), (2, 7)) else [])
        for a, b in pars:
            out.append(((2 * oh - a, 2 * ow - b), (5, 12, 20)[(k + a) % 3], 1 + (k + b) % 2))
    return out + [((3, 2 * ow - ow % 2), 12, 1) for ow in (255, 256, 257)]


# ---------------------------------------------------------------------------------------------------------------------
# max-pool 3x3 / s2 / p1: exact.  `edge`: -inf, both zeros, +-65504 and the smallest subnormals among the values
# ---------------------------------------------------------------------------------------------------------------------
def _mp_cases():
    cs = [Case("maxpool", f"h8 maxpool {kind} {n}x{c}x{_hw(hw)}", dict(n=n, c=c, hw=hw, kind=kind))
          for k, (hw, c, n) in enumerate(_pool_shapes()) for kind in (("randn", "neg", "edge")[k % 3], ("neg", "edge", "randn")[k % 3])]
    return cs + [Case("maxpool", "h8 maxpool round2 rows 1x5x131073x3", dict(n=1, c=5, hw=(131073, 3), kind="edge"), True),
                 Case("maxpool", "h8 maxpool round2 images 65537x8x3x3", dict(n=65537, c=8, hw=(3, 3), kind="neg"), True)]


def _pool_x(c, g, scale):
    p = c.p
    x = r16(torch.randn((p["n"], p["c"]) + p["hw"], generator=g) * scale)
    if p["kind"] == "neg":          # padding must never win
        x = r16(-(x.abs() + 0.125))
    elif p["kind"] == "edge":
        x = _sprinkle(x, g, [-INF, 0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24])
    return x


def _mp_build(c):
    return dict(x=_pool_x(c, gen(c), 2.0))


def _mp_ref(c, i, dt, rnd=None):
    return dict(y=F.max_pool2d(i["x"].to(dt), 3, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------
# average pool 3x3 / s2 / p1 (divisor 9) of x[n % B] * scale[n]: h16(4 * 2^-24)
# ---------------------------------------------------------------------------------------------------------------------
def _ap_cases():
    cs = []
    for k, (hw, c, n) in enumerate(_pool_shapes()):
        mode = ("plain", "scaled", "bcast")[k % 3]
        cs.append(Case("avgpool", f"h8 avgpool {mode} {n}x{c}x{_hw(hw)}", dict(n=n, c=c, hw=hw, mode=mode, kind="grid")))
    cs += [Case("avgpool", f"h8 avgpool {mode} {kind} 2x{c}x{_hw(hw)}", dict(n=2, c=c, hw=hw, mode=mode, kind=kind))
           for kind, mode, c, hw in (("fixed", "plain", 8, (5, 6)), ("fixed", "scaled", 8, (5, 6)), ("edge", "plain", 12, (6, 7)), ("edge", "bcast", 5, (7, 4)),
                                     ("half", "plain", 12, (7, 9)))]
    return cs + [Case("avgpool", "h8 avgpool round2 rows scaled 1x5x131073x3", dict(n=1, c=5, hw=(131073, 3), mode="scaled", kind="grid"), True),
                 Case("avgpool", "h8 avgpool round2 images plain 65537x8x3x3", dict(n=65537, c=8, hw=(3, 3), mode="plain", kind="grid"), True)]


def _ap_build(c):
    g, p = gen(c), c.p
    shape = (p["n"], p["c"]) + p["hw"]
    g8 = 8 * ((p["c"] + 7) // 8)
    n_out = p["n"] * (3 if p["mode"] == "bcast" else 1)
    if p["kind"] == "fixed":          # channel k is the plane of FIXED16[k]: inner outputs are the value itself, the border 6 / 9 and 4 / 9 of it
        x = torch.tensor(FIXED16).view(1, 8, 1, 1).expand(shape).clone()
        scale = torch.full((n_out, g8), 1.25) if p["mode"] == "scaled" else None          # 1.25 * 65504 overflows
    else:
        x = (torch.randn(shape, generator=g) * 256).round().clamp(-4095, 4095) / 1024          # multiples of 2^-10: the nine adds are exact
        if p["kind"] == "half":
            x = r16(torch.randn(shape, generator=g) * 0.25)
        if p["kind"] == "edge":
            x = _sprinkle(x, g, [-INF, 0.0, -0.0, 2.0 ** -14, -2.0 ** -24], share=0.2)
        scale = None if p["mode"] == "plain" else torch.randint(4, 13, (n_out, g8), generator=g).float() / 8
    assert torch.equal(x, r16(x))
    return dict(x=x, scale=scale, n_out=n_out)


def _ap_ref(c, i, dt, rnd=None, include_pad=True):
    x = i["x"].to(dt)[torch.arange(i["n_out"]) % i["x"].shape[0]]
    if i["scale"] is not None:
        x = x * i["scale"].to(dt)[:, :x.shape[1], None, None]
    return dict(y=F.avg_pool2d(x, 3, 2, 1, count_include_pad=include_pad))


# ---------------------------------------------------------------------------------------------------------------------
# space-to-depth, phase-major in whole blocks: y[n, (2p+q) 8G + c] = x[n, c, 2oy+p, 2ox+q] (+ phase (0, 0) alone), the last m of the C
# real channels replaced by meta[n, :, f (2oy+p), f (2ox+q)].half(): exact, bits
# ---------------------------------------------------------------------------------------------------------------------
def _s2d_case(n, c, out, m=0, f=1, phase00=True, tag="", big=False):
    meta = f" meta m{m} f{f}" if m else ""
    return Case("s2d", f"h8 space_to_depth{tag}{meta}{'' if phase00 else ' no00'} {n}x{c}x{2 * out[0]}x{2 * out[1]}",
                dict(n=n, c=c, out=out, m=m, f=f, phase00=phase00), big)


def _s2d_cases():
    cs = [_s2d_case(1 + k % 2, (5, 12, 20)[k % 3], out, phase00=k % 2 == 0) for k, out in enumerate(OUT_HW)]
    cs += [_s2d_case(1, 12, (3, ow), phase00=ow != 256) for ow in (255, 256, 257)]
    for k, (c, m) in enumerate(((8, 1), (8, 8), (5, 5), (20, 6), (12, 5))):
        cs += [_s2d_case(2, c, (3, 3), m, f, phase00=(k + j) % 2 == 0) for j, f in enumerate((1, 2, 4, 8))]
    cs += [_s2d_case(1, 20, (2, 7), 6, 2, phase00=True), _s2d_case(2, 20, (1, 1), 20, 4, phase00=False)]
    return cs + [_s2d_case(1, 8, (65537, 1), 2, 1, tag=" round2 rows", big=True), _s2d_case(65537, 8, (2, 2), tag=" round2 images", big=True)]


def _s2d_build(c):
    g, p = gen(c), c.p
    h, w = 2 * p["out"][0], 2 * p["out"][1]
    x = r16(torch.randn(p["n"], p["c"], h, w, generator=g) * 2)
    if not c.big:
        x = _sprinkle(x, g, [0.0, -0.0, INF, -INF, 65504.0, 2.0 ** -24], share=0.2)
    meta = None
    if p["m"]:          # fp32 values over twelve decades: those past 65520 become an infinity, those below 2^-25 a zero
        f = p["f"]
        meta = torch.randn(p["n"], p["m"], f * h, f * w, generator=g) * 10.0 ** torch.randint(-8, 5, (p["n"], p["m"], f * h, f * w), generator=g).float()
    return dict(x=x, meta=meta)


def _s2d_ref(c, i, dt, rnd=rne, use_f=True):
    p, x = c.p, i["x"]
    n, ch, h, w = x.shape
    xin = pad8(x.to(dt)).clone()
    if i["meta"] is not None:
        f = p["f"]
        xin[:, ch - p["m"]:ch] = rnd(i["meta"][:, :, ::f, ::f] if use_f else i["meta"][:, :, :h, :w]).to(dt)
    res = dict(y=torch.cat([xin[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], 1))
    if p["phase00"]:
        res["y00"] = xin[:, :, ::2, ::2].contiguous()
    return res


def _s2d_bars(c):
    return dict(y=("bits", "exact"), y00=("bits", "exact")) if c.p["phase00"] else dict(y=("bits", "exact"))


# ---------------------------------------------------------------------------------------------------------------------
# depth-to-space, channels ordered (i, j, cout): out[n, co, s h + i, s w + j] = y[n, (i s + j) Cout + co, h, w], into blocks
# [g_off, g_off + Cout / 8) of a buffer filled with the sentinel: exact, bits, the whole buffer
# ---------------------------------------------------------------------------------------------------------------------
def _d2s_case(n, cout, hw, s, gtot=None, g_off=1, tag="", big=False):
    go = cout // 8
    gtot = go + 2 if gtot is None else gtot
    return Case("d2s", f"h8 depth_to_space{tag} s{s} {n}x{s * s * cout}x{_hw(hw)} into {g_off}:{g_off + go} of {gtot}",
                dict(n=n, cout=cout, hw=hw, s=s, gtot=gtot, g_off=g_off), big)


def _d2s_cases():
    cs = [_d2s_case(1 + k % 2, (8, 16)[k % 2], hw, s) for k, hw in enumerate(OUT_HW) for s in ((2, 4, 8)[k % 3], (4, 8, 2)[k % 3])]
    cs += [_d2s_case(1, 16, (2, w), 2) for w in (127, 128, 129)] + [_d2s_case(1, 8, (1, 32), 8), _d2s_case(2, 24, (3, 5), 2, gtot=3, g_off=0)]
    return cs + [_d2s_case(1, 8, (8193, 1), 8, gtot=2, tag=" round2 rows", big=True), _d2s_case(65537, 8, (1, 1), 2, gtot=2, tag=" round2 images", big=True)]


def _d2s_build(c):
    g, p = gen(c), c.p
    x = r16(torch.randn((p["n"], p["s"] ** 2 * p["cout"]) + p["hw"], generator=g) * 2)
    return dict(x=x if c.big else _sprinkle(x, g, [0.0, -0.0, INF, -INF, 65504.0, 2.0 ** -24], share=0.2))


def _d2s_ref(c, i, dt, rnd=None, swap=False):
    p, x = c.p, i["x"].to(dt)
    n, _, h, w = x.shape
    s, co = p["s"], p["cout"]
    v = x.view(n, s, s, co, h, w)
    ps = (v.permute(0, 3, 4, 2, 5, 1) if swap else v.permute(0, 3, 4, 1, 5, 2)).reshape(n, co, s * h, s * w)
    out = torch.full((n, 8 * p["gtot"], s * h, s * w), SENTINEL, dtype=dt)
    out[:, 8 * p["g_off"]:8 * p["g_off"] + co] = ps
    return dict(out=out)


# ---------------------------------------------------------------------------------------------------------------------
# depth-to-space s = 2 of channels ordered (class, i, j) with ELU + 1, fp32 NCHW out: elem 1e-6
# ---------------------------------------------------------------------------------------------------------------------
def _elu_cases():
    cs = [Case("elu", f"h8 d2s elu+1 classes{cl} {n}x{_hw(hw)}", dict(n=n, classes=cl, hw=hw, kind="randn"))
          for k, hw in enumerate(OUT_HW + [(2, 255), (2, 256), (2, 257)]) for cl, n in (((1, 3, 5)[k % 3] if k < len(OUT_HW) else 3, 1 + k % 2),)]
    cs += [Case("elu", f"h8 d2s elu+1 fixed classes{cl} 1x2x3", dict(n=1, classes=cl, hw=(2, 3), kind="fixed")) for cl in (3, 5)]
    return cs + [Case("elu", "h8 d2s elu+1 round2 rows classes1 1x65537x1", dict(n=1, classes=1, hw=(65537, 1), kind="randn"), True),
                 Case("elu", "h8 d2s elu+1 round2 images classes2 65537x1x1", dict(n=65537, classes=2, hw=(1, 1), kind="randn"), True)]


def _elu_build(c):
    g, p = gen(c), c.p
    x = r16(torch.randn((p["n"], 4 * p["classes"]) + p["hw"], generator=g) * 3)
    if p["kind"] == "fixed":          # the list, over and over, along the flattened tensor
        flat = x.view(-1)
        flat[:] = torch.tensor(ELU_FIXED).repeat(flat.numel() // len(ELU_FIXED) + 1)[:flat.numel()]
    return dict(x=x)


def _elu_ref(c, i, dt, rnd=None, swap=False):
    ps = F.pixel_shuffle(i["x"].to(dt), 2)
    if swap:
        n, cl, hh, ww = ps.shape
        ps = ps.view(n, cl, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 5, 4, 3).reshape(n, cl, hh, ww)
    return dict(out=F.elu(ps) + 1)


# ---------------------------------------------------------------------------------------------------------------------
# bilinear up-sampling (align_corners = False), scales 2 / 4 / 8: h16(1e-6)
# ---------------------------------------------------------------------------------------------------------------------
def _bl_case(n, c, hw, s, kind="randn", tag="", big=False):
    return Case("bilinear", f"h8 bilinear{tag} {kind} s{s} {n}x{c}x{_hw(hw)}", dict(n=n, c=c, hw=hw, s=s, kind=kind), big)


def _bl_cases():
    cs = [_bl_case(1 + k % 2, (5, 12, 20)[k % 3], hw, s, ("randn", "wide")[(k + j) % 2]) for k, hw in enumerate(OUT_HW)
          for j, s in enumerate(((2, 4, 8)[k % 3], (4, 8, 2)[k % 3]))]
    cs += [_bl_case(1, 12, (2, w), 2) for w in (127, 128, 129)] + [_bl_case(1, 12, (1, 32), 8)] + [_bl_case(1, 8, (2, 3), s, "fixed") for s in (2, 4, 8)]
    return cs + [_bl_case(1, 8, (8193, 1), 8, tag=" round2 rows", big=True), _bl_case(65537, 8, (1, 1), 2, tag=" round2 images", big=True)]


def _bl_build(c):
    g, p = gen(c), c.p
    shape = (p["n"], p["c"]) + p["hw"]
    if p["kind"] == "fixed":          # channel k is the plane of FIXED16[k], but for one pixel of the opposite sign
        x = torch.tensor(FIXED16).view(1, 8, 1, 1).expand(shape).clone()
        x[:, :, 0, 1] = -x[:, :, 0, 1]
    else:
        x = r16((torch.randn(shape, generator=g) * (2e4 if p["kind"] == "wide" else 0.25)).clamp(-65504.0, 65504.0))
    return dict(x=x)


def _bl_ref(c, i, dt, rnd=None, align=False):
    return dict(y=F.interpolate(i["x"].to(dt), scale_factor=c.p["s"], mode="bilinear", align_corners=align))


def bilinear_by_hand(x, s, clamp=True):
    """fp64 bilinear of bilinear_taps; clamp=False: the second tap past the last row / column reads the 0 beyond the plane (a wrong kernel)"""
    n, c, h, w = x.shape
    xp = F.pad(x.double(), (0, 1, 0, 1))

    def taps(size):
        src = ((torch.arange(s * size, dtype=torch.float64) + 0.5) / s - 0.5).clamp_min(0.0)
        i0 = src.floor().long()
        i1 = i0 + 1
        return i0, (i1.clamp_max(size - 1) if clamp else i1), 1.0 - (src - i0), src - i0

    y0, y1, hl0, hl1 = taps(h)
    x0, x1, wl0, wl1 = taps(w)

    def row(yi):
        r = xp[:, :, yi]
        return r[:, :, :, x0] * wl0 + r[:, :, :, x1] * wl1

    return row(y0) * hl0[:, None] + row(y1) * hl1[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm over the stored values: (mean, rstd) and (x - mean) rstd gamma + beta [-> ReLU]
# ---------------------------------------------------------------------------------------------------------------------
GN_KINDS = ("3randn+1", "0.05randn+5", "const", "onegroupconst", "near65504", "near65504pos", "subnormal", "overflow")


def _gn_case(n, c, groups, hw, kind="3randn+1", relu=False, affine=True, dest="new", tag="", big=False):
    return Case("groupnorm", f"h8 groupnorm{tag} {kind}{' relu' if relu else ''}{'' if affine else ' noaffine'} {dest} {n}x{c}x{_hw(hw)} g{groups}",
                dict(n=n, c=c, groups=groups, hw=hw, kind=kind, relu=relu, affine=affine, dest=dest), big)


def _gn_cases():
    cs = []
    for k, hw in enumerate(((1, 1), (2, 2), (1, 1023), (32, 32), (25, 41), (3, 683))):          # HW = 1, 4, 1023, 1024, 1025, 2049
        cs += [_gn_case(2, 16, 4, hw, ("3randn+1", "0.05randn+5")[k % 2], relu=k % 2 == 1, dest=("new", "slice", "inplace")[k % 3]),
               _gn_case(1, 20, 10, hw, ("0.05randn+5", "3randn+1")[k % 2], relu=k % 2 == 0, affine=k % 3 != 0, dest=("slice", "inplace", "new")[k % 3])]
    # 66 parts of 1009 records, the last of 978, two rounds of the finalize kernel's lanes; 256 parts of 1025, the last of 772
    cs += [_gn_case(1, 8, 2, (1, 66563), "0.05randn+5", relu=True), _gn_case(2, 20, 5, (1, 66563), "3randn+1", dest="slice"),
           _gn_case(1, 8, 8, (1, 262147), "0.05randn+5", dest="inplace"), _gn_case(1, 12, 3, (1, 262147), "3randn+1", relu=True)]
    for c in (8, 16, 20, 24):          # every group width at every slot offset
        cs += [_gn_case(2, c, c // cpg, (3, 5), relu=cpg == 2, affine=cpg != 4, dest="slice" if cpg == 1 else "new") for cpg in (1, 2, 4, 8) if c % cpg == 0]
    for k, kind in enumerate(GN_KINDS[2:]):
        cs += [_gn_case(2, 16, 4, (25, 41), kind, relu=k % 2 == 0), _gn_case(1, 12, 6, (1, 5), kind, relu=k % 2 == 1, dest="slice")]
    return cs + [_gn_case(1, 8, 2, (4, 262219), "3randn+1", relu=True, dest="slice", tag=" round2", big=True)]          # HW = 1 048 876: 4098 tiles


def _gn_build(c):
    g, p = gen(c), c.p
    n, ch, kind = p["n"], p["c"], p["kind"]
    shape = (n, ch) + p["hw"]
    cpg = ch // p["groups"]
    z = torch.randn(shape, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(ch, generator=g) if p["affine"] else None
    beta = 0.3 * torch.randn(ch, generator=g) if p["affine"] else None
    if kind in ("3randn+1", "onegroupconst"):
        x = r16(3 * z + 1)
        if kind == "onegroupconst":
            x[:, :cpg] = r16(torch.tensor(0.3))
    elif kind == "0.05randn+5":
        x = r16(0.05 * z + 5)
    elif kind == "const":          # variance 0: rstd = 1 / sqrt(eps), y = beta
        x = torch.full(shape, 0.0625)
    elif kind.startswith("near65504"):          # 65504 - 32 k, k < 20; both signs, or the positive ones alone (|mean| / std about 350)
        x = 65504.0 - 32.0 * torch.randint(0, 20, shape, generator=g).float()
        if kind == "near65504":
            x = x * torch.sign(z)
    elif kind == "subnormal":          # inputs of a few hundred times 2^-24; with gamma = 2^-10 the outputs are subnormal too
        x = r16(3e-6 * z)
        gamma, beta = (torch.full((ch,), 2.0 ** -10) * (1 + torch.arange(ch) % 3), None) if p["affine"] else (None, None)
    elif kind == "overflow":          # |xhat gamma| reaches 9e4: the outputs past 65520 are infinities
        x = r16(3 * z + 1)
        gamma, beta = (torch.full((ch,), 3.0e4) * (1 - 2 * (torch.arange(ch) % 2)), beta) if p["affine"] else (None, None)
    return dict(x=x, gamma=gamma, beta=beta)


def gn_stats64(x, groups, unbiased=False, drop_tail=0, shift_group=0):
    """fp64 (mean, rstd) [N, groups] of the stored values.  drop_tail: records at the end of every plane left out of the sums;
    shift_group: statistics of the group `shift_group` channels further on (wrong kernels both)"""
    n, ch = x.shape[:2]
    xd = x.double().flatten(2)
    if drop_tail:
        xd = xd[:, :, :-drop_tail]
    if shift_group:
        xd = torch.roll(xd, -shift_group, 1)
    xg = xd.reshape(n, groups, -1)
    return xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=unbiased) + EPS)


def gn_apply(c, i, dt, mean, rstd):
    """y in dt from fp64 statistics rounded to dt, and the fp64 operand magnitude (|xhat| + |mean| rstd) |gamma| + |beta|"""
    p, x = c.p, i["x"]
    ch = x.shape[1]
    cpg = ch // p["groups"]
    gam = torch.ones(ch, dtype=dt) if i["gamma"] is None else i["gamma"].to(dt)
    bet = torch.zeros(ch, dtype=dt) if i["beta"] is None else i["beta"].to(dt)
    mu = mean.to(dt).repeat_interleave(cpg, 1)[:, :, None, None]
    rs = rstd.to(dt).repeat_interleave(cpg, 1)[:, :, None, None]
    y = (x.to(dt) - mu) * (rs * gam.view(1, ch, 1, 1)) + bet.view(1, ch, 1, 1)
    mag = ((x.double() - mu.double()).abs() * rs.double() + mu.double().abs() * rs.double()) * gam.double().abs().view(1, ch, 1, 1) + bet.double().abs().view(1, ch, 1, 1)
    return (F.relu(y) if p["relu"] else y), mag


def _gn_ref(c, i, dt, rnd=None):
    mean, rstd = gn_stats64(i["x"], c.p["groups"])
    y, mag = gn_apply(c, i, dt, mean, rstd)
    res = dict(mean=mean.reshape(-1).to(dt), rstd=rstd.reshape(-1).to(dt), y=y)
    if dt == torch.float64:
        res["y!tol"] = GN_COEF * mag
    return res


# ---------------------------------------------------------------------------------------------------------------------
# x * softmax(score over H W) + x: h16(1e-5)
# ---------------------------------------------------------------------------------------------------------------------
GATE_KINDS = ("4randn", "equal", "peak30", "spread100", "ninf1", "ninfmany", "big1e4")


def _gate_case(n, c, hw, kind, tag="", big=False):
    return Case("gate", f"h8 gate{tag} {kind} {n}x{c}x{_hw(hw)}", dict(n=n, c=c, hw=hw, kind=kind), big)


def _gate_cases():
    cs = []
    for k, hw in enumerate(((1, 1), (1, 3), (2, 2), (5, 1), (3, 341), (32, 32), (25, 41), (1, 4099))):          # HW = 1, 3, 4, 5, 1023, 1024, 1025, 4099
        cs += [_gate_case(1 + k % 2, 12, hw, GATE_KINDS[k % 7]), _gate_case(2 - k % 2, 20, hw, GATE_KINDS[(k + 3) % 7])]
    for hw in ((2, 4), (2, 3), (25, 41), (32, 32)):          # N = 3 with HW % 4 = 0, 2, 1, 0: the other images' statistics show up
        cs += [_gate_case(3, 12, hw, kind) for kind in ("4randn", "spread100")]
    cs += [_gate_case(2, c, hw, kind) for c in (8, 256) for hw in ((2, 2), (1, 5)) for kind in ("4randn", "peak30")]      # one block and 32 blocks of tiny planes
    # blocks shared over grid y (gate_grid_y < G, G no multiple of it): 32 blocks over 21, 3 over 2 (the last workgroup row has one round, the others two), 2 over 1
    cs += [_gate_case(3, 256, (1, 4099), "4randn"), _gate_case(1, 20, (1, 153601), "peak30"), _gate_case(1, 12, (1, 262147), "ninfmany")]
    cs += [_gate_case(1, 12, (5, 205), kind) for kind in GATE_KINDS] + [_gate_case(2, 12, (8, 8), kind) for kind in GATE_KINDS]
    cs += [_gate_case(1, 12, (2, 2), "fixed"), _gate_case(1, 12, (1, 1), "fixed")]
    return cs + [_gate_case(1, 8, (4, 262219), "4randn", tag=" round2", big=True)]


def gate_grid_y(n, c, hw):
    """grid y of spatial_gate_h8_kernel as slu_spatial_softmax_gate_h8 sets it: the blocks g = y, y + grid y, ... share a workgroup"""
    tiles = (hw + 255) // 256
    return max(1, min((1024 + tiles * n - 1) // (tiles * n), (c + 7) // 8, 65535))


def _gate_build(c):
    g, p = gen(c), c.p
    n, ch, (h, w), kind = p["n"], p["c"], p["hw"], p["kind"]
    hw = h * w
    x = r16(torch.randn(n, ch, h, w, generator=g) * 2)
    score = 4 * torch.randn(n, hw, generator=g)
    if n == 3:
        score = score + torch.tensor([-50.0, 0.0, 50.0])[:, None]
    if kind in ("equal", "fixed"):
        score = torch.full((n, hw), 0.75)
        if kind == "fixed":          # weight 1 / HW exactly: channel k is FIXED16[k], times 1.25 (HW = 4) or 2 (HW = 1): 65504 overflows, 32752 gives 65504
            x = torch.tensor(FIXED16 + [32752.0, -32752.0, 2.0 ** -15, -3.0 * 2.0 ** -24]).view(1, 12, 1, 1).expand(n, ch, h, w).clone()
    elif kind == "peak30":
        score[:, hw // 2] = score.amax(1) + 30.0
    elif kind == "spread100":          # ascending: the maximum is the LAST score, behind the last whole group of four
        score = torch.linspace(-50.0, 50.0, hw).repeat(n, 1) if hw > 1 else score
    elif kind == "ninf1":
        score[:, hw // 3] = -INF if hw > 1 else score[:, hw // 3]
    elif kind == "ninfmany":          # whole runs of -inf (groups of four and a thread's whole share) with finite scores between
        keep = torch.rand(n, hw, generator=g) < 0.1
        keep[:, hw - 1] = True
        score = torch.where(keep, score, torch.full_like(score, -INF))
    elif kind == "big1e4":
        score = 1e4 + 0.5 * torch.randn(n, hw, generator=g)
    return dict(x=x, score=score.view(n, 1, h, w).contiguous())


def _gate_ref(c, i, dt, rnd=None):
    x, s = i["x"].to(dt), i["score"].to(dt)
    n = x.shape[0]
    return dict(out=x * torch.softmax(s.view(n, -1), -1).view_as(s) + x)


# ---------------------------------------------------------------------------------------------------------------------
# out = v * softmax_W(b_a + sum_c w_a[c] tanh(t[c])), (t, v) the channel halves of tv: h16(1e-5 + 2e-7 sum |w_a|)
# ---------------------------------------------------------------------------------------------------------------------
def _att_case(n, c, h, w, tkind="randn", spread=3):
    return Case("attention", f"h8 attention t {tkind} spread{spread} {n}x{c}x{h}x{w}", dict(n=n, c=c, h=h, w=w, tkind=tkind, spread=spread))


def _att_cases():
    cs = [_att_case(2, 8, 1 + 2 * (k % 2), w, ("randn", "sat", "small")[k % 3], (3, 0, 60)[k % 3]) for k, w in enumerate((1, 2, 255, 256, 257, 4096))]
    cs += [_att_case(1, 64, 3, 257, "randn", 60), _att_case(2, 64, 1, 2, "sat", 3), _att_case(1, 512, 1, 256, "randn", 3), _att_case(1, 512, 3, 2, "small", 60),
           _att_case(1, 512, 1, 300, "sat", 60), _att_case(3, 16, 2, 300, "randn", 3), _att_case(1, 8, 1, 300, "randn", 0), _att_case(1, 8, 3, 257, "fixed", 3), _att_case(2, 16, 3, 1, "fixed", 3)]
    return cs


def _att_build(c):
    g, p = gen(c), c.p
    n, ch, h, w = p["n"], p["c"], p["h"], p["w"]
    t = torch.randn(n, ch, h, w, generator=g)
    if p["tkind"] == "small":
        t = t * 1e-3
    elif p["tkind"] == "sat":          # most values saturate tanh; the rest decide the score
        t = torch.where(torch.rand(t.shape, generator=g) < 0.7, torch.tensor([20.0, -20.0, 65504.0, -65504.0])[torch.randint(0, 4, t.shape, generator=g)], t)
    v = torch.randn(n, ch, h, w, generator=g) * 2
    if p["tkind"] == "fixed":          # the values of the list as v: with W = 1 the weight is 1 and the products are the list itself (a weight <= 1 cannot overflow);
        # with W = 257 the products are about 1 / 257 of it, down into the subnormals
        v = torch.tensor(FIXED16).repeat(n * ch * h * w // 8 + 1)[:n * ch * h * w].view(n, ch, h, w).clone()
    w_a = torch.randn(ch, generator=g) / ch ** 0.5 * (p["spread"] / 3.0)
    return dict(tv=r16(torch.cat([t, v], 1)), w_a=w_a, b_a=torch.randn(1, generator=g))


def _att_ref(c, i, dt, rnd=None, first=None):
    ch = c.p["c"]
    tv = i["tv"].to(dt)
    t, v = tv[:, :ch], tv[:, ch:]
    s = i["b_a"].to(dt) + (torch.tanh(t) * i["w_a"].to(dt).view(1, ch, 1, 1)).sum(1, keepdim=True)
    if first is None:
        p = torch.softmax(s, -1)
    else:          # the sum over the first `first` columns only (a wrong kernel)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        p = e / e[..., :first].sum(-1, keepdim=True)
    res = dict(out=v * p)
    if dt == torch.float64:
        res["out!tol"] = (1e-5 + 2e-7 * float(i["w_a"].double().abs().sum())) * res["out"].abs()
    return res


# ---------------------------------------------------------------------------------------------------------------------
# fp32 NCHW -> h8 [times scale[n, c]] and back
# ---------------------------------------------------------------------------------------------------------------------
ROUND2_HW = LIN_CAP * 256 + 257          # records of one plane: 8 388 865, a second round of the 32 768 x 256 grid with a ragged end


def _to_cases():
    cs = [Case("to_h8", f"h8 to_h8 {kind}{' scaled' if sc else ''} 2x{c}x3x5", dict(n=2, c=c, hw=(3, 5), kind=kind, scaled=sc))
          for k, c in enumerate((1, 7, 8, 9, 20)) for kind, sc in ((("randn", "overflow", "subnormal")[k % 3], False), (("overflow", "subnormal", "randn")[k % 3], True),
                                                                   ("randn", k % 2 == 0))]
    cs = list({c.id: c for c in cs}.values())
    return cs + [Case("to_h8", f"h8 to_h8 round2 pattern 1x2x1x{ROUND2_HW}", dict(n=1, c=2, hw=(1, ROUND2_HW), kind="pattern", scaled=False), True)]


def _to_build(c):
    g, p = gen(c), c.p
    shape = (p["n"], p["c"]) + p["hw"]
    if p["kind"] == "pattern":
        return dict(x=pattern(shape) + 2.0 ** -6, scale=None)          # one bit below fp16's last at 128 and above: ties and roundings both ways
    x = torch.randn(shape, generator=g)
    scale = 0.5 + torch.rand(p["n"], p["c"], generator=g) if p["scaled"] else None
    if p["kind"] == "randn":
        x = x * 3
    elif p["kind"] == "overflow":
        if p["scaled"]:          # well past 65520 / 0.5 or well inside: the product is never near the threshold
            x = torch.where(torch.rand(shape, generator=g) < 0.5, torch.sign(x) * 2.0e5 * (1 + x.abs()), x * 1e3)
        else:
            x = _sprinkle(x * 2e4, g, [65519.996, 65520.0, 65520.004, -65519.996, -65520.0, 1e5, -3e38, 65504.0, 65488.0, 65472.0], share=0.6)
    elif p["kind"] == "subnormal":          # ties between subnormals, half the smallest one (to zero) and just above it
        x = _sprinkle(x * 3e-6, g, [2.0 ** -25, -2.0 ** -25, 2.0 ** -25 * 1.0000002, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -0.0, 2.0 ** -14 - 2.0 ** -25, 1e-30], share=0.5)
    return dict(x=x, scale=scale)


def _to_ref(c, i, dt, rnd=rne):
    if i["scale"] is None:
        return dict(y=rnd(i["x"]).to(dt))
    return dict(y=i["x"].to(dt) * i["scale"].to(dt)[:, :, None, None])


def _to_bars(c):
    return dict(y=(2 * U, "h16")) if c.p["scaled"] else dict(y=("bits", "exact"))


def _from_cases():
    cs = [Case("from_h8", f"h8 from_h8 2x{c}x3x5", dict(n=2, c=c, hw=(3, 5))) for c in (1, 7, 8, 9, 20)]
    return cs + [Case("from_h8", f"h8 from_h8 round2 pattern 1x2x1x{ROUND2_HW}", dict(n=1, c=2, hw=(1, ROUND2_HW)), True)]


def _from_build(c):
    shape = (c.p["n"], c.p["c"]) + c.p["hw"]
    if c.big:
        return dict(x=pattern(shape))
    g = gen(c)
    return dict(x=_sprinkle(r16(torch.randn(shape, generator=g) * 2), g, [0.0, -0.0, INF, -INF, 65504.0, -2.0 ** -24, 2.0 ** -14], share=0.3))


def _from_ref(c, i, dt, rnd=None):
    return dict(y=i["x"].to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# nn.PixelShuffle(2) of x * s_in[n, c_in], times s_out[n, c_out]
# ---------------------------------------------------------------------------------------------------------------------
PS_MODES = {"plain": (False, False), "in": (True, False), "out": (False, True), "both": (True, True)}


def _ps_cases():
    return [Case("pixelshuffle", f"h8 pixel_shuffle {mode} {n}x{8 * gi}x{_hw(hw)}", dict(n=n, gi=gi, hw=hw, mode=mode))
            for k, gi in enumerate((1, 2, 4, 5)) for mode in PS_MODES for n, hw in ((1 + k % 2, ((3, 5), (1, 1), (2, 7), (5, 1))[k]),)] + \
        [Case("pixelshuffle", f"h8 pixel_shuffle {mode} 1x40x2x{w}", dict(n=1, gi=5, hw=(2, w), mode=mode)) for w, mode in ((127, "plain"), (128, "both"), (129, "plain"))]


def _ps_build(c):
    g, p = gen(c), c.p
    n, gi = p["n"], p["gi"]
    x = r16(torch.randn((n, 8 * gi) + p["hw"], generator=g) * 2)
    s_in, s_out = PS_MODES[p["mode"]]
    if p["mode"] == "plain":
        x = _sprinkle(x, g, [0.0, -0.0, INF, -INF, 65504.0, 2.0 ** -24], share=0.2)
    else:          # the list where a multiplier sees it: 65504 times a multiplier above 1.0003 overflows, 2^-24 times one below 0.5 vanishes
        x = _sprinkle(x, g, FIXED16, share=0.2)
    return dict(x=x, s_in=0.25 + 1.5 * torch.rand(n, 8 * gi, generator=g) if s_in else None, s_out=0.25 + 1.5 * torch.rand(n, 2 * gi, generator=g) if s_out else None)


def _ps_ref(c, i, dt, rnd=None, swap=False):
    x = i["x"].to(dt)
    if i["s_in"] is not None:
        x = x * i["s_in"].to(dt)[:, :, None, None]
    if swap:
        x = x.view(x.shape[0], -1, 2, 2, x.shape[2], x.shape[3]).transpose(2, 3).reshape(x.shape)
    y = F.pixel_shuffle(x, 2)
    if i["s_out"] is not None:
        y = y * i["s_out"].to(dt)[:, :, None, None]
    return dict(y=y)


def _ps_bars(c):
    k = sum(PS_MODES[c.p["mode"]])
    return dict(y=(2 * U * k, "h16")) if k else dict(y=("bits", "exact"))


FAMILIES: Dict[str, Family] = {
    "maxpool": Family(_mp_cases(), _mp_build, _mp_ref, _const(dict(y=("values", "exact")))),
    "avgpool": Family(_ap_cases(), _ap_build, _ap_ref, _const(dict(y=(4 * U, "h16")))),
    "s2d": Family(_s2d_cases(), _s2d_build, _s2d_ref, _s2d_bars),
    "d2s": Family(_d2s_cases(), _d2s_build, _d2s_ref, _const(dict(out=("bits", "exact")))),
    "elu": Family(_elu_cases(), _elu_build, _elu_ref, _const(dict(out=(1e-6, "elem")))),
    "bilinear": Family(_bl_cases(), _bl_build, _bl_ref, _const(dict(y=(1e-6, "h16")))),
    "groupnorm": Family(_gn_cases(), _gn_build, _gn_ref, _const(dict(mean=(4 * U, "rel"), rstd=(4 * U, "rel"), y=(None, "h16")))),
    "gate": Family(_gate_cases(), _gate_build, _gate_ref, _const(dict(out=(1e-5, "h16")))),
    "attention": Family(_att_cases(), _att_build, _att_ref, _const(dict(out=(None, "h16")))),
    "to_h8": Family(_to_cases(), _to_build, _to_ref, _to_bars),
    "from_h8": Family(_from_cases(), _from_build, _from_ref, _const(dict(y=("bits", "exact")))),
    "pixelshuffle": Family(_ps_cases(), _ps_build, _ps_ref, _ps_bars),
}
ALL_CASES = [c for fam in FAMILIES.values() for c in fam.cases]
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
STORED = dict(maxpool=("x",), avgpool=("x",), s2d=("x",), d2s=("x",), elu=("x",), bilinear=("x",), groupnorm=("x",), gate=("x",), attention=("tv",), to_h8=(),
              from_h8=("x",), pixelshuffle=("x",))          # the inputs a kernel reads as fp16 records


# ---------------------------------------------------------------------------------------------------------------------
# wrong kernels, written as variants of the references: tests/test_h8_pixel_edge_cases_cpu.py asserts that each is caught by a case
# ---------------------------------------------------------------------------------------------------------------------
def _gn_wrong(unbiased=False, drop_tail=0, shift_group=0, one_pass32=False):
    def fn(c, i):
        if drop_tail and c.p["hw"][0] * c.p["hw"][1] <= drop_tail:
            return None
        mean, rstd = gn_stats64(i["x"], c.p["groups"], unbiased=unbiased, drop_tail=drop_tail, shift_group=shift_group * (c.p["c"] // c.p["groups"]))
        if one_pass32:          # E[x^2] - mean^2 with fp32 sums
            xg = i["x"].reshape(i["x"].shape[0], c.p["groups"], -1)
            m = xg.mean(-1)
            mean, rstd = m.double(), (1.0 / torch.sqrt(((xg * xg).mean(-1) - m * m).clamp_min(0) + EPS)).double()
        return dict(mean=mean.reshape(-1), rstd=rstd.reshape(-1), y=gn_apply(c, i, torch.float64, mean, rstd)[0])
    return fn


def _gate_wrong_max(c, i):
    """the maximum over the first HW & ~3 scores only, in fp32 as the kernel would compute it"""
    x, s = i["x"], i["score"].view(i["x"].shape[0], -1)
    head = s[:, :s.shape[1] & ~3]
    if head.shape[1] == 0:
        return None
    e = torch.exp(s - head.amax(1, keepdim=True))
    return dict(out=x * (e / e.sum(1, keepdim=True)).view_as(i["score"]) + x)


WRONG = {
    "maxpool": {"pad 0 instead of -inf": lambda c, i: dict(y=F.max_pool2d(F.pad(i["x"].double(), (1, 1, 1, 1)), 3, 2, 0))},
    "avgpool": {"divided by the count of valid taps": lambda c, i: _ap_ref(c, i, torch.float64, include_pad=False)},
    "bilinear": {"source index not clamped at the last row / column": lambda c, i: dict(y=bilinear_by_hand(i["x"], c.p["s"], clamp=False)),
                 "align_corners=True weights": lambda c, i: _bl_ref(c, i, torch.float64, align=True)},
    "groupnorm": {"unbiased variance": _gn_wrong(unbiased=True), "the last ragged chunk dropped from the sums": _gn_wrong(drop_tail=772),
                  "fp32 one-pass variance": _gn_wrong(one_pass32=True), "the wrong group for slot k0": _gn_wrong(shift_group=1)},
    "gate": {"weight dropped (out = x)": lambda c, i: dict(out=i["x"].double()), "maximum over the first HW & ~3 scores only": _gate_wrong_max},
    "attention": {"softmax over the first 256 columns only": lambda c, i: dict(out=_att_ref(c, i, torch.float64, first=256)["out"])},
    "d2s": {"i and j swapped": lambda c, i: _d2s_ref(c, i, torch.float64, swap=True)},
    "elu": {"i and j swapped": lambda c, i: _elu_ref(c, i, torch.float64, swap=True)},
    "pixelshuffle": {"i and j swapped": lambda c, i: _ps_ref(c, i, torch.float64, swap=True)},
    "s2d": {"f ignored": lambda c, i: _s2d_ref(c, i, torch.float64, use_f=False) if c.p["m"] else None},
}
ROUNDINGS = {"truncated toward zero": trunc16, "rounded to 8 bits, then to fp16": bf16_then_16}
# the families that round a computed (or converted) value to fp16: the others move fp16 records or store fp32
FP16_STORING = ("avgpool", "bilinear", "groupnorm", "gate", "attention", "to_h8", "pixelshuffle", "s2d")


def wrongly_rounded(case: Case, inputs, rnd):
    """{result: the fp32 torch evaluation with the wrong rounding `rnd` to fp16} of the results that a kernel rounds"""
    fam = FAMILIES[case.family]
    res = fam.ref(case, inputs, torch.float32, rnd=rnd)
    return {k: (rnd(v) if spec[1] == "h16" else v) for k, spec in fam.bars(case).items() for v in (res[k],) if spec[1] in ("h16", "exact")}
