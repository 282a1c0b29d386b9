"""Ordinary (random) conv cases for the split-fp16 kernel, with their CPU references computed once and shared:
test_gpu_f16x3_split.py runs the kernels on them, test_f16x3_restatement_cpu.py shows that a lost piece of a `lo` image is far
outside the bar they use.  Values are drawn as test_gpu_f16x3._run draws them.

  want64      the exact operator in fp64 (the fp32 conv input times the fp32 weight)
  want_split  f16x3_restatement.fused_conv_split: the three-term sum in fp64 -- the kernel differs from it by fp32 accumulation only
  e_ref       max|fp32 CPU fused_conv - want64|: what one fp32 summation order costs on this case
  S           max|want64| (no floor)
  bar         4 e_ref + 1e-7 S   (4: the project's margin for another fp32 summation order, test_gpu_backward.py; 1e-7 S: one fp32
              rounding of the stored value, for cases where the CPU conv happens to be exact)
MARGIN: the one case whose correct kernels need more than 4.  K = 2 880 (PixelShuffle 256 + skip 256 -> 128, 3x3) is 2.5 x deeper than
any other case; the kernels add K terms in one k-ordered fp32 chain, whose error grows with sqrt(K), where the CPU conv's blocked sums
(e_ref) do not.  Measured on the MI355X: fp32 kernel 8.45 e_ref (1.6e-6 S), split-fp16 kernel 4.65 e_ref (9.0e-7 S); both are bit-exact
on the lattice version of this very shape (test_gpu_conv_lattice.py).  Margin 16 there; the smallest lost-lo difference of that case is
147 x the 4-bar, so 37 x the 16-bar (test_f16x3_restatement_cpu.py asserts > 10 x with whatever bar the case carries)."""
import functools
from types import SimpleNamespace

import torch

from conv_lattice_cases import small_cases
from f16x3_restatement import fused_conv64, fused_conv_split, fused_conv_split_mfma
from oracle import salsanext as osalsa

SLOPE = 0.01
SWEEP_EX = [14, 0, -6, -12, -18, -24]
SWEEP_EW = [0, -6, -12]
# (id, Cin parts, Cout, N, H, W, family)
SWEEP_SHAPES = [("64->32|k3d1|1x8x64", [64], 32, 1, 8, 64, (3, 1, 1)),
                ("21->40|k3d2|3x5x33", [21], 40, 3, 5, 33, (3, 2, 2)),
                ("32->64|k1d1|1x16x64", [32], 64, 1, 16, 64, (1, 1, 0))]


MARGIN = {"shuffle|k3d1|256+256->128|N2|8x64": 16}


def _finish(c, margin=4):
    args = (c.srcs, c.wgt, c.bias, c.pad, c.dil, c.slope, c.bn_a, c.bn_b, c.res)
    c.want64 = fused_conv64(*args)
    c.want_split = fused_conv_split(*args)
    c.want32 = osalsa.fused_conv(*args)
    c.e_ref = float((c.want32.double() - c.want64).abs().max())
    c.S = float(c.want64.abs().max())
    c.bar = margin * c.e_ref + 1e-7 * c.S
    return c


def random_case(n, cin_parts, cout, h, w, fam, seed, scales=False, ps_first=False, bias=True, bn=True, act=True, resid=True, margin=4):
    k, dil, pad = fam
    g = torch.Generator().manual_seed(seed)
    srcs, cin = [], 0
    for i, c in enumerate(cin_parts):
        ps = ps_first and i == 0
        t = torch.randn(n, c, h // 2 if ps else h, w // 2 if ps else w, generator=g)
        s = (torch.rand(n, c, generator=g) > 0.2).float() * 1.25 if scales else None
        srcs.append((t, s, ps))
        cin += c // 4 if ps else c
    wgt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b_ = torch.randn(cout, generator=g) * 0.1 if bias else None
    bn_a = torch.rand(cout, generator=g) + 0.5 if bn else None
    bn_b = torch.randn(cout, generator=g) * 0.1 if bn else None
    res = torch.randn(n, cout, h, w, generator=g) if resid else None
    return _finish(SimpleNamespace(srcs=srcs, wgt=wgt, bias=b_, bn_a=bn_a, bn_b=bn_b, res=res, slope=SLOPE if act else None,
                                   k=k, dil=dil, pad=pad), margin)


SPLIT_CASES = small_cases()


@functools.lru_cache(maxsize=None)
def split_case(i):
    """Case i of SPLIT_CASES with its references, computed once per process and left unchanged."""
    return random_case(margin=MARGIN.get(SPLIT_CASES[i][0], 4), **SPLIT_CASES[i][1])


@functools.lru_cache(maxsize=None)
def sweep_case(shape_i, ex, ew):
    """The bare conv (no bias, activation, BatchNorm or residual: they would set a scale of their own) of N(0, 1) inputs times 2^ex and
    He-scaled weights times 2^ew.  Powers of two, so every cell of one shape has the same mantissas."""
    _, parts, cout, n, h, w, fam = SWEEP_SHAPES[shape_i]
    k, dil, pad = fam
    g = torch.Generator().manual_seed(100 + shape_i)
    x = torch.randn(n, parts[0], h, w, generator=g)
    wgt = torch.randn(cout, parts[0], k, k, generator=g) / (parts[0] * k * k) ** 0.5
    c = SimpleNamespace(srcs=[(x * 2.0 ** ex, None, False)], wgt=wgt * 2.0 ** ew, bias=None, bn_a=None, bn_b=None, res=None, slope=None,
                        k=k, dil=dil, pad=pad)
    c.rms_x, c.rms_w = float(c.srcs[0][0].square().mean().sqrt()), float(c.wgt.square().mean().sqrt())
    _finish(c)
    # the same sum through the model of the matrix core's block alignment (fused_conv_split_mfma).  A cell is `affected` when the model
    # itself leaves the plain restatement by more than the bar: decided on the CPU, from the operands, never from what a kernel returns
    c.want_mfma = fused_conv_split_mfma(c.srcs, c.wgt, None, c.pad, c.dil)
    c.model_gap = float((c.want_mfma - c.want_split).abs().max())
    c.affected = c.model_gap > c.bar
    return c


def lost_lo_variants(kw, cin, k):
    """Ways a kernel could lose part of a `lo` image, as fused_conv_split arguments: name -> (operand whose lo is touched, kwargs).
    kw: the case's lattice_case / random_case kwargs; cin: conv input channels; k: kernel size."""
    tap = torch.ones(k, k)
    tap[k - 1, k - 1] = 0
    first, last = torch.ones(1, 1, 1, kw["w"]), torch.ones(1, 1, 1, kw["w"])
    first[..., 0], last[..., -1] = 0, 0
    v = {"x-lo term left out": ("x", dict(terms=("hh", "hl"))),
         "w-lo term left out": ("w", dict(terms=("hh", "lh"))),
         "x-lo zeroed at one tap": ("x", dict(x_lo_tap_mask=tap)),
         "w-lo zeroed at one tap": ("w", dict(w_lo_mask=tap[None, None])),
         "x-lo zeroed in the first column": ("x", dict(x_lo_mask=first)),
         "x-lo zeroed in the last column": ("x", dict(x_lo_mask=last))}
    if cin % 16:
        m = torch.ones(1, cin, 1, 1)
        m[:, cin - cin % 16:] = 0
        v["x-lo zeroed in the last K=16 chunk"] = ("x", dict(x_lo_mask=m))
        v["w-lo zeroed in the last K=16 chunk"] = ("w", dict(w_lo_mask=m))
    if len(kw["cin_parts"]) > 1:
        c0 = kw["cin_parts"][0] // (4 if kw.get("ps_first") else 1)
        m = torch.ones(1, cin, 1, 1)
        m[:, c0:c0 + kw["cin_parts"][1]] = 0
        v["x-lo zeroed in the second source"] = ("x", dict(x_lo_mask=m))
        v["w-lo zeroed in the second source"] = ("w", dict(w_lo_mask=m))
    return v
