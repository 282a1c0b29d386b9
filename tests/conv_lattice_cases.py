"""Conv inputs whose answer is exact in any summation order, for bit-equality tests of conv2d.hip and conv2d_f16x3.hip.

Two orientations, so that each `lo` path of the split-fp16 kernel is exercised with the dropped lo*lo term exactly zero:
  "x"  the input carries a lo:   x = +-(a + b/4096), a in {0..3}, b in 0..7   (b/1024 with multipliers, so 1.25 x still splits exactly);
                                 weights from {0, +-1/2, +-1, +-2}
  "w"  the weight carries a lo:  w = +-(a + b/4096)/2, a in {0, 1, 2}, b in 0..7;   x a small integer (+-1, +-2; +-4 with multipliers,
                                 so that 1.25 x is an integer), thinned with zeros
Both: bias, bn_b, residual multiples of 1/4 in [-2, 2]; bn_a in {1/2, 1, 2, -1}; slope 1/4; multipliers {0, 1.25}; `big` scales x by 16.

Every product lies on the grid g = 2^-13 (x 16 with big).  lattice_case() asserts, for every case it returns:
  * hi + lo == operand for the operand that carries a lo; every nonzero lo is a normal fp16 (|lo| >= 2^-14); at least half of that
    operand's elements have lo != 0; the other operand has lo == 0 everywhere;
  * every partial sum, in any order, is an exact fp32: either the worst-case bound  max|x| * max_co sum|w[co]| + epilogue slack < 2^24 g
    (independent of N, H, W: the weights are drawn from the seed alone, so the bound proved at one N holds at every N), or, with
    verify=True, conv(|x|, |w|) in fp64 < 2^24 g at every output.  Cases too deep for the worst-case bound (K = 2 880) need verify=True;
  * with verify=True: every intermediate value of the epilogue is an exact fp32, and the fp64 answer, the fp32 CPU fused_conv and
    fused_conv_split agree bit for bit.
These are conditions, not tolerances."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from f16x3_restatement import F16_MIN_NORMAL, conv_input, fused_conv64, fused_conv_split, split
from oracle import salsanext as osalsa

SLOPE = 0.25
GRID = 2.0 ** -13
OFFSET_MAX = 2.0                                   # |bias|, |bn_b|, |resid| <= 2
# the leaky (x 1/4) and bn_a = 1/2 paths move a value to the grid g / 8 without changing its bit count; bn_b and the residual then add
# up to 2 each on that grid: |conv| + |bias| + 8 (|bn_b| + |resid|) < 2^24 g keeps every epilogue intermediate exact
EPI_SLACK = OFFSET_MAX + 8 * 2 * OFFSET_MAX
X_A = torch.tensor([0., 1., 1., 2., 2., 2., 3., 3.])
W_A = torch.tensor([0., 1., 1., 1., 1., 1., 2., 2.])
W_MAG = torch.tensor([0.5, 1.0, 2.0])
BN_A = torch.tensor([0.5, 1.0, 2.0, -1.0])


def _lattice_table(a_table, den):
    """The 128 values +-(a + b / den): code r has a = a_table[r & 7], b = (r >> 3) & 7, sign = r >> 6."""
    r = torch.arange(128)
    v = a_table[r & 7] + ((r >> 3) & 7).float() / den
    return torch.where((r >> 6) > 0, -v, v)


QUARTERS = torch.arange(-8, 9).float() / 4


def _draw(g, shape, table):
    """Elements drawn uniformly from a value table, and their codes (every per-value condition can then be checked on the table)."""
    idx = torch.randint(0, table.numel(), shape, generator=g, dtype=torch.int32)
    return table[idx], idx


def _quarters(g, shape):
    return _draw(g, shape, QUARTERS)[0]


def _keep(g, shape, p):
    return (torch.rand(shape, generator=g) < p).float()


def _exact32(v):
    return bool((v.float().double() == v).all())


def lattice_case(n, cin_parts, cout, h, w, fam, seed, orient, scales=False, ps_first=False, bias=True, bn=True, act=True, resid=True,
                 big=False, verify=True):
    """One case as CPU tensors: SimpleNamespace(srcs, wgt, bias, bn_a, bn_b, res, slope, k, dil, pad, want, worst_case, bound).
    want is the fp32 CPU fused_conv answer (exact on the lattice)."""
    assert orient in ("x", "w")
    k, dil, pad = fam
    gw, gx = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 7919)
    mult = 16.0 if big else 1.0
    g = GRID * mult
    limit = 2.0 ** 24 * g - EPI_SLACK
    cin = sum(c // 4 if (ps_first and i == 0) else c for i, c in enumerate(cin_parts))
    K = cin * k * k
    sc = 1.25 if scales else 1.0
    if orient == "x":
        x_max, x_mean = (3 + 7 / (1024 if scales else 4096)) * sc * mult, 1.8 * sc * mult
        w_mean = 7 / 6
    else:
        x_max = x_mean = (5.0 if scales else 2.0) * mult           # x thinned below; x_mean is that of a nonzero element
        if not scales:
            x_mean = 1.5 * mult
        w_mean = 0.85 * 9 / 16
    # --- weights: from the seed alone (never from N, H, W) ---
    wshape = (cout, cin, k, k)
    if orient == "x":
        p_wc = 0.7 * limit / (K * x_max * w_mean)
        worst_case = p_wc >= 0.2
        p = min(0.75, p_wc) if worst_case else min(0.75, 0.45 * limit / (K * x_mean * w_mean))
        wgt = W_MAG[torch.randint(0, 3, wshape, generator=gw)] * (torch.randint(0, 2, wshape, generator=gw) * 2 - 1).float()
        wgt = wgt * _keep(gw, wshape, p)
        px = 1.0
    else:
        wgt = _draw(gw, wshape, _lattice_table(W_A, 4096) / 2)[0] * _keep(gw, wshape, 0.85)
        worst_case = 1.3 * K * x_max * w_mean < limit
        px = 0.6 if worst_case else min(0.6, 0.45 * limit / (K * x_mean * (0.8 if scales else 1.0) * w_mean))
    b_ = _quarters(gw, (cout,)) if bias else None
    bn_a = BN_A[torch.randint(0, 4, (cout,), generator=gw)] if bn else None
    bn_b = _quarters(gw, (cout,)) if bn else None
    # --- sources: every element is table[code] * mult (* its multiplier), so per-value conditions are checked on the table ---
    if orient == "x":
        table = _lattice_table(X_A, 1024 if scales else 4096) * mult
    else:
        nzv = max(4, 4 * round(px * 25))                                  # of 100 codes: +-4 with multipliers (1.25 x an integer), else +-1, +-2
        vals = torch.tensor([4., -4., 4., -4.] if scales else [1., -1., 2., -2.])
        table = torch.cat([vals.repeat(nzv // 4), torch.zeros(100 - nzv)]) * mult
    hi_t, lo_t = split(table * sc)
    assert bool((hi_t.double() + lo_t.double() == (table * sc).double()).all()), "hi + lo != operand"
    if orient == "x":
        assert float(lo_t[lo_t != 0].abs().min()) >= F16_MIN_NORMAL, "a nonzero lo is an fp16 subnormal"
    else:
        assert not bool(lo_t.any()), "the other operand carries a lo"
    srcs, n_lo, n_all = [], 0, 0
    for i, c in enumerate(cin_parts):
        ps = ps_first and i == 0
        t, idx = _draw(gx, (n, c, h // 2 if ps else h, w // 2 if ps else w), table)
        s = (torch.rand(n, c, generator=gx) > 0.2).float() * 1.25 if scales else None
        srcs.append((t, s, ps))
        carries = (lo_t != 0)[idx]
        n_lo += int((carries & (s != 0)[:, :, None, None]).sum()) if scales else int(carries.sum())
        n_all += idx.numel()
    res = _quarters(gx, (n, cout, h, w)) if resid else None
    slope = SLOPE if act else None
    if orient == "x":
        assert n_lo >= 0.5 * n_all, f"only {n_lo / n_all:.3f} of the input's elements carry a lo"
    else:
        hi, lo = split(wgt)
        nz = lo != 0
        assert bool((hi.double() + lo.double() == wgt.double()).all()), "hi + lo != operand"
        assert float(lo[nz].abs().min()) >= F16_MIN_NORMAL, "a nonzero lo is an fp16 subnormal"
        assert float(nz.float().mean()) >= 0.5, f"only {float(nz.float().mean()):.3f} of the weight's elements carry a lo"
    if orient == "x":
        assert not bool(split(wgt)[1].any()), "the other operand carries a lo"
    xin = conv_input(srcs) if verify else None
    if verify:                                                            # the same conditions, element by element
        lo_op, plain_op = (xin, wgt) if orient == "x" else (wgt, xin)
        hi, lo = split(lo_op)
        assert bool((hi.double() + lo.double() == lo_op.double()).all()) and float(lo[lo != 0].abs().min()) >= F16_MIN_NORMAL
        assert float((lo != 0).float().mean()) >= 0.5 and not bool(split(plain_op)[1].any())
        assert float(xin.abs().max()) <= float(table.abs().max()) * sc
    # --- conditions on the sums ---
    bound = float(table.abs().max()) * sc * float(wgt.abs().sum((1, 2, 3)).max())
    if worst_case:
        assert bound < limit, (bound, limit)
    else:
        assert verify, "this case is too deep for the worst-case bound: it needs verify=True"
    want = osalsa.fused_conv(srcs, wgt, b_, pad, dil, slope, bn_a, bn_b, res)
    case = SimpleNamespace(srcs=srcs, wgt=wgt, bias=b_, bn_a=bn_a, bn_b=bn_b, res=res, slope=slope, k=k, dil=dil, pad=pad, want=want,
                           worst_case=worst_case, bound=bound, absconv=None)
    if verify:
        case.absconv = float(F.conv2d(xin.abs().double(), wgt.abs().double(), None, padding=pad, dilation=dil).max())
        assert case.absconv < limit, (case.absconv, limit)
        c = lambda t: t.double()[None, :, None, None]
        v = F.conv2d(xin.double(), wgt.double(), None, padding=pad, dilation=dil)
        assert _exact32(v)
        if bias:
            v = v + c(b_)
            assert _exact32(v)
        if act:
            v = torch.where(v > 0, v, v * SLOPE)
            assert _exact32(v)
        if bn:
            v = v * c(bn_a)
            assert _exact32(v)
            v = v + c(bn_b)
            assert _exact32(v)
        if resid:
            v = v + res.double()
            assert _exact32(v)
        want64 = fused_conv64(srcs, wgt, b_, pad, dil, slope, bn_a, bn_b, res)
        assert torch.equal(v, want64)
        assert torch.equal(want.double(), want64), "the fp32 CPU conv is not exact on this lattice"
        assert torch.equal(fused_conv_split(srcs, wgt, b_, pad, dil, slope, bn_a, bn_b, res), want64), "the split is not exact on this lattice"
    return case


FAMILIES = [(1, 1, 0), (3, 1, 1), (3, 2, 2), (2, 2, 1)]


def small_cases():
    """The small shapes of test_gpu_conv.py / test_gpu_f16x3.py: (id, kwargs of lattice_case without orient / verify)."""
    out = []

    def add(name, n, parts, cout, h, w, fam, seed, **opts):
        out.append((f"{name}|k{fam[0]}d{fam[1]}|{'+'.join(map(str, parts))}->{cout}|N{n}|{h}x{w}",
                    dict(n=n, cin_parts=parts, cout=cout, h=h, w=w, fam=fam, seed=seed, **opts)))

    for fam in FAMILIES:
        for cout, hw in [(32, (16, 128)), (64, (8, 64)), (128, (8, 64)), (256, (4, 64)), (20, (16, 64))]:
            add("tile", 2, [32], cout, hw[0], hw[1], fam, cout + fam[0] * 7 + fam[1])
        # Cin % 16 != 0, W % 4 != 0, Cout % 32 != 0; with and without bias / BN / activation / residual
        add("ragged", 1, [5], 32, 13, 70, fam, 3)
        add("ragged-plain", 1, [5], 32, 13, 70, fam, 23, bias=False, bn=False, act=False, resid=False)
        add("ragged", 3, [21], 40, 5, 33, fam, 4, bn=False, resid=False)
        add("ragged-full", 3, [21], 40, 5, 33, fam, 24)
        add("ragged", 1, [7], 70, 9, 129, fam, 5, act=False)
        add("ragged-nobias", 1, [7], 70, 9, 129, fam, 25, bias=False)
    add("concat", 2, [32, 16, 48], 32, 8, 64, (3, 1, 1), 11, scales=True)
    add("concat", 2, [64, 64, 64], 64, 8, 64, (1, 1, 0), 10, scales=True)
    add("concat-plain", 2, [64, 64, 64], 64, 8, 64, (1, 1, 0), 9)            # the streaming 1x1 kernel with three sources
    add("shuffle", 2, [256, 256], 128, 8, 64, (3, 1, 1), 12, scales=True, ps_first=True)
    add("shuffle", 2, [64, 64], 32, 8, 64, (3, 1, 1), 13, scales=True, ps_first=True)
    add("tiled-1x1", 1, [32], 64, 5, 12, (1, 1, 0), 14)                      # H W % 32 != 0: the tiled kernel takes this 1x1
    return out


def table_case_kwargs(case):
    """A row (name, fam, parts, cout, n, h, w, opts) of test_gpu_dispatch_coverage's FP32_CASES / F16X3_CASES as lattice_case kwargs
    (the seed is the table tests' own; `stats` is the runner's business, not the generator's)."""
    _, fam, parts, cout, n, h, w, opts = case
    opts = {k: v for k, v in opts.items() if k != "stats"}
    return dict(n=n, cin_parts=parts, cout=cout, h=h, w=w, fam=fam, seed=cout + n + h + sum(parts), **opts)
