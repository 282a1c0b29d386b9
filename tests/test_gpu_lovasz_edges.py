"""GPU: the radix sort of csrc/radix_sort.hip, the Jaccard scan and gradient of csrc/lovasz.hip at the sizes where their tail logic works -- more than
one 2048-key tile with a partial last tile, 2 to 32 classes, absent classes between present ones -- and on inputs with ties
(saturated probabilities: errors exactly 0 and exactly 1); then the stability of the shared sort through the AUROC entry point.

Reference (`_reference`): err = |1[y==c] - p_c| as ONE fp32 subtraction, the kernel's own definition and exactly rounded on both
sides, so the tie groups are identical; everything after it in fp64.

Value bar 1e-6 absolute, derived: by Abel summation sum_k err_(k) (J_k - J_{k-1}) = sum_k J_k (err_(k) - err_(k+1)), so the fp32
rounding of J_k (one division, one subtraction: <= 1.5 ulp of 1 = 9e-8) moves the loss by at most max|dJ| * err_(1) <= 9e-8; the
fp32 products err * step add <= 6e-8 * loss, the final cast 6e-8.  `oracle.losses.lovasz_softmax` on the same probabilities in
fp64 forms err in fp64, up to 3e-8 from the fp32 one; the loss is 1-Lipschitz in err (non-negative steps that sum to J_n <= 1),
so the two references are within 1e-7 of each other and the kernel within 1e-6 of both.

Gradient, valid with or without ties: with g_err = n_summed * grad_p * (fg ? -1 : +1), the sum of g_err over a group of equal
fp32 err > 0 equals J(after the group) - J(before the group) of the fp64 reference within 1e-6 (consecutive steps telescope, only
the two end values are rounded); every g_err >= -2.5e-7 (the steps are non-negative; two fp32 roundings); exactly 0.0 at ignored
pixels, at err == 0 and in classes that are not summed.  Groups of one are the element-wise check."""
import numpy as np
import pytest
import torch

from oracle import losses as olosses
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.losses.lovasz import LovaszSoftmaxStable

pytestmark = pytest.mark.gpu

VALUE_BAR = 1e-6
GROUP_BAR = 1e-6
NEG_BAR = 2.5e-7
TILE = 2048


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _absent(c):
    """class 1, the last class and two adjacent middle classes (as far as c classes leave something present)"""
    if c <= 2:
        return set()
    if c <= 5:
        return {1, c - 1}
    return {1, c // 2, c // 2 + 1, c - 1}


def _labels(shape, c, ignore, gen):
    b, h, w = shape
    present = torch.tensor(sorted(set(range(c)) - _absent(c)))
    lab = present[torch.randint(0, len(present), (b, h, w), generator=gen)]
    if ignore is not None:
        lab[torch.rand(b, h, w, generator=gen) < 0.1] = ignore
    return lab


def _probs(kind, shape, c, lab, gen):
    b, h, w = shape
    if kind == "random":                      # (i) softmax outputs, ties only by chance
        return torch.softmax(torch.randn(b, c, h, w, generator=gen) * 2.0, 1)
    if kind == "grid":                        # (ii) multiples of 1/16: heavy ties, err exactly 0 and exactly 1 included
        wgt = torch.softmax(torch.randn(b * h * w, c, generator=gen) * 3.0, 1)
        draws = torch.multinomial(wgt, 16, replacement=True, generator=gen)
        counts = torch.zeros(b * h * w, c).scatter_add_(1, draws, torch.ones(b * h * w, 16))
        return (counts / 16.0).reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous()
    if kind == "onehot":                      # (iii) every err in {0, 1}; 40 % of the one-hots are on a random (mostly wrong) class
        hot = torch.where(torch.rand(b, h, w, generator=gen) < 0.6, lab.clamp(0, c - 1), torch.randint(0, c, (b, h, w), generator=gen))
        return torch.nn.functional.one_hot(hot, c).permute(0, 3, 1, 2).float().contiguous()
    if kind == "radix":                       # (iv) background errors 2^-e (1 + j/8) over 120 binades: all four key bytes vary; normal floats only
        e = torch.randint(0, 121, (b, c, h, w), generator=gen)
        j = torch.randint(0, 8, (b, c, h, w), generator=gen)
        e = torch.where((j > 0) & (e == 0), torch.ones_like(e), e)        # keep p <= 1
        p = torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double()) * (1.0 + j.double() / 8.0)
        p = p.float()                                                     # exact: 4 significant bits
        fg = torch.nn.functional.one_hot(lab.clamp(0, c - 1), c).permute(0, 3, 1, 2).bool() & (lab < c).unsqueeze(1)
        return torch.where(fg, torch.rand(b, c, h, w, generator=gen), p).contiguous()
    raise ValueError(kind)


def _class_list(c):
    return [1, min(3, c - 2), c - 1] if c > 3 else [1]        # an absent class (1), a present one, the last (absent) class


# ---- fp64 reference -----------------------------------------------------------------------------------------------------------
def _reference(probs, lab, ignore, classes):
    """-> (loss float, summed class ids, {c: dict(valid, err, fg, order, J, ends)}) ; probs fp32 [B,C,H,W] on the CPU."""
    c = probs.shape[1]
    y = lab.reshape(-1).numpy()
    valid = np.ones_like(y, dtype=bool) if ignore is None else y != ignore
    p32 = probs.permute(1, 0, 2, 3).reshape(c, -1).numpy().astype(np.float32)
    if classes == "present":
        summed = [k for k in range(c) if np.any(valid & (y == k))]
    else:
        summed = list(range(c)) if classes == "all" else list(classes)
    per, total = {}, 0.0
    for k in summed:
        fg = (y == k) & valid
        err32 = np.abs(fg.astype(np.float32) - p32[k])                  # one fp32 subtraction: the kernel's definition
        assert err32.dtype == np.float32
        e = err32[valid].astype(np.float64)
        f = fg[valid].astype(np.float64)
        order = np.argsort(-e, kind="stable")
        es, fs = e[order], f[order]
        n = es.size
        if n == 0:
            per[k] = dict(err32=err32, fg=fg, n=0)
            continue
        g = fs.sum()
        cum = np.cumsum(fs)
        jac = 1.0 - (g - cum) / (g + np.arange(1, n + 1) - cum)
        total += float(np.sum(es * np.diff(np.concatenate(([0.0], jac)))))
        ends = np.flatnonzero(np.concatenate((es[1:] != es[:-1], [True])))
        per[k] = dict(err32=err32, fg=fg, n=n, order=order, es=es, jac=jac, ends=ends)
    return (total / len(summed) if summed else 0.0), summed, per


def _check_gradient(grad, lab, ignore, summed, per, figures):
    """grad: fp32 [B,C,H,W] on the CPU."""
    c = grad.shape[1]
    y = lab.reshape(-1).numpy()
    valid = np.ones_like(y, dtype=bool) if ignore is None else y != ignore
    g = grad.permute(1, 0, 2, 3).reshape(c, -1).numpy()
    for k in range(c):
        if k not in summed:
            assert not g[k].any(), f"class {k} is not summed but has a gradient"
    for k in summed:
        r = per[k]
        assert not g[k][~valid].any(), f"class {k}: gradient at an ignored pixel"
        assert not g[k][r["err32"] == 0.0].any(), f"class {k}: gradient at err == 0"
        if r["n"] == 0:
            continue
        gerr = len(summed) * g[k].astype(np.float64) * np.where(r["fg"], -1.0, 1.0)
        figures["neg"] = min(figures["neg"], float(gerr.min()))
        assert gerr.min() >= -NEG_BAR, f"class {k}: negative Jaccard step {gerr.min():.3e}"
        gs = gerr[valid][r["order"]]
        ends = r["ends"]
        starts = np.concatenate(([0], ends[:-1] + 1))
        gsum = np.add.reduceat(gs, starts)
        jend = r["jac"][ends]
        want = jend - np.concatenate(([0.0], jend[:-1]))
        pos = r["es"][ends] > 0.0
        if pos.any():
            d = float(np.abs(gsum - want)[pos].max())
            figures["group"] = max(figures["group"], d)
            assert d <= GROUP_BAR, f"class {k}: tie-group sum off by {d:.3e}"


def _run(cuda, probs, lab, ignore, classes):
    """value and gradient of the gradient path, the value of the no-gradient path"""
    mod = LovaszSoftmaxStable(ignore, classes)
    pd = probs.to(cuda).requires_grad_(True)
    loss = mod(pd, lab.to(cuda), "probs")
    loss.backward()
    with torch.no_grad():
        plain = mod(probs.to(cuda), lab.to(cuda), "probs")
    return float(loss.detach()), pd.grad.cpu(), float(plain)


def _check_case(cuda, probs, lab, ignore, classes, tag):
    want, summed, per = _reference(probs, lab, ignore, classes)
    oracle = float(olosses.lovasz_softmax(probs.double(), lab, ignore, classes))
    assert abs(oracle - want) <= 1e-7, (tag, oracle, want)                # the two fp64 references (docstring)
    got, grad, plain = _run(cuda, probs, lab, ignore, classes)
    figures = {"group": 0.0, "neg": 0.0}
    try:
        assert abs(got - want) <= VALUE_BAR and abs(got - oracle) <= VALUE_BAR, (tag, got, want, oracle)
        assert plain == got, (tag, plain, got)                            # the no-gradient path runs the same kernels
        _check_gradient(grad, lab, ignore, summed, per, figures)
    finally:
        print(f"{tag}: |value - fp64| = {abs(got - want):.3e}, max tie-group |sum - dJ| = {figures['group']:.3e}, min g_err = {figures['neg']:.3e}")
    return got, grad


# shapes by N = B*H*W: 2047 one tile less a key | 2048 one full tile | 2049 one key in a second tile | 2050 b = i / HW with odd HW |
# 2561 a tile, one wave slice and 1 | 6153 = 3*2048 + 9 several tiles, short tail | 8205 several tiles, odd B and HW
CASES = [
    ((1, 1, 2047), 2, None, "present", "random"),
    ((1, 1, 2047), 21, 0, "all", "grid"),
    ((1, 1, 2048), 5, 0, "all", "grid"),
    ((1, 1, 2048), 32, 255, "present", "radix"),
    ((1, 1, 2049), 20, 255, "present", "onehot"),
    ((1, 1, 2049), 32, 0, "present", "grid"),
    ((1, 1, 2049), 2, None, "present", "random"),
    ((1, 1, 2049), 21, 0, "all", "radix"),
    ((2, 5, 205), 21, 0, "list", "grid"),
    ((2, 5, 205), 5, None, "present", "random"),
    ((1, 1, 2561), 32, 255, "all", "radix"),
    ((1, 1, 2561), 20, 0, "list", "onehot"),
    ((3, 7, 293), 21, 0, "present", "grid"),
    ((3, 7, 293), 32, None, "list", "random"),
    ((3, 7, 293), 2, 255, "all", "grid"),
    ((5, 3, 547), 32, 255, "present", "onehot"),
    ((5, 3, 547), 5, 0, "all", "radix"),
    ((5, 3, 547), 20, 0, "present", "random"),
    ((5, 3, 547), 21, 255, "list", "grid"),
]


@pytest.mark.parametrize("shape,c,ignore,classes,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_value_and_tie_group_gradient(cuda, shape, c, ignore, classes, kind):
    gen = torch.Generator().manual_seed(1000 * c + shape[2])
    lab = _labels(shape, c, ignore, gen)
    probs = _probs(kind, shape, c, lab, gen)
    cls = _class_list(c) if classes == "list" else classes
    _, grad = _check_case(cuda, probs, lab, ignore, cls, f"{shape} C={c} ign={ignore} {classes} {kind}")
    # reproducible run to run: the sort is stable and every step is a function of its sorted position
    pd = probs.to(cuda).requires_grad_(True)
    LovaszSoftmaxStable(ignore, cls)(pd, lab.to(cuda), "probs").backward()
    assert torch.equal(pd.grad.cpu(), grad)


def test_single_valid_pixel_in_the_second_tile(cuda):
    gen = torch.Generator().manual_seed(5)
    lab = torch.full((1, 1, 2049), 255, dtype=torch.int64)
    lab[0, 0, 2048] = 3
    probs = _probs("grid", (1, 1, 2049), 5, lab, gen)
    probs[0, :, 0, 2048] = torch.tensor([0.25, 0.0, 0.125, 0.5, 0.125])
    for classes in ("present", "all", [1, 3, 4]):
        got, grad = _check_case(cuda, probs, lab, 255, classes, f"single valid pixel {classes}")
    want = (0.0 + 0.5 + 0.125) / 3                 # classes 1, 3, 4 at that pixel: err 0, 1 - 0.5, 0.125, each with a Jaccard step of 1
    assert abs(got - want) <= VALUE_BAR


@pytest.mark.parametrize("kind", ["grid", "random"])
@pytest.mark.parametrize("classes", ["present", "all"])
def test_last_tile_entirely_ignored(cuda, classes, kind):
    shape, c = (3, 7, 293), 5                       # 6153 pixels: the last tile holds pixels 6144 .. 6152
    gen = torch.Generator().manual_seed(11)
    lab = _labels(shape, c, 255, gen)
    lab.reshape(-1)[3 * TILE:] = 255
    probs = _probs(kind, shape, c, lab, gen)
    _check_case(cuda, probs, lab, 255, classes, f"last tile ignored {classes} {kind}")


def test_every_pixel_ignored_and_nothing_summed(cuda):
    shape, c = (1, 1, 2049), 5
    gen = torch.Generator().manual_seed(12)
    lab = torch.zeros(shape, dtype=torch.int64)
    probs = _probs("random", shape, c, lab, gen)
    for classes in ("present", "all"):
        got, grad = _check_case(cuda, probs, lab, 0, classes, f"all ignored {classes}")
        assert got == 0.0 and not grad.any()


def test_size_change_between_calls(cuda):
    """The workspace is carved from a fresh allocation on every call, and the caching allocator hands back blocks that hold the
    previous call's keys, histograms and tile prefixes: a large call, a small one, the large one again -- each must equal a call
    made right after the cache was emptied."""
    gen = torch.Generator().manual_seed(21)
    big_lab = _labels((5, 3, 547), 32, 0, gen)
    big = _probs("random", (5, 3, 547), 32, big_lab, gen)          # no zero errors: every sorted position of every tile counts
    small_lab = _labels((1, 1, 2049), 5, 0, gen)
    small = _probs("random", (1, 1, 2049), 5, small_lab, gen)
    torch.cuda.empty_cache()
    fresh = {}
    for name, (p, y) in (("big", (big, big_lab)), ("small", (small, small_lab))):
        fresh[name] = _check_case(cuda, p, y, 0, "present", f"fresh {name}")
        torch.cuda.empty_cache()
    for name, (p, y) in (("big", (big, big_lab)), ("small", (small, small_lab)), ("big", (big, big_lab))):
        got, grad, plain = _run(cuda, p, y, 0, "present")
        assert got == fresh[name][0] and plain == got and torch.equal(grad, fresh[name][1]), name


# ---- the shared sort: stability ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 6221])
def test_shared_sort_is_stable_and_auroc_is_the_integer_formula(cuda, n):
    """7 distinct finite scores of both signs, +inf and -inf (no -0.0: its key differs from +0.0's): every tile holds long runs of
    equal keys, so the order inside a run shows whether each LSD pass kept the order of the pass before across lanes, waves and
    tiles.  The sorted output must be the input in the order of a stable descending sort, and the AUROC the header's formula,
    sum over negatives of (#positives ranked before) / (P N), in integers on that order."""
    gen = torch.Generator().manual_seed(n)
    values = torch.tensor([-3.5, -1.0, -1e-30, 0.0, 2e-20, 0.75, 1e10, float("inf"), float("-inf")])
    scores = values[torch.randint(0, len(values), (n,), generator=gen)]
    err = (torch.rand(n, generator=gen) < 0.4).to(torch.uint8)
    if n > 1:
        err[0], err[1] = 1, 0
    a, pos, neg, ss, se = ops.auroc_from_samples(scores.to(cuda), err.to(cuda), want_sorted=True)
    order = torch.sort(scores, descending=True, stable=True).indices
    assert torch.equal(ss.cpu(), scores[order]) and torch.equal(se.cpu(), err[order])
    flags = err[order].to(torch.int64)
    p_want = int(flags.sum())
    assert pos == p_want and neg == n - p_want
    if p_want == 0 or p_want == n:
        assert np.isnan(a)
    else:
        before = torch.cumsum(flags, 0)                                    # at a negative: the positives ranked before it
        total = int(before[flags == 0].sum())
        assert abs(a - total / (p_want * (n - p_want))) <= 1e-12
