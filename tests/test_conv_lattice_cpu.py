"""CPU: the lattice generator (conv_lattice_cases.py) keeps its conditions on every case test_gpu_conv_lattice.py runs, and the
lattice cases have teeth: the restated split differs from the exact answer as soon as any piece of a `lo` image is lost.

lattice_case(verify=True) asserts the conditions itself (operands split exactly into normal fp16 parts, the other operand has no lo,
every partial sum and epilogue intermediate is an exact fp32, fp64 == fp32 CPU conv == fused_conv_split bit for bit)."""
import pytest
import torch

from conv_lattice_cases import lattice_case, small_cases, table_case_kwargs
from f16x3_restatement import fused_conv_split
from f16x3_split_cases import lost_lo_variants
from test_gpu_dispatch_coverage import F16X3_CASES, FP32_CASES, _id

SMALL = small_cases()


@pytest.mark.parametrize("orient", ["x", "w"])
@pytest.mark.parametrize("kw", [c[1] for c in SMALL], ids=[c[0] for c in SMALL])
def test_small_case_keeps_the_conditions_and_has_teeth(kw, orient):
    c = lattice_case(orient=orient, verify=True, **kw)
    args = (c.srcs, c.wgt, c.bias, c.pad, c.dil, c.slope, c.bn_a, c.bn_b, c.res)
    variants = {n: a for n, (op, a) in lost_lo_variants(kw, c.wgt.shape[1], c.k).items() if op == orient}
    assert len(variants) >= 2
    for name, a in variants.items():
        diff = float((fused_conv_split(*args, **a) - c.want.double()).abs().max())
        assert diff > 0, f"{name}: not seen by this case"
    # the other operand has no lo: leaving its term out changes nothing (the dropped lo*lo term is exactly zero for the same reason)
    other = ("hh", "lh") if orient == "x" else ("hh", "hl")
    assert torch.equal(fused_conv_split(*args, terms=other), c.want.double())


@pytest.mark.parametrize("orient", ["x", "w"])
@pytest.mark.parametrize("row", FP32_CASES + F16X3_CASES, ids=_id)
def test_table_row_keeps_the_conditions(row, orient):
    """The full-size rows at N = 1 and at most 8 image rows: the weights, K and every option are the row's own (the generator draws the
    weights from the seed alone), and the worst-case bound max|x| * max_co sum|w| it asserts does not depend on N, H or W -- it is what
    lets test_gpu_conv_lattice.py build these rows at full size with verify=False."""
    kw = table_case_kwargs(row)
    kw["n"], kw["h"] = 1, min(kw["h"], 8)
    c = lattice_case(orient=orient, verify=True, **kw)
    assert c.worst_case
    full = lattice_case(orient=orient, verify=True, **dict(kw, n=2, h=4, w=8))      # another size: the same weights
    assert torch.equal(full.wgt, c.wgt) and all(torch.equal(a, b) for a, b in ((full.bias, c.bias), (full.bn_a, c.bn_a)) if a is not None)


def test_generator_refuses_a_deep_case_without_verification():
    kw = dict(n=1, cin_parts=[256, 256], cout=128, h=8, w=64, fam=(3, 1, 1), seed=12, scales=True, ps_first=True)
    with pytest.raises(AssertionError):
        lattice_case(orient="w", verify=False, **kw)
