"""The edge-shape cases of tests/pixel_edge_cases.py are fair before a GPU sees them: every case's reference runs here in fp64 and in
fp32, and for every result that is not exact the fp32 torch evaluation lies within a quarter of the bar of the fp64 one (a condition
on the inputs, not a measurement of a kernel).  The two GroupNorm offset inputs are the exception: their bar is four times that gap, and
it is computed and printed here (profiles/r24/README.md records the figures)."""
import pytest
import torch
import torch.nn.functional as F

import pixel_edge_cases as pe


@pytest.mark.parametrize("case", pe.ALL_CASES, ids=pe.case_id)
def test_conditioning(case):
    inputs, want64, want32 = pe.evaluate(case)
    for t in inputs.values():
        if torch.is_tensor(t):
            assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert set(want64) == set(want32)
    if "round2" in case.id:          # slu_grid_1d caps the grid of 256-thread workgroups: more elements than that, or no thread takes a second one
        cap = pe.GRID_CAP[case.family]
        assert next(iter(want64.values())).numel() > cap * 256, f"{case.id}: no second round of a {cap} x 256 grid"
    for key, gap, bar, spec in pe.conditioning(case, want64, want32):
        print(f"{case.id} {key}: fp32 torch-fp64 {gap:.3e}, bar {bar:.3e}")
        if spec[1] == "gap4":
            assert bar == 4.0 * gap and bar > 20 * 2e-5, "the offset inputs are meant to be out of fp32 torch's reach"
        elif spec[2:] != ("unconditioned",):
            assert gap <= bar / 4, f"{case.id} {key}: fp32 torch is {gap:.3e} from fp64, more than a quarter of the bar {bar:.3e}"


def test_case_tables_hold_what_they_promise():
    ids = {c.id for c in pe.ALL_CASES}
    by = {name: fam.cases for name, fam in pe.FAMILIES.items()}
    assert sum(c.big for c in pe.ALL_CASES) == 12          # one second-round case per walk form, and the two pool shapes that fall short of it
    assert {c.family for c in pe.ALL_CASES if "round2" in c.id} == set(pe.GRID_CAP)
    assert {c.p["shape"][3] for c in by["rowsoftmax"]} >= set(pe.ROW_W) and "row_softmax_mul wide 3x1x1x65" in ids
    counts = {(c.p["shape"][3] * (6 // c.p["groups"]), c.p["groups"]) for c in by["groupnorm"] if "stats" in c.id}
    assert {n for n, _ in counts} >= set(pe.COUNTS) and {g for _, g in counts} == {6, 3, 1}
    assert {c.p["shape"][3] for c in by["gate"] if not c.big} == set(pe.COUNTS)
    assert (pe.SE_MAX[0] + pe.SE_MAX[1]) * 4 == 64 * 1024
    assert len(pe.FIXED) == 22 and all(v in pe.FIXED for v in (0.0, 88.5, -89.0, 1e4, -1e-30))


def test_relu_const_group_is_exactly_zero_in_the_reference():
    """the ReLU'd constant group: y == 0 exactly in both dtypes, so `y > 0` masks the same elements everywhere"""
    case = next(c for c in pe.FAMILIES["groupnorm"].cases if "const relu zeros" in c.id)
    _, want64, want32 = pe.evaluate(case)
    assert bool((want64["y"][:, :2] == 0).all()) and bool((want32["y"][:, :2] == 0).all())
    assert bool((want64["dx"][:, :2] == 0).all())
    assert float(want64["rstd"][0]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)


def test_maxpool_tie_cases_have_ties():
    for case in pe.FAMILIES["maxpool"].cases:
        if case.p["kind"] == "ties" and case.p["shape"][2] * case.p["shape"][3] >= 9:
            x = pe.FAMILIES["maxpool"].build(case)["x"]
            y = F.max_pool2d(x, 3, 2, 1)
            hits = F.unfold(F.pad(x, (1, 1, 1, 1), value=-1.0), 3, stride=2).view(x.shape[0], x.shape[1], 9, -1) == y.flatten(2)[:, :, None]
            assert int((hits.sum(2) > 1).sum()) > 0, case.id


def test_activation_list_finite_and_silu_formulas():
    """Every reference output and gradient on the fixed list is finite; the kernel's fp32 SiLU formulas stay within 5e-8 of fp64 on it;
    at x = 0 the gradient is ATen's: 0 for ReLU, the slope for leaky, 1 for ELU + 1."""
    x = torch.tensor(pe.FIXED)
    for name in pe.POINTWISE:
        for dt in (torch.float64, torch.float32):
            xl = x.clone().to(dt).requires_grad_(True)
            y = pe.pointwise_fn(name, xl)
            (g,) = torch.autograd.grad(y, xl, torch.ones_like(y))
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(g).all()), name
            if name in pe.GRAD_AT_ZERO:
                assert float(g[0]) == float(g[1]) == float(torch.tensor(pe.GRAD_AT_ZERO[name], dtype=dt)), name
    xl = x.double().requires_grad_(True)
    y64 = F.silu(xl)
    (g64,) = torch.autograd.grad(y64, xl, torch.ones_like(y64))
    y32, g32 = pe.silu_as_kernel(x)
    assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(g32).all())
    fwd, bwd = float((y32.double() - y64.detach()).abs().max()), float((g32.double() - g64).abs().max())
    print(f"SiLU as the kernel computes it, fp32 on the fixed list: forward {fwd:.3e}, derivative {bwd:.3e} from fp64")
    assert fwd <= 5e-8 and bwd <= 5e-8
