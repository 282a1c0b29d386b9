"""The value-branch cases of tests/dirichlet_value_cases.py are fair before a GPU sees them.  For every case, here, without a GPU:
the reference runs in fp64 and in fp32 on the same fp32 inputs; every branch predicate of the kernels (the eps clamps, pred, pred != y,
the hard-margin comparison, h > 0, the softplus side, the argmax, p against eps, the number of recurrence steps) has the same truth value
in both evaluations on every counted pixel, so no input sits on an edge that rounding decides; where the bar is the coefficient alone the
fp32 oracle lies within a quarter of it on every pixel; the gradient entries that are 0 by construction are exactly 0 in both.  The
branch census then shows that every outcome of every named branch has a pixel in each case that is there for it, and the gap-bound list
holds nothing that does not need it.  Each test prints its figures (profiles/r25/README.md records the gap-bound ones)."""
import functools

import pytest
import torch

import dirichlet_value_cases as dv


@functools.lru_cache(maxsize=None)
def _evaluated(case_id):
    return dv.evaluate(next(c for c in dv.ALL_CASES if c.id == case_id))


@pytest.mark.parametrize("case", dv.ALL_CASES, ids=dv.case_id)
def test_case_is_fair(case):
    inputs, want64, want32 = _evaluated(case.id)
    for t in inputs.values():
        assert not bool(torch.isnan(t).any())
        if t.is_floating_point():
            assert t.dtype == torch.float32 and t.is_contiguous()
            assert bool(torch.isfinite(t).all()) or case.p.get("kind") == "neg-inf class"
    if case.p.get("kind") == "neg-inf class":          # one class per column, never the whole column
        x = inputs["logits"]
        assert bool((torch.isinf(x).sum(-3) == 1).all()) and bool((x[torch.isinf(x)] < 0).all())
    assert set(want64) == set(want32)
    # same decisions in fp32 and fp64
    d64, d32 = dv.DECISIONS[case.family](case, inputs, torch.float64), dv.DECISIONS[case.family](case, inputs, torch.float32)
    for name in d64:
        differ = int((d64[name] != d32[name]).sum())
        print(f"{case.id} decision '{name}': {tuple(d64[name].shape)} agree" if not differ else f"{case.id} decision '{name}': {differ} DIFFER")
        assert not differ, f"{case.id}: '{name}' differs between the fp32 and the fp64 evaluation in {differ} places: the input needs another constant"
    # conditioning
    for key, frac, gap, bar, gap_bound in dv.conditioning(case, want64, want32):
        print(f"{case.id} {key}: fp32 oracle-fp64 {gap:.3e}, at worst {frac:.3g} of the coefficient's bar ({bar:.3e} there){' (gap-bound: bar >= 4 x the gap)' if gap_bound else ''}")
        if not gap_bound:
            assert frac <= 0.25, f"{case.id} {key}: the fp32 oracle is {frac:.3g} of the bar from fp64, more than a quarter: another seed or scale, or the gap-bound list"
    # exact zeros
    if case.family == "loss":
        mask = dv.zero_gradient_mask(case, inputs)
        assert bool((want64["grad"][mask] == 0).all()) and bool((want32["grad"][mask] == 0).all()), f"{case.id}: a gradient that is 0 by construction is not"
        print(f"{case.id}: {int(mask.sum())} of {mask.numel()} gradient entries are 0 by construction")


@pytest.mark.parametrize("entry", dv.CENSUS, ids=lambda e: f"{e[0]}-{e[1]}-{e[2]}".replace(" ", "-"))
def test_branch_census(entry):
    family, branch, outcome = entry[:3]
    cases = dv.census_cases(entry)
    assert cases, f"no case is listed for {branch} = {outcome}"
    for case in cases:
        inputs = _evaluated(case.id)[0]
        d = dv.DECISIONS[family](case, inputs, torch.float64)[branch]
        n = int((d == outcome).sum())
        print(f"{branch} = {outcome}: {n} of {d.numel()} in {case.id}")
        assert n > 0, f"{case.id}: no pixel takes {branch} = {outcome}"


def test_gap_bound_list_holds_only_what_needs_it():
    """every (loss kind, regime, result) of GAP_BOUND has a case whose fp32 oracle is further than a quarter of the coefficient's bar from fp64,
    and only the regimes named for it are listed"""
    assert {r for _, r in dv.GAP_BOUND} == {"large-evidence", "evidence-free", "confident-right", "saturated"}
    worst = {}
    for case in dv.FAMILIES["loss"].cases:
        kind = dv.LOSSES[case.p["loss"]].kind
        if (kind, case.p["regime"]) in dv.GAP_BOUND:
            _, want64, want32 = _evaluated(case.id)
            for key, frac, gap, _, gap_bound in dv.conditioning(case, want64, want32):
                if gap_bound:
                    k = (kind, case.p["regime"], key)
                    worst[k] = max(worst.get(k, (0.0, 0.0)), (frac, gap))
    for (kind, regime), (results, _) in dv.GAP_BOUND.items():
        for key in results:
            frac, gap = worst[(kind, regime, key)]
            print(f"gap-bound {kind} {regime} {key}: fp32 oracle-fp64 up to {gap:.3e}, {frac:.3g} of the coefficient's bar")
            assert frac > 0.25, f"{kind} {regime} {key} does not need the gap bound"


def test_case_tables_hold_what_they_promise():
    by = {}
    for c in dv.FAMILIES["loss"].cases:
        by.setdefault((c.p["loss"], c.p["regime"]), []).append(c)
    for regime, (names, _) in dv.REGIMES.items():
        for name in names:
            cs = by[(name, regime)]
            assert {c.p["c"] for c in cs} == ({3, 20, 32} if name in dv.FROM_THREE else {20, 32}), (name, regime)
    assert len(dv.LOSSES) == 13 and set(dv.SCALES) <= set(dv.SALTS) | {c.id for c in dv.ALL_CASES}
    assert set(dv.SALTS) <= {c.id for c in dv.ALL_CASES} and set(dv.SCALES) <= {c.id for c in dv.ALL_CASES}
    for c in dv.FAMILIES["loss"].cases:
        inputs = _evaluated(c.id)[0]
        a, lab = inputs["alpha"], inputs["labels"]
        assert tuple(a.shape) == (c.p["shape"][0], c.p["c"]) + c.p["shape"][1:] and bool((lab >= 0).all()) and bool((lab < c.p["c"]).all())
        loss = dv.LOSSES[c.p["loss"]]
        rows, y, counted = dv.counted_rows(inputs, loss)
        if lab.numel() > 1 and loss.ignore == 0:
            assert 0.03 <= float((lab == 0).float().mean()) <= 0.2, c.id          # about 10 % carry the ignore value
        elif lab.numel() == 1:
            assert int(counted.sum()) == 1
        ay = rows.gather(1, y[:, None])
        if c.p["regime"] in ("clamped", "clamped-tiny"):
            assert bool((ay >= 1.0).all()) and bool(((rows < 1e-8).sum(1) == min(4, c.p["c"] - 2)).all()), c.id
        if c.p["regime"] in ("tie-label-lower", "tie-label-higher"):
            top = rows.topk(2, dim=1)
            assert bool((top.values[:, 0] == top.values[:, 1]).all()) and bool((ay[:, 0] == top.values[:, 0]).all()), c.id
            first = rows.argmax(1)
            assert bool((first == y).all() if c.p["regime"] == "tie-label-lower" else (first < y).all()), c.id
        if c.p["regime"] == "margin-sides":
            p = rows.double() / rows.double().sum(1, keepdim=True)
            gap = p.max(1).values - p.gather(1, y[:, None])[:, 0]
            margin = loss.prm["margin"] or 0.05
            away = torch.minimum((gap - margin).abs(), torch.where(gap == 0, torch.full_like(gap, 1.0), gap.abs()))
            assert float(away.min()) > 0.009 and bool((gap > margin).any()) and bool(((gap < margin) & (gap > 0)).any()) and bool((gap == 0).any()), c.id
    for fam in ("mc", "single"):
        for c in dv.FAMILIES[fam].cases:
            if c.p["kind"] in ("swap", "top-two equal", "equal"):
                inputs, want64, _ = _evaluated(c.id)
                for dt in (torch.float64, torch.float32):
                    assert bool(dv.DECISIONS[fam](c, inputs, dt)["tie of the top two"].all()), c.id
                if c.p["kind"] == "equal":
                    assert not bool(want64["preds"].any()) and float((want64["H_norm"] - 1).abs().max()) < 1e-12
                if c.p["kind"] == "swap":
                    assert not bool(want64["preds"].any())
            if c.p["kind"] == "identical":
                assert float(_evaluated(c.id)[1]["MI"].max()) < 1e-12
    for c in dv.FAMILIES["head"].cases:
        if c.p["kind"] == "equal":
            assert not bool(_evaluated(c.id)[1]["preds"].any())
    scale = {float(v) for v in dv.SCALE_LOGITS}
    assert {19.999, 20.0, 20.001} <= scale and len(scale) == 9 and dv.TEMPERATURES == [0.5, 1.0, 4.0]
