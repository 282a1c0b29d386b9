"""The edge-shape cases of tests/h8_pixel_edge_cases.py are fair before a GPU sees them, and fine enough to tell a subtly wrong kernel
from a right one.  Fair: every case's reference runs here in fp64 and in fp32; the stored inputs are fp16-valued; for every result that is
not exact torch's fp32 evaluation, rounded to fp16 where the kernel stores fp16, lies within the bar with a quarter of its coefficient
term; no reference value is NaN or within the coefficient term of 65520.  Fine: for each family, wrong variants of the reference written
in torch (never a broken kernel) miss the bar of at least one case."""
import pytest
import torch
import torch.nn.functional as F

import h8_pixel_edge_cases as hp

SMALL = [c for c in hp.ALL_CASES if not c.big]


@pytest.mark.parametrize("case", hp.ALL_CASES, ids=hp.case_id)
def test_conditioning(case):
    inputs, want64, want32 = hp.evaluate(case)
    for name, t in inputs.items():
        if torch.is_tensor(t):
            assert t.dtype == torch.float32 and not bool(torch.isnan(t).any()), name
            if name in hp.STORED[case.family]:
                assert torch.equal(t, t.half().float()), f"{case.id}: stored input {name} is not fp16-valued"
    assert {k for k in want64 if "!" not in k} == set(want32) == set(hp.FAMILIES[case.family].bars(case))
    for key, share in hp.conditioning(case, want64, want32):
        print(f"{case.id} {key}: fp32 torch at {share:.3f} of its quarter bar")
    if case.family == "groupnorm":          # GN_COEF is four times torch's fp32 gap in operand units: no case is further than a quarter of it
        gap = (want32["y"].double() - want64["y"]).abs()
        fin = torch.isfinite(want32["y"].double()) & (want64["y!tol"] > 0)
        worst = float((gap[fin] / want64["y!tol"][fin]).max()) * hp.GN_COEF / hp.U if bool(fin.any()) else 0.0
        print(f"{case.id}: fp32 torch-fp64 in operand units {worst:.3f} * 2^-24, GN_COEF {hp.GN_COEF / hp.U:.2f} * 2^-24")
        # the worst case of the table sits at 3.245 of the 3.25 this allows: a new GroupNorm case or seed that measures more trips this assertion, and
        # then GN_COEF is measured again (four times the new gap, written next to it), it is not the case that gives way
        assert worst <= hp.GN_COEF / hp.U / 4


def _gn_parts(planes, hw):
    """gn_parts of csrc/fpn_opt_h8.hip"""
    return max(1, min(256, (hw + 1023) // 1024, (2048 + planes - 1) // planes))


def test_case_tables_hold_what_they_promise():
    by = {name: fam.cases for name, fam in hp.FAMILIES.items()}
    assert set(by) == {"maxpool", "avgpool", "s2d", "d2s", "elu", "bilinear", "groupnorm", "gate", "attention", "to_h8", "from_h8", "pixelshuffle"}
    assert len({c.id for c in hp.ALL_CASES}) == len(hp.ALL_CASES) and len({hp.case_id(c) for c in hp.ALL_CASES}) == len(hp.ALL_CASES)
    # --- the row walk: output sizes, tile edges, a second round of grid y and of grid z, pad channels
    for fam, rows_of in (("maxpool", lambda p: ((p["hw"][0] + 1) // 2, (p["hw"][1] + 1) // 2, p["n"])), ("avgpool", lambda p: ((p["hw"][0] + 1) // 2, (p["hw"][1] + 1) // 2, p["n"] * (3 if p["mode"] == "bcast" else 1))),
                         ("s2d", lambda p: p["out"] + (p["n"],)), ("d2s", lambda p: (p["s"] * p["hw"][0], p["s"] * p["hw"][1], p["n"])),
                         ("bilinear", lambda p: (p["s"] * p["hw"][0], p["s"] * p["hw"][1], p["n"])), ("elu", lambda p: p["hw"] + (p["n"],))):
        walked = [rows_of(c.p) for c in by[fam]]
        sizes = {w[:2] for w in walked}
        if fam in ("maxpool", "avgpool", "s2d", "elu"):
            assert sizes >= set(hp.OUT_HW) and {w[1] for w in walked} >= {255, 256, 257}, fam
        else:          # s-fold outputs: the listed sizes as inputs, 2x2 as an output, columns on both sides of a tile edge
            assert {c.p["hw"] for c in by[fam]} >= set(hp.OUT_HW) and (2, 2) in sizes and {w[1] for w in walked} >= {254, 256, 258}, fam
            assert {c.p["s"] for c in by[fam]} == {2, 4, 8}, fam
        assert sum(w[0] > hp.ROW_CAP + 1 and w[1] <= 8 for w in walked) == 1 and sum(w[2] > hp.ROW_CAP + 1 for w in walked) == 1, fam
        assert all(c.big == (w[0] > hp.ROW_CAP or w[2] > hp.ROW_CAP) for c, w in zip(by[fam], walked)), fam
    for fam in ("maxpool", "avgpool"):
        assert {(c.p["hw"][0] % 2, c.p["hw"][1] % 2) for c in by[fam]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {c.p["c"] for c in by[fam]} >= {5, 12, 20}
    assert {c.p["classes"] for c in by["elu"]} >= {1, 3, 5}
    assert {c.p["mode"] for c in by["avgpool"]} == {"plain", "scaled", "bcast"}
    meta = [c.p for c in by["s2d"] if c.p["m"]]
    assert {p["f"] for p in meta} == {1, 2, 4, 8} and {(p["c"], p["m"]) for p in meta} >= {(8, 1), (8, 8), (5, 5), (20, 6), (20, 20)}
    assert {p["phase00"] for p in meta} == {True, False} and any((p["c"] - p["m"]) // 8 != (p["c"] - 1) // 8 for p in meta)
    # --- GroupNorm: plane sizes, ragged parts, group widths at every slot, the tile cap
    gn = [c.p for c in by["groupnorm"]]
    assert {p["hw"][0] * p["hw"][1] for p in gn} >= {1, 4, 1023, 1024, 1025, 2049, 66563, 262147, 1048876}
    for p in gn:
        hw, planes = p["hw"][0] * p["hw"][1], p["n"] * ((p["c"] + 7) // 8)
        parts = _gn_parts(planes, hw)
        chunk = (hw + parts - 1) // parts
        if hw == 66563:
            assert parts == 66 and parts * chunk > hw > (parts - 1) * chunk
        if hw == 262147:
            assert parts == 256 and parts * chunk > hw > (parts - 1) * chunk
    slots = {(p["c"] // p["groups"], (k * (p["c"] // p["groups"])) % 8) for p in gn for k in range(p["groups"])}
    assert slots == {(1, k) for k in range(8)} | {(2, 0), (2, 2), (2, 4), (2, 6), (4, 0), (4, 4), (8, 0)}
    assert {p["c"] for p in gn} >= {8, 16, 20, 24} and {p["kind"] for p in gn} == set(hp.GN_KINDS)
    assert {(p["relu"], p["affine"]) for p in gn} == {(a, b) for a in (False, True) for b in (False, True)} and {p["dest"] for p in gn} == {"new", "slice", "inplace"}
    assert any((p["hw"][0] * p["hw"][1] + 255) // 256 > hp.TILE_CAP for p in gn)
    # --- gate
    gate = [c.p for c in by["gate"]]
    assert {p["hw"][0] * p["hw"][1] for p in gate} >= {1, 3, 4, 5, 1023, 1024, 1025, 4099, 1048876}
    assert {(p["hw"][0] * p["hw"][1]) % 4 for p in gate if p["n"] == 3} >= {0, 2} and {p["c"] for p in gate} >= {8, 256}
    assert {p["kind"] for p in gate} == set(hp.GATE_KINDS) | {"fixed"}
    shared = {(hp.gate_grid_y(p["n"], p["c"], p["hw"][0] * p["hw"][1]), (p["c"] + 7) // 8) for p in gate}      # (grid y, blocks)
    shared = {(y, g) for y, g in shared if y < g}
    assert any(g % y and y > 1 for y, g in shared) and any(y == 1 for y, g in shared) and len(shared) >= 3, shared
    # --- attention, layout
    att = [c.p for c in by["attention"]]
    assert {p["w"] for p in att} >= {1, 2, 255, 256, 257, 4096} and {p["c"] for p in att} >= {8, 64, 512} and {p["h"] for p in att} >= {1, 3}
    assert {p["spread"] for p in att} == {0, 3, 60} and {p["tkind"] for p in att} >= {"randn", "sat", "small"}
    for fam in ("to_h8", "from_h8"):
        assert {c.p["c"] for c in by[fam]} >= {1, 7, 8, 9, 20}
        assert sum(c.big for c in by[fam]) == 1 and all((c.p["hw"][0] * c.p["hw"][1] * c.p["n"] * ((c.p["c"] + 7) // 8) > hp.LIN_CAP * 256) == c.big for c in by[fam])
    assert {(c.p["kind"], c.p["scaled"]) for c in by["to_h8"]} >= {(k, s) for k in ("randn", "overflow", "subnormal") for s in (False, True)}
    assert {(c.p["gi"], c.p["mode"]) for c in by["pixelshuffle"]} >= {(g, m) for g in (1, 2, 4, 5) for m in hp.PS_MODES}


def test_special_values_reach_the_results():
    """the tables promise outputs in the fp16 subnormal range, outputs that round to 65504 and to infinity, and -inf / signed-zero pool inputs"""
    for fam in ("avgpool", "bilinear", "groupnorm", "gate", "attention", "to_h8", "pixelshuffle"):
        sub = top = over = 0
        for c in hp.FAMILIES[fam].cases:
            if c.big:
                continue
            inputs = hp.FAMILIES[fam].build(c)
            w = next(iter(v for k, v in hp.FAMILIES[fam].ref(c, inputs, torch.float64).items() if k in ("y", "out"))).abs()
            sub += int(((w > 0) & (w < 2.0 ** -14)).sum())
            top += int(((w >= 65488.0) & (w < 65520.0)).sum())
            over += int((w >= 65520.0).sum())
        print(f"{fam}: {sub} subnormal results, {top} that round to 65504, {over} that round to an infinity")
        assert sub > 0 and (over > 0 or fam in ("bilinear", "attention")), fam          # a convex combination, or a weight <= 1, cannot overflow
        if fam != "groupnorm":
            assert top > 0, fam
    for fam in ("maxpool", "avgpool"):
        xs = [hp.FAMILIES[fam].build(c)["x"] for c in hp.FAMILIES[fam].cases if c.p["kind"] == "edge" and not c.big]
        assert len(xs) >= 2 and all(bool((x == -hp.INF).any()) for x in xs) and any(bool(((x == 0) & torch.signbit(x)).any()) for x in xs)


def test_bilinear_by_hand_is_torchs():
    x = hp.r16(torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1)))
    for s in (2, 4, 8):
        want = F.interpolate(x.double(), scale_factor=s, mode="bilinear", align_corners=False)
        assert float((hp.bilinear_by_hand(x, s) - want).abs().max()) <= 1e-15


def test_wrong_roundings_are_what_they_say():
    t = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -11 + 2.0 ** -20), 1.0 + 2.0 ** -9, 70000.0, 2.0 ** -25 * 1.5, 1.0 + 2.0 ** -8 - 2.0 ** -20])
    assert hp.rne(t).tolist() == [1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0 + 2.0 ** -9, hp.INF, 2.0 ** -24, 1.0 + 2.0 ** -8]
    assert hp.trunc16(t).tolist() == [1.0, -1.0, 1.0 + 2.0 ** -9, 65504.0, 0.0, 1.0 + 2.0 ** -8 - 2.0 ** -10]
    assert hp.bf16_then_16(t).tolist()[:3] == [1.0, -1.0, 1.0]


def _caught_by(family, wrong):
    """the first small case of the family whose bar the wrong variant misses"""
    for case in hp.FAMILIES[family].cases:
        if case.big:
            continue
        inputs = hp.FAMILIES[family].build(case)
        got = wrong(case, inputs)
        if not got:
            continue
        want64 = hp.FAMILIES[family].ref(case, inputs, torch.float64)
        bars = hp.FAMILIES[family].bars(case)
        if any(hp.result_fails(case, k, v, want64) for k, v in got.items() if k in bars):
            return case.id
    return None


@pytest.mark.parametrize("family,name", [(f, n) for f, d in hp.WRONG.items() for n in d], ids=lambda v: v.replace(" ", "-"))
def test_a_wrong_kernel_is_caught(family, name):
    hit = _caught_by(family, hp.WRONG[family][name])
    print(f"{family}, {name}: caught by {hit}")
    assert hit is not None, f"no case of {family} tells '{name}' from the reference: the table is missing a case"


@pytest.mark.parametrize("family", hp.FP16_STORING)
@pytest.mark.parametrize("name", list(hp.ROUNDINGS), ids=lambda v: v.replace(" ", "-"))
def test_a_wrong_rounding_is_caught(family, name):
    rnd = hp.ROUNDINGS[name]
    hit = _caught_by(family, lambda case, inputs: hp.wrongly_rounded(case, inputs, rnd))
    print(f"{family}, fp32 result {name}: caught by {hit}")
    assert hit is not None, f"no case of {family} tells a result {name} from one rounded to nearest even"


def test_a_right_kernel_passes():
    """the fp32 torch evaluation rounded to nearest even, i.e. a right kernel, passes every small case: the sensitivity above is not a bar that fails everything"""
    for case in SMALL:
        inputs = hp.FAMILIES[case.family].build(case)
        want64 = hp.FAMILIES[case.family].ref(case, inputs, torch.float64)
        got = hp.wrongly_rounded(case, inputs, hp.rne)
        assert not any(hp.result_fails(case, k, v, want64) for k, v in got.items()), case.id
