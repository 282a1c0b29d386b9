"""The fp16-storage ("h8") per-pixel kernels of csrc/fpn_opt_h8.hip, csrc/fpn_h8.hip and csrc/layout_h8.hip, called through their
`h8` wrappers at the shapes where kernels go wrong and compared with the fp64 references of tests/h8_pixel_edge_cases.py: a second round
of grid y and of grid z of the row walk, of the 32 768-block and the 4 096-tile grid-stride loops, GroupNorm planes cut into ragged parts
and into more parts than the finalize kernel has lanes, groups 1 / 2 / 4 / 8 wide at every slot, constant planes, the scalar and the
vector statistics of the gate with fewer scores than threads, rows of 1 to 4096 columns, planes of one pixel, pad channels, results in the
fp16 subnormal range, at 65504 and past it, -inf and signed zeros.

Bars (the cases module derives them): exact equality for data movement, and for arithmetic that stores fp16 half an fp16 ulp of the fp64
result -- the one rounding to nearest even a kernel is entitled to -- plus a coefficient for the fp32 arithmetic ahead of it; a reference
value of 65520 or more must come back as the infinity.  Every comparison prints the worst error next to its bar.  h8 tensors are packed and
unpacked with plain torch on the CPU, so no kernel under test prepares another one's data; pad channels must be 0, the sentinel blocks
around an output slice untouched, and two runs of a kernel give the same bits (every reduction has a fixed order).

Measured on an MI355X, worst case of each family: avgpool, bilinear, to_h8 and PixelShuffle with multipliers are correctly rounded (nothing
beyond the half ulp); beyond it the gate uses 0.005 of its coefficient term, GroupNorm apply 0.105, the attention row 0.284; GroupNorm mean and
rstd are 5.6e-8 relative (bar 2.4e-7), ELU + 1 is 6.0e-8 (bar 1e-6); every exact family is bit for bit."""
import pytest
import torch

import h8_pixel_edge_cases as hp
from semanticlidarunc_amd import h8
from semanticlidarunc_amd._lib import SluError

pytestmark = pytest.mark.gpu


def _cases(family):
    return pytest.mark.parametrize("case", hp.FAMILIES[family].cases, ids=hp.case_id)


def _h8_out(y8, shape, c=None):
    """an h8 result on the device -> NCHW fp32 on the CPU, after its shape, dtype and (c given: the real channels) zero pad channels"""
    assert y8.dtype == torch.float16 and tuple(y8.shape) == tuple(shape) and y8.is_contiguous(), (y8.dtype, tuple(y8.shape), tuple(shape))
    y = hp.unpack_h8(y8.cpu())
    if c is None:
        return y
    assert bool((y[:, c:] == 0).all()), "pad channels are not 0"
    return y[:, :c].contiguous()


def _run(cuda, case, fn):
    """fn(case, inputs on the device) -> {result: device tensor or CPU NCHW tensor}, twice: the same bits, then against the references"""
    inputs, want64, want32 = hp.evaluate(case)
    dev = {k: v.to(cuda) if torch.is_tensor(v) else v for k, v in inputs.items() if k not in hp.STORED[case.family]}
    for k in hp.STORED[case.family]:
        dev[k] = hp.pack_h8(inputs[k]).to(cuda)
    first = fn(case, dev)
    again = fn(case, dev)
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k], again[k]), f"{case.id} {k}: two runs differ"
    hp.check(case, first, want64, want32)


def _sentinel(cuda, n, g, h, w):
    return torch.full((n, g, h, w, 8), hp.SENTINEL, dtype=torch.float16, device=cuda)


# ---- the row walk: pools, space <-> depth, bilinear -----------------------------------------------------------------------------------
@_cases("maxpool")
def test_maxpool3s2_h8(cuda, case):
    def fn(c, d):
        p = c.p
        g, (h, w) = (p["c"] + 7) // 8, p["hw"]
        return dict(y=_h8_out(h8.maxpool3s2_h8(d["x"]), (p["n"], g, (h + 1) // 2, (w + 1) // 2, 8), p["c"]))
    _run(cuda, case, fn)


@_cases("avgpool")
def test_avgpool3s2_h8(cuda, case):
    def fn(c, d):
        p = c.p
        g, (h, w) = (p["c"] + 7) // 8, p["hw"]
        y8 = h8.avgpool3s2_h8(d["x"], d["scale"], d["n_out"] if p["mode"] == "bcast" else None)
        return dict(y=_h8_out(y8, (d["n_out"], g, (h + 1) // 2, (w + 1) // 2, 8), p["c"]))
    _run(cuda, case, fn)


@_cases("s2d")
def test_space_to_depth2_h8(cuda, case):
    def fn(c, d):
        p = c.p
        g, (oh, ow) = (p["c"] + 7) // 8, p["out"]
        y, y00 = h8.space_to_depth2_h8(d["x"], d["meta"], channels=p["c"] if p["m"] else None, factor=p["f"], phase00=p["phase00"])
        res = dict(y=_h8_out(y, (p["n"], 4 * g, oh, ow, 8)))          # pad channels lie inside every phase: the reference holds them
        if p["phase00"]:
            res["y00"] = _h8_out(y00, (p["n"], g, oh, ow, 8))
        else:
            assert y00 is None
        return res
    _run(cuda, case, fn)


@_cases("d2s")
def test_depth_to_space_h8(cuda, case):
    def fn(c, d):
        p = c.p
        s, (h, w), go = p["s"], p["hw"], p["cout"] // 8
        if p["gtot"] == go and p["g_off"] == 0:
            out = h8.depth_to_space_h8(d["x"], s)
        else:
            out = _sentinel(cuda, p["n"], p["gtot"], s * h, s * w)          # the blocks outside the slice must keep the sentinel
            assert h8.depth_to_space_h8(d["x"], s, out=out, g_off=p["g_off"]) is out
        return dict(out=_h8_out(out, (p["n"], p["gtot"], s * h, s * w, 8)))
    _run(cuda, case, fn)


@_cases("elu")
def test_depth_to_space2_elu_h8(cuda, case):
    def fn(c, d):
        p = c.p
        out = h8.depth_to_space_h8(d["x"], 2, elu_plus_one=True, classes=p["classes"])
        assert out.dtype == torch.float32 and tuple(out.shape) == (p["n"], p["classes"], 2 * p["hw"][0], 2 * p["hw"][1])
        return dict(out=out.cpu())
    _run(cuda, case, fn)


@_cases("bilinear")
def test_bilinear_upsample_h8(cuda, case):
    def fn(c, d):
        p = c.p
        s, (h, w) = p["s"], p["hw"]
        return dict(y=_h8_out(h8.bilinear_upsample_h8(d["x"], s), (p["n"], (p["c"] + 7) // 8, s * h, s * w, 8), p["c"]))
    _run(cuda, case, fn)


# ---- GroupNorm, the spatial gate, the attention row -----------------------------------------------------------------------------------
@_cases("groupnorm")
def test_groupnorm_h8(cuda, case):
    def fn(c, d):
        p = c.p
        n, ch, (h, w), g = p["n"], p["c"], p["hw"], (p["c"] + 7) // 8
        stats = h8.groupnorm_stats_h8(d["x"], ch, p["groups"], hp.EPS)
        assert stats.dtype == torch.float32 and tuple(stats.shape) == (2, n * p["groups"])
        if p["dest"] == "slice":
            buf = _sentinel(cuda, n, g + 2, h, w)
            assert h8.groupnorm_apply_h8(d["x"], ch, p["groups"], stats, d["gamma"], d["beta"], relu=p["relu"], out=buf, g_off=1) is buf
            assert bool((buf[:, 0] == hp.SENTINEL).all()) and bool((buf[:, g + 1] == hp.SENTINEL).all()), "a block outside the slice was written"
            y8 = buf[:, 1:g + 1].contiguous()
        elif p["dest"] == "inplace":
            y8 = d["x"].clone()
            assert h8.groupnorm_apply_h8(y8, ch, p["groups"], stats, d["gamma"], d["beta"], relu=p["relu"], out=y8) is y8
        else:
            y8 = h8.groupnorm_apply_h8(d["x"], ch, p["groups"], stats, d["gamma"], d["beta"], relu=p["relu"])
        return dict(mean=stats[0].cpu(), rstd=stats[1].cpu(), y=_h8_out(y8, (n, g, h, w, 8), ch))
    _run(cuda, case, fn)


@pytest.mark.parametrize("c,groups", [(24, 8), (20, 4), (48, 3)])
def test_groupnorm_h8_refuses_groups_that_straddle_a_record(cuda, c, groups):
    x8 = torch.zeros(1, (c + 7) // 8, 2, 4, 8, dtype=torch.float16, device=cuda)
    with pytest.raises(SluError):
        h8.groupnorm_stats_h8(x8, c, groups)
    torch.cuda.synchronize()


def test_groupnorm_h8_refuses_65536_planes(cuda):
    """grid y holds 65535 planes; one more is refused before any launch, and 65535 planes of one record run"""
    x8 = torch.zeros(65536, 1, 1, 1, 8, dtype=torch.float16, device=cuda)
    with pytest.raises(SluError):
        h8.groupnorm_stats_h8(x8, 8, 1)
    stats = h8.groupnorm_stats_h8(x8[:65535], 8, 1)
    torch.cuda.synchronize()
    assert bool((stats[0] == 0).all()) and bool((stats[1] == float(torch.tensor(hp.EPS, dtype=torch.float64).rsqrt().float())).all())


@_cases("gate")
def test_spatial_softmax_gate_h8(cuda, case):
    def fn(c, d):
        p = c.p
        return dict(out=_h8_out(h8.spatial_softmax_gate_h8(d["x"], d["score"]), (p["n"], (p["c"] + 7) // 8) + p["hw"] + (8,), p["c"]))
    _run(cuda, case, fn)


@_cases("attention")
def test_attention_row_h8(cuda, case):
    def fn(c, d):
        p = c.p
        return dict(out=_h8_out(h8.attention_row_h8(d["tv"], d["w_a"], d["b_a"]), (p["n"], p["c"] // 8, p["h"], p["w"], 8)))
    _run(cuda, case, fn)


@pytest.mark.parametrize("c,w", [(8, 4097), (520, 2)])
def test_attention_row_h8_refuses_what_does_not_fit_its_lds(cuda, c, w):
    """W = 4097 does not fit the LDS row and C = 520 not the LDS weights: refused before the launch"""
    tv = torch.zeros(1, c // 4, 1, w, 8, dtype=torch.float16, device=cuda)
    with pytest.raises(SluError):
        h8.attention_row_h8(tv, torch.zeros(c, device=cuda), torch.zeros(1, device=cuda))
    torch.cuda.synchronize()


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
@_cases("to_h8")
def test_to_h8(cuda, case):
    def fn(c, d):
        p = c.p
        return dict(y=_h8_out(h8.to_h8(d["x"], d["scale"]), (p["n"], (p["c"] + 7) // 8) + p["hw"] + (8,), p["c"]))
    _run(cuda, case, fn)


@_cases("from_h8")
def test_from_h8(cuda, case):
    def fn(c, d):
        p = c.p
        y = h8.from_h8(d["x"], p["c"])
        assert y.dtype == torch.float32 and tuple(y.shape) == (p["n"], p["c"]) + p["hw"]
        return dict(y=y.cpu())
    _run(cuda, case, fn)


@_cases("pixelshuffle")
def test_pixel_shuffle_h8(cuda, case):
    def fn(c, d):
        p = c.p
        (h, w), co = p["hw"], 2 * p["gi"]
        return dict(y=_h8_out(h8.pixel_shuffle_h8(d["x"], d["s_in"], d["s_out"]), (p["n"], (co + 7) // 8, 2 * h, 2 * w, 8), co))
    _run(cuda, case, fn)
