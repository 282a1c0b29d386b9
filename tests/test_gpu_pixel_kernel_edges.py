"""The fp32 per-pixel kernels that share csrc/pixel_common.h, called through their `ops` wrappers at the shapes where kernels go wrong and
compared with the fp64 references of tests/pixel_edge_cases.py: a second round of every grid-stride walk, 3x3 windows on planes smaller
than the window and on odd planes, rows of 1 to 4096 columns, 1024-thread reductions over fewer values than threads, groups and planes of
one value, activations at 0, at tiny arguments and where expf overflows, channel slices of larger buffers.

Bars: those of the project's tests of the same ops (the cases module lists them), exact equality for data movement and for the max-pool.
Every comparison prints device-fp64, fp32 torch-fp64 and the bar, and asserts that the fp32 torch result lies within a quarter of the
bar (the inputs are fair) before it asserts the bar.  The two GroupNorm offset inputs (mean 100 and 1000 with a spread of 0.1 and 0.01)
are out of fp32 torch's reach; their bar is four times torch's own fp32 gap, which fp64 statistics meet with room and fp32 statistics
would miss by orders of magnitude.

Bilinear: the 1e-6 bar holds for power-of-two scales only (torch's own fp32 path is 1.2e-5 to 2.4e-5 from fp64 at scales 3, 5, 6); scale 1
is the identity, bit for bit, forward and backward.  Not covered: a max-pool window of -inf only (ATen sends its gradient to the window's
first element, window_argmax to none; the stem's pool follows a ReLU), NaN and +-inf inputs."""
import pytest
import torch

import pixel_edge_cases as pe
from semanticlidarunc_amd import ops
from semanticlidarunc_amd._lib import SluError

pytestmark = pytest.mark.gpu


def _run(cuda, case, fn):
    inputs, want64, want32 = pe.evaluate(case)
    dev = {k: v.to(cuda) if torch.is_tensor(v) else v for k, v in inputs.items()}
    got = fn(case, dev)
    torch.cuda.synchronize()
    pe.check(case, got, want64, want32)


def _cases(family):
    return pytest.mark.parametrize("case", pe.FAMILIES[family].cases, ids=pe.case_id)


# ---- 3x3 windows -------------------------------------------------------------------------------------------------------------------
@_cases("maxpool")
def test_maxpool3s2(cuda, case):
    def fn(c, d):
        out = dict(y=ops.maxpool3s2(d["x"]))
        if not c.big:
            out["dx"] = ops.maxpool3s2_bwd(d["x"], d["dy"])
        return out
    _run(cuda, case, fn)


@_cases("avgpool")
def test_avgpool3s2(cuda, case):
    def fn(c, d):
        if c.p["mode"].startswith("bcast"):
            return dict(y=ops.avgpool3s2_bcast(d["x"], d["scale"], d["n_out"]))
        out = dict(y=ops.avgpool3s2(d["x"], d["scale"]))
        out["y@bcast"] = ops.avgpool3s2_bcast(d["x"], d["scale"], d["n_out"])          # in_batch = n_out: the same result through the other entry
        return out
    _run(cuda, case, fn)


@_cases("dwconv")
def test_dwconv3x3(cuda, case):
    _run(cuda, case, lambda c, d: dict(y=ops.dwconv3x3(d["x"], d["w"], d["bias"], stride=c.p["stride"], act=c.p["act"])))


@_cases("dwwgrad")
def test_dwconv3x3_wgrad(cuda, case):
    _run(cuda, case, lambda c, d: dict(dw=ops.dwconv3x3_wgrad(d["x"], d["dy"])))


# ---- data movement -------------------------------------------------------------------------------------------------------------------
@_cases("nearest")
def test_nearest_down(cuda, case):
    def fn(c, d):
        out = dict(y=ops.nearest_down(d["x"], c.p["f"]))
        if not c.big:
            out["dx"] = ops.nearest_down_bwd(d["dy"], c.p["f"])
        return out
    _run(cuda, case, fn)


@_cases("s2d")
def test_space_to_depth2(cuda, case):
    def fn(c, d):
        if d["b"] is None:
            return dict(y=ops.space_to_depth2(d["a"]))
        return dict(y=ops.space_to_depth2_cat(d["a"], c.p["ca"], d["b"]))
    _run(cuda, case, fn)


@_cases("d2s")
def test_depth_to_space(cuda, case):
    def fn(c, d):
        p = c.p
        if p.get("fresh"):
            res = dict(out=ops.depth_to_space(d["x"], p["r"], p["elu"]))
        else:
            buf = torch.full(d["dy"].shape, pe.SENTINEL, device=cuda)          # the channels outside the slice must keep the sentinel
            assert ops.depth_to_space(d["x"], p["r"], p["elu"], out=buf, c_off=p["c_off"]) is buf
            res = dict(out=buf)
        if not p["elu"] and not c.big:
            res["dx"] = ops.depth_to_space_bwd(d["dy"], p["cout"], p["r"], p["c_off"])
        return res
    _run(cuda, case, fn)


@_cases("replace_tail")
def test_replace_tail(cuda, case):
    def fn(c, d):
        m = c.p["m"]
        res = dict(out=ops.replace_tail(d["x"], d["meta"]))
        res["dx"], res["dmeta"] = ops.replace_tail_bwd(d["dout"], m)
        if not c.big:
            res["dx@only"], none = ops.replace_tail_bwd(d["dout"], m, want_dmeta=False)
            assert none is None
            none, res["dmeta@only"] = ops.replace_tail_bwd(d["dout"], m, want_dx=False)
            assert none is None
        return res
    _run(cuda, case, fn)


# ---- row softmax ---------------------------------------------------------------------------------------------------------------------
@_cases("rowsoftmax")
def test_row_softmax_mul(cuda, case):
    def fn(c, d):
        res = dict(out=ops.row_softmax_mul(d["score"], d["value"]))
        res["dscore"], res["dvalue"] = ops.row_softmax_mul_bwd(d["score"], d["value"], d["dout"])
        res["dscore@only"], none = ops.row_softmax_mul_bwd(d["score"], d["value"], d["dout"], want_dvalue=False)
        assert none is None
        none, res["dvalue@only"] = ops.row_softmax_mul_bwd(d["score"], d["value"], d["dout"], want_dscore=False)
        assert none is None
        return res
    _run(cuda, case, fn)


def test_row_softmax_mul_refuses_4097_columns(cuda):
    """W = 4097 does not fit the kernels' LDS row: both wrappers raise, and nothing is launched"""
    score, value = torch.zeros(1, 1, 1, 4097, device=cuda), torch.ones(1, 2, 1, 4097, device=cuda)
    with pytest.raises(SluError):
        ops.row_softmax_mul(score, value)
    with pytest.raises(SluError):
        ops.row_softmax_mul_bwd(score, value, value.clone())
    torch.cuda.synchronize()


# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
@_cases("bilinear")
def test_bilinear_upsample(cuda, case):
    def fn(c, d):
        out = dict(y=ops.bilinear_upsample(d["x"], c.p["s"]))
        if not c.big:
            out["dx"] = ops.bilinear_upsample_bwd(d["dy"], c.p["s"])
        return out
    _run(cuda, case, fn)


# ---- 1024-thread reductions: GroupNorm and the spatial gate -----------------------------------------------------------------------------
@_cases("groupnorm")
def test_groupnorm(cuda, case):
    def fn(c, d):
        p = c.p
        y, stats = ops.groupnorm(d["x"], p["groups"], d["gamma"], d["beta"], pe.EPS, relu=p["relu"], return_stats=True)
        alone = ops.groupnorm_stats(d["x"], p["groups"], pe.EPS)
        assert torch.equal(alone, stats), f"{c.id}: groupnorm_stats alone differs from the statistics of groupnorm(return_stats=True)"
        res = dict(y=y, mean=stats[0], rstd=stats[1])
        if p["bwd"]:
            dx, dg, db = ops.groupnorm_bwd(d["x"], y, d["dy"], d["gamma"], stats, p["groups"], p["relu"], want_affine=p["want_affine"])
            res["dx"] = dx
            if p["want_affine"]:
                res["dgamma"], res["dbeta"] = dg, db
            else:
                assert dg is None and db is None
        return res
    _run(cuda, case, fn)


@_cases("gate")
def test_spatial_softmax_gate(cuda, case):
    def fn(c, d):
        out, stats = ops.spatial_softmax_gate(d["x"], d["score"], return_stats=True)
        res = dict(out=out, smax=stats[0::2], sinv=stats[1::2])
        if not c.big:
            res["dx"], res["dscore"] = ops.spatial_softmax_gate_bwd(d["x"], d["score"], stats, d["dout"])
        return res
    _run(cuda, case, fn)


# ---- activations -----------------------------------------------------------------------------------------------------------------------
@_cases("pointwise")
def test_pointwise(cuda, case):
    def fn(c, d):
        op, slope = pe.POINTWISE[c.p["name"]]
        y = ops.pointwise_fwd(d["x"], op, slope)
        # as the autograd nodes call it: from the forward's output, SiLU from its input
        dx = ops.pointwise_bwd(d["dy"], d["x"] if op == "silu" else y, op, slope)
        if c.p["name"] in pe.GRAD_AT_ZERO and not c.big:          # x[0] = 0 (and x[1] = -0): ATen's choice of the gradient there
            want = torch.tensor(pe.GRAD_AT_ZERO[c.p["name"]], dtype=torch.float32)
            for k in range(min(2, c.p["n"])):
                assert float(dx[k]) == float(d["dy"][k].cpu() * want), f"{c.id}: gradient at x = {float(d['x'][k])}"
        return dict(y=y, dx=dx)
    _run(cuda, case, fn)


# ---- SqueezeExcitation -----------------------------------------------------------------------------------------------------------------
@_cases("gap")
def test_global_avgpool(cuda, case):
    _run(cuda, case, lambda c, d: dict(avg=ops.global_avgpool(d["x"])))


@_cases("se")
def test_se_scale(cuda, case):
    _run(cuda, case, lambda c, d: dict(scale=ops.se_scale(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])))


def test_se_scale_refuses_one_channel_past_the_lds_limit(cuda):
    """C + S = 16385 floats do not fit 64 KB of LDS: the gate is refused before its launch"""
    c, s = pe.SE_MAX[0] + 1, pe.SE_MAX[1]
    with pytest.raises(SluError):
        ops.se_scale(torch.zeros(1, c, 1, 1, device=cuda), torch.zeros(s, c, device=cuda), None, torch.zeros(c, s, device=cuda), None)
    torch.cuda.synchronize()
