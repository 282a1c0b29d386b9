"""GPU: the exact-fp32 conv (conv2d.hip) and the split-fp16 conv (conv2d_f16x3.hip) held to bit equality on inputs whose answer is
exact in any summation order (conv_lattice_cases.py): no tolerance to choose, and a lost `lo` image of one tap, of a halo column, of
the ragged last K-chunk, of one source of a concat or of the packed weights changes bits (test_conv_lattice_cpu.py shows each does).

Two orientations: "x" (the input carries a lo, the weight none) and "w" (the weight carries a lo, the input none), so the dropped
lo*lo term is exactly zero and hi*lo, lo*hi are each exercised.  Every nonzero lo is a normal fp16, so nothing here hinges on how the
matrix core treats subnormal operands (test_gpu_f16x3_split.py measures that).
  * the small shapes of test_gpu_conv.py / test_gpu_f16x3.py (tile edges, K-chunks, source boundaries), both precisions;
  * every row of test_gpu_dispatch_coverage's FP32_CASES and F16X3_CASES at its own precision, shape, options and kernel name;
    `big` rows scale the lattice by 16, `stats` rows keep their statistics check;
  * the same call twice gives the same bits."""
import pytest
import torch

from conv_lattice_cases import lattice_case, small_cases, table_case_kwargs
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.ops import ConvSource
from test_gpu_dispatch_coverage import F16X3_CASES, FP32_CASES, _id

pytestmark = pytest.mark.gpu
SMALL = small_cases()
# the instantiations the 1x1 shapes must reach: the streaming split-fp16 kernel, and the tiled one where H W % 32 != 0
SMALL_NAMES = {("tile|k1d1|32->32|N2|16x128", "f16x3"): "conv1x1_f16x3_kernel<1, 1>",
               ("tile|k1d1|32->64|N2|8x64", "f16x3"): "conv1x1_f16x3_kernel<2, 1>",
               ("tile|k1d1|32->128|N2|8x64", "f16x3"): "conv1x1_f16x3_kernel<4, 1>",
               ("tile|k1d1|32->256|N2|4x64", "f16x3"): "conv1x1_f16x3_kernel<8, 1>",
               ("concat-plain|k1d1|64+64+64->64|N2|8x64", "f16x3"): "conv1x1_f16x3_kernel<2, 1>",
               ("tiled-1x1|k1d1|32->64|N1|5x12", "f16x3"): "conv_f16x3_kernel<1, 1, 0, 1, 1, 4, 1, false>",
               ("tiled-1x1|k1d1|32->64|N1|5x12", "fp32"): "conv_fwd_kernel<1, 1, 0, 16, 1, 1, 4, 1, false>"}


def run_conv(dev, c, precision, stats=False, expect_kernel=None):
    """One launch of ops.conv2d_fused on a case of conv_lattice_cases / f16x3_split_cases; returns (output, statistics or None)."""
    d = lambda t: None if t is None else t.to(dev).contiguous()
    cout = c.wgt.shape[0]
    wpack = (ops.pack_conv_weight_f16x3 if precision == "f16x3" else ops.pack_conv_weight)(d(c.wgt))
    srcs = [ConvSource(d(t), d(s), ps) for t, s, ps in c.srcs]
    st = torch.zeros((2, cout), dtype=torch.float64, device=dev) if stats else None
    if expect_kernel is not None:
        ops.TIMING, ops.TIMING_TAGS = [], []              # measurement mode records the instantiation slu_conv2d_kernel_name reports
    try:
        got = ops.conv2d_fused(srcs, wpack, cout, c.k, c.dil, c.pad, bias=d(c.bias), slope=c.slope, bn_a=d(c.bn_a), bn_b=d(c.bn_b),
                               resid=d(c.res), precision=precision, stats=st)
        launched = [t[0] for t in ops.TIMING] if expect_kernel is not None else None
    finally:
        if expect_kernel is not None:
            ops.TIMING, ops.TIMING_TAGS = None, []
    torch.cuda.synchronize()
    if expect_kernel is not None:
        assert launched == [expect_kernel], launched
    return got, st


def _mismatch(got, want):
    """Where the bits differ: count, the largest difference, and the (n, c, y, x) box -- the pattern localises a lost image."""
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    return (f"{int(bad.sum())} of {bad.numel()} elements differ, max |diff| {float((got - want)[bad].abs().max()):.3e}, "
            f"first {idx[0].tolist()}, box min {idx.min(0).values.tolist()} max {idx.max(0).values.tolist()}")


def _bit_equal(got, want):
    got = got.cpu()
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("orient", ["x", "w"])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,kw", SMALL, ids=[c[0] for c in SMALL])
def test_small_shape_is_bit_exact(cuda, name, kw, precision, orient):
    c = lattice_case(orient=orient, verify=True, **kw)
    got, _ = run_conv(cuda, c, precision, expect_kernel=SMALL_NAMES.get((name, precision)))
    _bit_equal(got, c.want)


def _table_row(dev, row, precision, orient):
    name, opts = row[0], row[7]
    c = lattice_case(orient=orient, verify=False, **table_case_kwargs(row))
    got, st = run_conv(dev, c, precision, stats=bool(opts.get("stats")), expect_kernel=name)
    _bit_equal(got, c.want)
    if st is not None:                                      # as test_gpu_conv._run: the fused BatchNorm statistics of the stored output
        s, q = ops.bn_stats(got)
        assert float(((st[0] - s).abs() / (s.abs() + 1.0)).max()) <= 1e-5 and float(((st[1] - q).abs() / q).max()) <= 1e-5
        ref = got.double()
        assert float(((st[0] - ref.sum((0, 2, 3))).abs() / (ref.abs().sum((0, 2, 3)) + 1.0)).max()) <= 1e-6


@pytest.mark.parametrize("orient", ["x", "w"])
@pytest.mark.parametrize("row", FP32_CASES, ids=_id)
def test_fp32_table_row_is_bit_exact(cuda, row, orient):
    _table_row(cuda, row, "fp32", orient)


@pytest.mark.parametrize("orient", ["x", "w"])
@pytest.mark.parametrize("row", F16X3_CASES, ids=_id)
def test_f16x3_table_row_is_bit_exact(cuda, row, orient):
    _table_row(cuda, row, "f16x3", orient)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_same_call_twice_gives_the_same_bits(cuda, precision):
    # ordinary values here: on a lattice every order gives the same bits, so equality there would say nothing about the order of a run
    from f16x3_split_cases import SPLIT_CASES, split_case
    for i, (name, _) in enumerate(SPLIT_CASES):
        if name.startswith(("ragged-full", "concat|", "shuffle", "tiled-1x1")):
            c = split_case(i)
            a, _ = run_conv(cuda, c, precision)
            b, _ = run_conv(cuda, c, precision)
            assert torch.equal(a, b) and not bool(torch.isnan(a).any()), name
