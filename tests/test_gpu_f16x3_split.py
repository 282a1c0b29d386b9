"""GPU: the split-fp16 conv on ordinary values, judged against a CPU restatement of its own arithmetic (f16x3_restatement.py), and
the exact-fp32 conv against fp64 at the same bar.

    f16x3:  max|got - want_split| <= 4 e_ref + 1e-7 S        fp32:  max|got - want64| <= 4 e_ref + 1e-7 S
want_split is the three-term sum hi*hi + hi*lo + lo*hi in fp64 (the kernel differs from it by fp32 accumulation only), want64 the
exact fp64 operator, e_ref = max|fp32 CPU conv - want64| on the same case (the reference is the CPU conv, never the kernel),
S = max|want64| with no floor; 4 is the project's margin for another fp32 summation order (test_gpu_backward.py).  That is about
1e-6 S, where test_gpu_f16x3.py accepts 1e-4 / 2e-5 of max(1, S); test_f16x3_restatement_cpu.py shows every lost piece of a lo image is
more than 10 x outside it.  One case carries a margin of 16 instead of 4 (f16x3_split_cases.MARGIN, with the measured ratios).

The magnitude sweep scales x by 2^ex and w by 2^ew: down into the range where hi and lo are fp16 subnormals, and up (ex = +14) past
65504 where hi saturates.  The kernel is held to the restatement at the same bar in every cell; its distance to the exact answer is
the restatement's (test_f16x3_restatement_cpu.py states the law) and is printed, not asserted.
What the sweep found (profiles/r29): the fp16 MFMA keeps subnormal operands -- every cell down to ex = -18 follows the plain restatement
-- but aligns the addends of a block by exponent field, so at ex = -24 (hi of x is 0..4 steps of 2^-24, ten bits un-normalised) the
accumulator loses the hi*lo sums: 2e-5 S from the plain restatement, in a cell that is 0.5 S from the exact answer either way.  Those
cells (`affected`: decided on the CPU, where the model leaves the plain restatement by more than the bar) are held to
f16x3_restatement.fused_conv_split_mfma, the same sum through a model of that alignment, at the same bar."""
import pytest
import torch

from f16x3_split_cases import SPLIT_CASES, SWEEP_EW, SWEEP_EX, SWEEP_SHAPES, split_case, sweep_case
from test_gpu_conv_lattice import run_conv

pytestmark = pytest.mark.gpu


def _judge(dev, c, precision, what, model=False):
    got, _ = run_conv(dev, c, precision)
    got = got.cpu().double()
    assert not bool(torch.isnan(got).any()), what
    want, name = (c.want_mfma, "want_mfma") if model else ((c.want_split, "want_split") if precision == "f16x3" else (c.want64, "want64"))
    err = float((got - want).abs().max())
    dist = lambda a, b: float((a - b).abs().max()) / c.S
    print(f"{what} {precision}: S {c.S:.3e}  |got - {name}| {err:.3e} = {err / c.S:.2e} S = {err / c.e_ref:.2f} e_ref   "
          f"e_ref {c.e_ref:.3e} = {c.e_ref / c.S:.2e} S   |got - want_split| {dist(got, c.want_split):.2e} S   "
          f"|want_split - want64| {dist(c.want_split, c.want64):.2e} S   |got - want64| {dist(got, c.want64):.2e} S"
          + (f"   |got - want_mfma| {dist(got, c.want_mfma):.2e} S" if hasattr(c, "want_mfma") else ""))
    assert err <= c.bar, (what, precision, err, c.bar, err / c.e_ref)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("i", range(len(SPLIT_CASES)), ids=[c[0] for c in SPLIT_CASES])
def test_kernel_follows_its_restatement(cuda, i, precision):
    _judge(cuda, split_case(i), precision, SPLIT_CASES[i][0])


@pytest.mark.parametrize("ew", SWEEP_EW)
@pytest.mark.parametrize("ex", SWEEP_EX)
@pytest.mark.parametrize("shape_i", range(len(SWEEP_SHAPES)), ids=[s[0] for s in SWEEP_SHAPES])
def test_magnitude_sweep_follows_the_restatement(cuda, shape_i, ex, ew):
    c = sweep_case(shape_i, ex, ew)
    _judge(cuda, c, "f16x3", f"{SWEEP_SHAPES[shape_i][0]} ex {ex} ew {ew}{' (affected)' if c.affected else ''}", model=c.affected)
