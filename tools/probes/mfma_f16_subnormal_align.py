"""Probe: how v_mfma_f32_32x32x16_f16 aligns the products of a K-step when some operands are fp16 subnormals (un-normalised), seen
through the split-fp16 1x1 conv with a few nonzero channels whose hi parts are exact (lo = 0).  Run from the repository root on the
GPU; prints, per configuration, how many of 32 x 32 outputs equal the rounded exact sum and the range of got - exact.  Findings and the
model built from them: profiles/r29/README.md, tests/f16x3_restatement.py::fused_conv_split_mfma."""
import sys
sys.path.insert(0, ".")
import torch
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.ops import ConvSource

dev = torch.device("cuda:0")
u = 2.0 ** -24
k = torch.arange(1, 33).double()
m = torch.arange(1, 33).double()


def run(x, w):
    wp = ops.pack_conv_weight_f16x3(w.float().to(dev).contiguous())
    out = ops.conv2d_fused([ConvSource(x.float().to(dev).contiguous())], wp, w.shape[0], 1, 1, 0, precision="f16x3")
    torch.cuda.synchronize()
    return out.cpu()[0, :, 0, :].double()


def case(tag, terms, cin=32):
    """terms: list of (channel, xvec[32] or scalar, wvec[32] or scalar)."""
    x = torch.zeros(1, cin, 1, 32, dtype=torch.float64)
    w = torch.zeros(32, cin, 1, 1, dtype=torch.float64)
    exact = torch.zeros(32, 32, dtype=torch.float64)
    for ch, xv, wv in terms:
        xv = torch.as_tensor(xv, dtype=torch.float64).expand(32)
        wv = torch.as_tensor(wv, dtype=torch.float64).expand(32)
        x[0, ch, 0, :] = xv
        w[:, ch, 0, 0] = wv
        exact += wv[:, None] * xv[None, :]
    got = run(x, w)
    d = got - exact
    r32 = exact.float().double()
    print(f"{tag}: got==fp32(exact) {int((got == r32).sum())}/1024  min d {float(d.min()):.4e} max d {float(d.max()):.4e}  "
          f"log2 max|d| {float(d.abs().max().log2()) if d.abs().max() > 0 else float('-inf'):.2f}")
    return got, exact


BIGS = [(4 * u, 1.0)]
# P1 grouping: big (subnormal 2^-22 x 1.0, exponent fields -14 + 0) and small (subnormal x subnormal, k m 2^-42) at various channels
for cb, cs in [(0, 1), (0, 4), (0, 7), (0, 8), (0, 15), (3, 12), (9, 10), (0, 16), (16, 0), (5, 21), (21, 5)]:
    case(f"P1 big ch {cb} small ch {cs}", [(cb, 4 * u, 1.0), (cs, k * u, m * u * 64)])
# P2 sign
case("P2 small negative", [(0, 4 * u, 1.0), (1, k * u, -m * u * 64)])
case("P2 big negative", [(0, 4 * u, -1.0), (1, k * u, m * u * 64)])
case("P2 both negative", [(0, 4 * u, -1.0), (1, k * u, -m * u * 64)])
# P3 big from two normal operands of the same value 2^-22: exponent fields -11 + -11
case("P3 big normal x normal", [(0, 2.0 ** -11, 2.0 ** -11), (1, k * u, m * u * 64)])
case("P3 big normal x normal, other K-step", [(0, 2.0 ** -11, 2.0 ** -11), (16, k * u, m * u * 64)])
# P4 window and final rounding with normal operands: 1 + k m 2^-28 (k m up to 1024: bits from 2^-28 to 2^-18)
case("P4 one plus small, same K-step", [(0, 1.0, 1.0), (1, k * 2.0 ** -14, m * 2.0 ** -14)])
case("P4 one plus small, next K-step", [(0, 1.0, 1.0), (16, k * 2.0 ** -14, m * 2.0 ** -14)])
case("P4 small then one, next K-step", [(16, 1.0, 1.0), (0, k * 2.0 ** -14, m * 2.0 ** -14)])
g, e = case("P4 minus one plus small", [(0, 1.0, -1.0), (1, k * 2.0 ** -14, m * 2.0 ** -14)])
print("   sample got-exact in 2^-28 units, row m=1:", ((g - e)[0] * 2.0 ** 28).tolist()[:16])
g, e = case("P4 one plus small again", [(0, 1.0, 1.0), (1, k * 2.0 ** -14, m * 2.0 ** -14)])
print("   sample got-exact in 2^-28 units, row m=1:", ((g - e)[0] * 2.0 ** 28).tolist()[:16])
print("   sample got-exact in 2^-28 units, row m=3:", ((g - e)[2] * 2.0 ** 28).tolist()[:16])
# P5 many small terms against one un-normalised big: 15 channels of small
case("P5 15 smalls one big", [(0, 4 * u, 1.0)] + [(c, k * u, m * u * 64) for c in range(1, 16)])
case("P5 15 smalls one big alternating sign", [(0, 4 * u, 1.0)] + [(c, k * u, m * u * 64 * (-1) ** c) for c in range(1, 16)])
# P6 lo path: w with a lo part (normal hi, subnormal lo) times subnormal x
case("P6 w = 0.04 + lo, x subnormal", [(0, k * u, 0.04 + m * u)])
case("P6 w = 0.04 + lo, x subnormal, 16 channels", [(c, k * u, 0.04 + m * u) for c in range(16)])
