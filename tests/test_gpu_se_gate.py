"""GPU: the one SqueezeExcitation gate kernel (csrc/se_gate.hip) through its three entry points -- slu_se_gate (ops.se_scale), slu_regnet_se_gate
(ops.regnet_se_gate, ReLU), slu_se_gate_psum (ops.se_gate_psum, SiLU) -- against the fp64 formula and against each other.

Bar: 1e-5 absolute on outputs in (0, 1), the bar of test_gpu_regnet.py::test_gate_kernel and test_gpu_mbconv_unit.py::test_gate_kernel.  Where two
entry points compute the same chain (a plain mean, T = 1) they agree bit for bit, and the mean the kernel writes is the fp32 tile-order sum.
Shapes (C, S, T), N = 2: one channel; odd sizes with three tiles; one channel in the second slice of a 256-thread launch with more hidden
units (17) than the 16 waves of slu_se_gate_psum, so the wave loop wraps; the limit of slu_se_gate_psum.  Null biases through se_scale are also
the case "se_scale C65 S3 no bias" of pixel_edge_cases.py."""
import pytest
import torch
import torch.nn.functional as F

from semanticlidarunc_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (65, 3, 3), (257, 17, 1), (1536, 96, 3)]
N, COUNT = 2, 7
_PROBLEMS = {}


def _problem(c, s, t):
    """Drawn as in test_gpu_mbconv_unit.py::test_gate_kernel; the means are pushed away from zero so that no element is a zero of either sign."""
    if (c, s, t) not in _PROBLEMS:
        g = torch.Generator().manual_seed(1000 * t + s + c)
        mean = torch.randn(N, c, generator=g)
        mean = torch.where(mean >= 0, mean + 0.01, mean - 0.01)
        w1 = torch.randn(s, c, generator=g) * (2.0 / c) ** 0.5
        w2 = torch.randn(c, s, generator=g) * (2.0 / s) ** 0.5
        b1, b2 = torch.randn(s, generator=g) * 0.5, torch.randn(c, generator=g) * 0.5
        if t == 1:
            psum, count = mean.unsqueeze(2).clone(), 1
        else:                                                                              # the same means as t partial sums over COUNT pixels
            parts = torch.rand(N, c, t, generator=g) + 0.5
            psum, count = parts / parts.sum(2, keepdim=True) * (mean * float(COUNT)).unsqueeze(2), COUNT
        assert bool((psum != 0).all())
        _PROBLEMS[(c, s, t)] = (psum, count, w1, b1, w2, b2)
    return _PROBLEMS[(c, s, t)]


def _want(psum, count, w1, b1, w2, b2, act):
    mean = psum.double().sum(2) / count
    hid = F.linear(mean, w1.double(), None if b1 is None else b1.double())
    return torch.sigmoid(F.linear(act(hid), w2.double(), None if b2 is None else b2.double()))


@pytest.mark.parametrize("c,s,t", SHAPES, ids=[f"C{c}_S{s}_T{t}" for c, s, t in SHAPES])
def test_both_activations_against_fp64(cuda, c, s, t):
    psum, count, w1, b1, w2, b2 = _problem(c, s, t)
    d = [x.to(cuda) for x in (w1, b1, w2, b2)]
    for name, fn, act in (("silu", ops.se_gate_psum, F.silu), ("relu", ops.regnet_se_gate, F.relu)):
        got = fn(psum.to(cuda), count, *d)
        err = float((got.cpu().double() - _want(psum, count, w1, b1, w2, b2, act)).abs().max())
        print(f"C {c}, S {s}, T {t}, {name}: err {err:.2e}")
        assert got.shape == (N, c) and err <= 1e-5                                         # NaN fails
        assert torch.equal(fn(psum.to(cuda), count, *d), got)                              # the same bits every run


@pytest.mark.parametrize("c,s,t", SHAPES, ids=[f"C{c}_S{s}_T{t}" for c, s, t in SHAPES])
def test_the_mean_written_is_the_tile_order_sum(cuda, c, s, t):
    psum, count, w1, b1, w2, b2 = _problem(c, s, t)
    gate, mean = ops.regnet_se_gate(psum.to(cuda), count, *[x.to(cuda) for x in (w1, b1, w2, b2)], want_mean=True)
    acc = torch.zeros(N, c)
    for i in range(t):
        acc = acc + psum[:, :, i]
    assert torch.equal(mean.cpu(), acc * torch.tensor(1.0 / float(count), dtype=torch.float32))
    assert torch.equal(gate, ops.regnet_se_gate(psum.to(cuda), count, *[x.to(cuda) for x in (w1, b1, w2, b2)]))


@pytest.mark.parametrize("c,s", [(c, s) for c, s, _ in SHAPES], ids=[f"C{c}_S{s}" for c, s, _ in SHAPES])
def test_a_plain_mean_gives_the_same_bits_through_every_silu_entry_point(cuda, c, s):
    psum, _, w1, b1, w2, b2 = _problem(c, s, 1)
    mean = psum[:, :, 0].contiguous().to(cuda)
    d = [x.to(cuda) for x in (w1, b1, w2, b2)]
    got = ops.se_gate_psum(mean, 1, *d)                                                    # [N, C] is taken as [N, C, 1]
    assert torch.equal(ops.se_gate_psum(mean.unsqueeze(2).contiguous(), 1, *d), got)
    assert torch.equal(ops.se_scale(mean.view(N, c, 1, 1), *d), got)                       # the mean of one pixel is the pixel


def test_null_biases_through_se_scale(cuda):
    c, s = 65, 3
    psum, _, w1, _, w2, _ = _problem(c, s, 1)
    got = ops.se_scale(psum[:, :, 0].contiguous().view(N, c, 1, 1).to(cuda), w1.to(cuda), None, w2.to(cuda), None)
    err = float((got.cpu().double() - _want(psum, 1, w1, None, w2, None, F.silu)).abs().max())
    print(f"no bias: err {err:.2e}")
    assert err <= 1e-5
