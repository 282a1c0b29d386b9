"""GPU: avgpool3s2_h8 (csrc/layout_h8.hip) bit for bit against a CPU emulation of the kernel's own fp32 sequence on zero-padded
tensors: acc = +0.0, the nine taps added one after the other (rows -1 .. 1 outside, columns -1 .. 1 inside; a tap outside the image
is the pad's +0.0, which leaves acc as it is), then acc * s, then the true division by 9, then round to fp16.  Every step is one IEEE
fp32 operation (no contraction is possible between a multiply and a divide), so the emulation has one answer;
test_emulation_has_one_answer checks torch's element-wise ops against numpy's on the same inputs without a GPU.  Results are compared
as bit patterns, so a -0.0 where the kernel gives +0.0 counts as a difference."""
import numpy as np
import pytest
import torch

from semanticlidarunc_amd import h8

# (N, C, H, W): 2x2 (every tap row and column has a pad), odd H and W, W > 2 * 64 (two waves per row), several blocks per image, H = 1;
# the last: more than 256 output columns, so a row takes several workgroups of each of its 2 channel blocks
SHAPES = [(1, 8, 2, 2), (1, 8, 5, 33), (2, 24, 3, 130), (3, 64, 16, 64), (1, 8, 1, 7), (1, 16, 3, 1030)]
SCALES = ["none", "mask", "0.3"]


def _input(n, c, h, w, seed):
    """fp16-representable values: normal draws, with -0.0, 65504 (nine of them sum to 589 536, outside fp16, before the division) and
    runs of +-60000 / tiny values written over them."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, h, w, generator=g) * 3.0).half().float()
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)
    k = max(1, flat.numel() // 8)
    flat[idx[:k]] = -0.0
    flat[idx[k:2 * k]] = 65504.0
    flat[idx[2 * k:3 * k]] = -60000.0
    flat[idx[3 * k:4 * k]] = 2.0 ** -24                   # the smallest fp16 subnormal
    if h * w >= 9:
        x[0, 0] = 65504.0                                 # every full window of this plane sums to 589 536 and comes back to 65504
        x[0, 1] = -0.0                                    # and one plane of -0.0 only: +0.0 + -0.0 = +0.0
    return x


def _scale(kind, n, c, seed):
    if kind == "none":
        return None
    if kind == "0.3":
        return torch.full((n, c), 0.3)
    return (torch.rand(n, c, generator=torch.Generator().manual_seed(seed)) > 0.2).float() * 1.25


def _emulate(x, s):
    n, c, h, w = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    xp = torch.zeros(n, c, h + 2, w + 2)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    acc = torch.zeros(n, c, oh, ow)
    for i in range(3):
        for j in range(3):
            acc = acc + xp[:, :, i:i + 2 * oh - 1:2, j:j + 2 * ow - 1:2]
    if s is None:
        s = torch.ones(n, c)
    acc = acc * s[:, :, None, None]
    return (acc / torch.full_like(acc, 9.0)).half()


def _emulate_numpy(x, s):
    x = x.numpy()
    n, c, h, w = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((n, c, h + 2, w + 2), np.float32)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    acc = np.zeros((n, c, oh, ow), np.float32)
    for i in range(3):
        for j in range(3):
            acc = acc + xp[:, :, i:i + 2 * oh - 1:2, j:j + 2 * ow - 1:2]
    sv = np.ones((n, c), np.float32) if s is None else s.numpy()
    acc = (acc * sv[:, :, None, None]).astype(np.float32)
    with np.errstate(over="ignore"):
        return (acc / np.float32(9.0)).astype(np.float32).astype(np.float16)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_has_one_answer(shape):
    n, c, h, w = shape
    x = _input(n, c, h, w, seed=h * w + c)
    for kind in SCALES:
        s = _scale(kind, n, c, seed=n + c)
        a, b = _emulate(x, s), torch.from_numpy(_emulate_numpy(x, s))
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(_emulate(x.clone(), s)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_h8_bit_exact(cuda, shape, kind):
    n, c, h, w = shape
    x = _input(n, c, h, w, seed=h * w + c)
    s = _scale(kind, n, c, seed=n + c)
    got = h8.from_h8(h8.avgpool3s2_h8(h8.to_h8(x.to(cuda)), None if s is None else s.to(cuda)), c).cpu()
    want = _emulate(x, s)
    assert got.shape == want.shape
    assert torch.equal(_bits(got.half()), _bits(want)) and torch.equal(got, want.float())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SCALES)
def test_avgpool_h8_broadcast_bit_exact(cuda, kind):
    """n_out = 6 outputs over 2 shared images: the same bits as the plain call on the repeated input, and as the emulation."""
    x = _input(2, 24, 5, 130, seed=77)
    s = _scale(kind, 6, 24, seed=78)
    sd = None if s is None else s.to(cuda)
    got = h8.avgpool3s2_h8(h8.to_h8(x.to(cuda)), sd, 6)
    rep = h8.avgpool3s2_h8(h8.to_h8(x.repeat(3, 1, 1, 1).to(cuda)), sd)
    assert got.shape == rep.shape and torch.equal(_bits(got.cpu()), _bits(rep.cpu()))
    assert torch.equal(_bits(h8.from_h8(got, 24).cpu().half()), _bits(_emulate(x.repeat(3, 1, 1, 1), s)))
