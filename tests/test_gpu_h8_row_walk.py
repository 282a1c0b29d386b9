"""GPU: the shared row walk of the h8 data-movement kernels (h8_row_col / h8_row_grid, csrc/h8_common.h) where it can go wrong: a row that needs
more than one 256-column tile, the last tile partly filled, of more than one channel block.  avgpool3s2_h8 (W = 1030, test_gpu_avgpool_h8_bits.py)
and bilinear_upsample_h8 (1024 output columns, test_gpu_fpn_opt_h8.py) are there already; these are the other four kernels.  Inputs hold
fp16-representable values, N = 2, and the comparison is bit-exact except for ELU + 1, which keeps the bar of
test_last_depth_to_space_with_elu_plus_one (test_gpu_fpn_h8.py)."""
import pytest
import torch
import torch.nn.functional as F

from semanticlidarunc_amd import h8

pytestmark = pytest.mark.gpu


def _rand16(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half().float()


def test_maxpool_two_tiles_two_blocks(cuda):
    x = (-(_rand16(21, 2, 16, 3, 601).abs() + 0.5)).half().float()      # all negative: a zero pad tap would win every border maximum
    got = h8.maxpool3s2_h8(h8.to_h8(x.to(cuda)))
    assert tuple(got.shape) == (2, 2, 2, 301, 8)                 # 301 output columns: tiles of 256 and 45
    assert torch.equal(h8.from_h8(got).cpu(), F.max_pool2d(x, 3, 2, 1))


def test_space_to_depth_two_tiles_two_blocks_with_meta(cuda):
    m, f = 3, 2
    x = _rand16(22, 2, 16, 4, 604)
    meta = _rand16(23, 2, m, 4 * f, 604 * f, scale=30.0)
    xin = torch.cat([x[:, :-m], meta[:, :, ::f, ::f]], 1)       # nearest 1 / f down-sampling of meta in the last m channels
    y, y00 = h8.space_to_depth2_h8(h8.to_h8(x.to(cuda)), meta.to(cuda), 16, f, phase00=True)
    assert tuple(y.shape) == (2, 8, 2, 302, 8) and tuple(y00.shape) == (2, 2, 2, 302, 8)      # 302 output columns: 256 + 46
    y, y00 = h8.from_h8(y).cpu(), h8.from_h8(y00).cpu()
    for p in (0, 1):
        for q in (0, 1):
            assert torch.equal(y[:, (2 * p + q) * 16:(2 * p + q + 1) * 16], xin[:, :, p::2, q::2]), (p, q)
    assert torch.equal(y00, xin[:, :, ::2, ::2])


def test_depth_to_space_two_tiles_into_a_slice(cuda):
    s, cout = 2, 16                                              # 8 input blocks = s s Go with Go = 2
    y = _rand16(24, 2, s * s * cout, 2, 151)
    sentinel = torch.full((2, 3, 4, 302, 8), -7.0, dtype=torch.float16, device=cuda)
    out = sentinel.clone()
    h8.depth_to_space_h8(h8.to_h8(y.to(cuda)), s, out, 1)       # blocks [1, 3) of 3; 302 output columns: 256 + 46
    # channels ordered (i, j, cout): out[n, c, s h + i, s w + j] = y[n, (i s + j) cout + c, h, w]
    want = torch.empty(2, cout, 4, 302)
    for i in range(s):
        for j in range(s):
            want[:, :, i::s, j::s] = y[:, (i * s + j) * cout:(i * s + j + 1) * cout]
    assert torch.equal(h8.from_h8(out[:, 1:3].contiguous()).cpu(), want)
    assert torch.equal(out[:, 0], sentinel[:, 0])                # the block before the slice: untouched


def test_last_depth_to_space_with_elu_plus_one_two_tiles_three_blocks(cuda):
    classes = 5                                                  # 20 channels: 3 blocks, the last half pad; the walk is over 300 INPUT columns
    y = _rand16(25, 2, 4 * classes, 2, 300, scale=2.0)
    got = h8.depth_to_space_h8(h8.to_h8(y.to(cuda)), 2, elu_plus_one=True, classes=classes).cpu()
    want = F.elu(F.pixel_shuffle(y, 2)) + 1
    assert got.shape == want.shape and got.dtype == torch.float32
    assert float((got - want).abs().max()) <= 1e-6
