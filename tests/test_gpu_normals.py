"""GPU: surface normals of the projected image (dataset/utils.py:30-58) against the oracle -- on the golden
projection of the reference (a real projected cloud with empty pixels), on a full-size 64x2048 and 128x2048 image, on the
smallest sizes that have an interior and on sizes that have none (all-zero normals, exactly).  The kernel evaluates the same
float32 expressions in the same order without FMA contraction, so the bar is 2e-6 absolute on every component (division / sqrt
rounding), and the zero normals are the same pixels.
The oracle's Scharr is restated from OpenCV's definition (parity unpinned, see oracle/normals.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import normals as onorm
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.dataset.utils import build_normal_xyz

pytestmark = pytest.mark.gpu


def _check(xyz, got):
    want = onorm.build_normal_xyz(xyz)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got - want).max() <= 2e-6
    assert np.array_equal(got == 0, want == 0)                                  # parallel / vanishing tangents: the zero normal, exactly


def _surface(rs, h, w):
    el, az = np.meshgrid(np.linspace(0.05, -0.43, h), np.linspace(np.pi, -np.pi, w, endpoint=False), indexing="ij")
    rng_m = 20.0 + 5.0 * np.sin(3 * az) + rs.normal(0, 0.05, (h, w))
    return (rng_m[..., None] * np.dstack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])).astype(np.float32)


@pytest.mark.parametrize("h,w", [(3, 3), (3, 5), (4, 257), (5, 513)])
def test_small_images_with_an_interior(cuda, h, w):
    """The smallest sizes with an interior pixel, and columns on both sides of a 256-lane block edge: the oracle's bar, borders exactly 0
    (a border pixel has one vanishing tangent), and an interior that is not -- so the case cannot pass on zeros."""
    xyz = _surface(np.random.default_rng(h * 1000 + w), h, w)
    got = build_normal_xyz(xyz)
    _check(xyz, got)
    assert np.all(got[0] == 0) and np.all(got[-1] == 0) and np.all(got[:, 0] == 0) and np.all(got[:, -1] == 0)
    inner = np.linalg.norm(got[1:-1, 1:-1].astype(np.float64), axis=-1)
    assert inner.size > 0 and np.all(inner > 0.5)                                                # a normal in every interior pixel


@pytest.mark.parametrize("norm_factor", [1.0, 0.5])
def test_four_channels_and_other_norm_factors(cuda, norm_factor):
    """channels = 4 (the pixel stride differs from 3) and norm_factor != the default 0.25, against the oracle with the same factor."""
    rs = np.random.default_rng(11)
    xyz = _surface(rs, 6, 300)
    xyz[rs.random((6, 300)) < 0.1] = 0.0
    xyzi = np.concatenate([xyz, rs.uniform(1, 2, (6, 300, 1)).astype(np.float32)], -1)
    got = ops.build_normals(torch.from_numpy(xyzi).to(cuda), norm_factor).cpu().numpy()
    want = onorm.build_normal_xyz(xyz, norm_factor)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got - want).max() <= 2e-6 and np.array_equal(got == 0, want == 0)
    assert (np.linalg.norm(got[1:-1, 1:-1], axis=-1) > 0.5).mean() > 0.5


def test_normals_against_oracle(cuda):
    g = golden("spherical_projection_30000x5_32x256")
    _check(g["img:data_range"][..., :3], build_normal_xyz(g["img:data_range"][..., :3]))        # numpy in, numpy out (the reference's contract)
    rs = np.random.default_rng(3)
    for h, w in ((64, 2048), (128, 2048), (1, 7), (5, 1), (2, 2)):
        xyz = _surface(rs, h, w)
        if h * w > 100:
            xyz[rs.random((h, w)) < 0.1] = 0.0                                                   # empty returns
            _check(xyz, build_normal_xyz(xyz))
        else:       # every pixel is a border pixel: the derivative taps are antisymmetric under BORDER_REFLECT_101, so the normal is 0
            got = build_normal_xyz(xyz)
            assert got.shape == (h, w, 3) and got.dtype == np.float32 and np.all(got == 0) and np.all(onorm.build_normal_xyz(xyz) == 0)
    # a device tensor stays on the device; 4-channel images (x, y, z, intensity) read the first three
    t = torch.from_numpy(np.concatenate([xyz, np.ones((*xyz.shape[:2], 1), np.float32)], -1)).to(cuda)
    assert torch.equal(build_normal_xyz(t), ops.build_normals(t[..., :3].contiguous())) and build_normal_xyz(t).is_cuda
    with pytest.raises(RuntimeError):
        ops.build_normals(torch.zeros(4, 4, 2, device=cuda))
    with pytest.raises(RuntimeError):
        ops.build_normals(torch.zeros(4, 4, 3))                                                  # CPU tensor: no fallback
