"""GPU: slu_spherical_projection_ex held to ``==`` on constructed clouds (tests/projection_cases.py): interior grids, the +-pi seam and
phi = 0, the theta-extreme rows, theta = 0 on a row edge, degenerate ranges, equal ranges, theta extremes only the grid-stride loop
of theta_minmax_kernel visits -- each also flipped -- and stale output / workspace memory.

No pixel fraction and no value tolerance: no point of these clouds is within 2^-40 rad of a bin edge except those placed on one with
an exactly representable angle (tests/test_projection_cases_cpu.py asserts it, and that each fault of its teeth table changes the
reference image of one of these cases).  theta_range is compared at 1e-15 as in test_gpu_projection.py.  Channel 3 of every cloud with
C >= 4 is the point index, so a failure names the point that won."""
import numpy as np
import pytest
import torch

import projection_cases as pc
from oracle import projection as oproj
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.dataset import utils as dutils

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in pc.constructed_cases()]


def _project(c, cuda, flip=False, out=None):
    bins = None if c.bins_h is None else torch.from_numpy(np.ascontiguousarray(c.bins_h)).to(cuda)
    increasing = c.bins_h is not None and c.bins_h.size > 1 and c.bins_h[-1] > c.bins_h[0]
    img, tr = ops.spherical_projection(torch.from_numpy(c.cloud).to(cuda), c.H, c.W, c.theta_range, bins_h=bins, bins_increasing=bool(increasing),
                                       keep_farthest=c.keep_farthest, flip=flip, out=out)
    return img.cpu().numpy(), tr.cpu().numpy()


def _assert_same_image(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = np.argwhere(np.any(got != want, axis=-1))
    if bad.size:
        y, x = bad[0]
        who = (got[y, x, 3], want[y, x, 3]) if got.shape[2] >= 4 else (got[y, x].tolist(), want[y, x].tolist())
        raise AssertionError(f"{name}: {len(bad)} pixel(s) differ; first (row {y}, column {x}): point {who[0]} on the device, {who[1]} expected")


@pytest.mark.parametrize("flip", [False, True], ids=["asis", "flip"])
@pytest.mark.parametrize("name", NAMES)
def test_image_is_exact(cuda, name, flip):
    c = pc.case(name)
    pc.check_preconditions(c)
    want, win, tr_want = pc.expected(name, flip)
    got, tr = _project(c, cuda, flip)
    assert np.allclose(tr, np.asarray(tr_want, dtype=np.float64), rtol=0, atol=1e-15), (tr, tr_want)
    _assert_same_image(got, want, name)


def test_out_tensor_full_of_nan_comes_back_with_zero_empty_pixels(cuda):
    for name in ("interior 8x64 C5 n1500 decreasing bins_h", "seam W=23", "degenerate: one point, farthest"):
        c = pc.case(name)
        for flip in (False, True):
            want, win, _ = pc.expected(name, flip)
            out = torch.full((c.H, c.W, c.cloud.shape[1]), float("nan"), dtype=torch.float32, device=cuda)
            got, _ = _project(c, cuda, flip, out=out)
            assert (win < 0).any() and not np.isnan(got).any()
            _assert_same_image(got, want, name)
            assert np.array_equal(out.cpu().numpy(), got)


def test_second_call_holds_no_survivor_of_the_first(cuda):
    """A dense cloud, then a sparse one of the same N, H and W: the allocator hands the second call the first call's workspace and image."""
    dense = pc.case("interior 8x64 C5 n1500 decreasing bins_h")
    n = dense.cloud.shape[0]
    sparse_xyz = dense.cloud[:, :3].copy()
    sparse_xyz[:] = sparse_xyz[np.arange(n) % 7]                            # 7 distinct points, each many times: at most 7 pixels occupied
    sparse_xyz *= (1.0 + np.arange(n) / n)[:, None]                         # distinct ranges, same angles up to rounding
    sparse = pc.Case("sparse", pc._finish(sparse_xyz, 5, np.random.default_rng(0)), dense.H, dense.W, None, dense.bins_h, False)
    pc.check_preconditions(sparse)
    for far in (False, True):
        a, b = dense._replace(keep_farthest=far), sparse._replace(keep_farthest=far)
        want_b = pc.image(b.cloud, pc.winners(b.cloud, b.H, b.W, bins_h=b.bins_h, keep_farthest=far))
        got_a, _ = _project(a, cuda)
        got_b, _ = _project(b, cuda)
        assert (np.any(got_a != 0, -1)).sum() > 100 and (np.any(want_b != 0, -1)).sum() <= 7
        _assert_same_image(got_b, want_b, f"sparse after dense, farthest={far}")


@pytest.mark.parametrize("name", ["interior 5x23 C5 n257 data range", "interior 8x64 C5 n1500 decreasing bins_h", "interior 7x1 C7 n15 increasing bins_h",
                                  "interior 5x23 C3 n257 fixed range, farthest", "row edges: theta 0 on increasing bins_h"])
def test_wrapper_returns_the_reference_tuple(cuda, name):
    """dataset.utils.spherical_projection: image exact, alpha to 1e-14 (numpy on both sides, bins from a theta range equal to 1e-15),
    (theta_min, theta_max) and (phi_min, phi_max) as the reference returns them -- the data range in bins_h mode, the given one otherwise."""
    c = pc.case(name)
    want, alpha_w, th_w, ph_w = oproj.spherical_projection(c.cloud, c.H, c.W, theta_range=c.theta_range, sort_largest_first=c.keep_farthest, bins_h=c.bins_h)
    img, alpha, th, ph = dutils.spherical_projection(c.cloud, c.H, c.W, theta_range=c.theta_range, sort_largest_first=c.keep_farthest, bins_h=c.bins_h)
    _assert_same_image(img, pc.expected(name)[0], name)
    _assert_same_image(img, want, name)                                     # tie-free: the oracle agrees with the per-pixel reference
    assert alpha.shape == alpha_w.shape == (c.H, c.W) and alpha.dtype == np.float64
    assert np.abs(alpha - alpha_w).max() <= 1e-14
    assert len(th) == 2 and np.allclose(np.asarray(th, dtype=np.float64), np.asarray(th_w, dtype=np.float64), rtol=0, atol=1e-15)
    if c.theta_range is not None:
        assert tuple(th) == tuple(c.theta_range)
    assert ph == ph_w == (-np.pi, np.pi)
