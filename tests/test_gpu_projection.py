"""GPU: spherical projection against the reference's golden image and the oracle on a full-size scan.
The device evaluates atan2 / sqrt in fp64 like numpy; a last-bit difference could move only a point within a few ulps of pi of a
bin edge, and the closest point of either cloud is 4e-9 rad away (tests/test_projection_cases_cpu.py asserts it), so the bar is an
identical image.  Should a fixture ever gain an edge-near point, both sides get the cloud without it (projection_cases.drop_edge_near)."""
import numpy as np
import pytest
import torch

import projection_cases as pc
from conftest import golden
from oracle import projection as oproj
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.dataset.utils import spherical_projection

pytestmark = pytest.mark.gpu


def test_against_reference_golden(cuda):
    g = golden("spherical_projection_30000x5_32x256")
    g_cloud = g["cloud"]
    for tag, tr in (("data_range", None), ("fixed_range", [-np.pi / 8, np.pi / 8])):
        assert pc.drop_edge_near(g_cloud, 32, 256, tr) is g_cloud                 # the golden image was written from the whole cloud
        img, alpha, th, ph = spherical_projection(g_cloud, 32, 256, theta_range=tr)
        assert img.dtype == np.float32 and img.shape == (32, 256, 5)
        assert np.allclose(np.asarray(th, dtype=np.float64), g["theta_range:" + tag], rtol=0, atol=1e-15)
        diff = np.any(img != g["img:" + tag], axis=-1)
        assert not diff.any(), (tag, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert alpha.shape == (32, 256) and ph == (-np.pi, np.pi)
    far, _, _, _ = spherical_projection(g_cloud, 32, 256, sort_largest_first=True)         # ascending write order: the FARTHEST point survives
    assert np.array_equal(far, pc.image(g_cloud, pc.winners(g_cloud, 32, 256, keep_farthest=True)))
    near = g["img:data_range"]
    rf, rn = np.linalg.norm(far[..., :3], axis=-1), np.linalg.norm(near[..., :3], axis=-1)
    assert np.all(rf >= rn - 1e-4) and (rf > rn + 1e-3).mean() > 0.05 and np.array_equal(rf > 0, rn > 0)
    with pytest.raises(RuntimeError):
        ops.spherical_projection(torch.zeros(10, 2, dtype=torch.float64, device=cuda), 4, 8)


def test_full_size_scan_against_oracle(cuda):
    cloud = pc.drop_edge_near(pc.full_size_scan(), 64, 2048)                    # 123 457 points, none dropped
    assert cloud.shape == (123_457, 5)
    want, _, th_w, _ = oproj.spherical_projection(cloud, 64, 2048)
    img, tr = ops.spherical_projection(torch.from_numpy(cloud).to(cuda), 64, 2048)
    assert np.allclose(tr.cpu().numpy(), np.asarray(th_w), rtol=0, atol=1e-15)
    got = img.cpu().numpy()
    diff = np.any(got != want, axis=-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(got[..., 0] != 0, want[..., 0] != 0)                  # the same pixels are occupied
