"""GPU: the kernels around the projection, each called directly and held to bit equality with numpy -- slu_kitti_decode (label mask, LUT
edges, unmapped-label count, the unfused fp64 yaw rotation), slu_range_image_split (float32 range in the reference's summation order,
channel split, C != 5) and slu_resize_nearest_hwc (index tables of oracle.kitti.resize_nearest, flip, the grid-stride loop's second
round).  The pipeline tests see them only behind a whole scan; here every block edge and every argument has its own case."""
import numpy as np
import pytest
import torch

from oracle import kitti as okitti
from semanticlidarunc_amd import ops

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------
# kitti_decode
# ---------------------------------------------------------------------------------------------------------------------
LUT_SIZE, HOLE = 40, 5


def _decode_inputs(n, seed):
    rs = np.random.default_rng(seed)
    lut = rs.integers(0, 20, LUT_SIZE).astype(np.int32)
    lut[HOLE] = -1
    xyzi = np.concatenate([rs.uniform(-60, 60, (n, 3)), rs.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    sem = rs.integers(0, LUT_SIZE, n).astype(np.uint32)
    sem[sem == HOLE] = HOLE + 1
    unmapped = {}
    if n == 1:
        unmapped = {0: LUT_SIZE}
    else:
        sem[0] = LUT_SIZE - 1                                               # the last entry is valid
        unmapped = {n - 1: LUT_SIZE, n // 2: HOLE}                          # one past the table; an entry of -1
        if n >= 1000:
            unmapped.update({3: HOLE, 300: 0xFFFF, 600: LUT_SIZE + 7, 601: HOLE})       # spread over four blocks
    for i, v in unmapped.items():
        sem[i] = v
    label = sem | (rs.integers(1, 0x10000, n).astype(np.uint32) << np.uint32(16))       # instance ids in the upper half: masked
    want_cls = np.where(np.isin(np.arange(n), list(unmapped)), 0, lut[np.minimum(sem, LUT_SIZE - 1)]).astype(np.float64)
    return xyzi, label, lut, want_cls, len(unmapped)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_kitti_decode(cuda, n):
    xyzi, label, lut, want_cls, n_bad = _decode_inputs(n, n)
    t_xyzi, t_label, t_lut = (torch.from_numpy(a).to(cuda) for a in (xyzi, label.view(np.int32), lut))
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    x, y, z = (xyzi[:, k].astype(np.float64) for k in range(3))
    calls = 0
    for angle in (None, 0, 90, -180, 37):
        got = ops.kitti_decode(t_xyzi, t_label, t_lut, bad, angle).cpu().numpy()
        calls += 1
        assert int(bad.item()) == calls * n_bad                            # exact, and accumulated over the calls
        assert got.shape == (n, 5) and got.dtype == np.float64
        assert np.array_equal(_bits(got[:, 2]), _bits(z)) and np.array_equal(_bits(got[:, 3]), _bits(xyzi[:, 3].astype(np.float64)))
        assert np.array_equal(got[:, 4], want_cls)
        if angle is None:                                                   # the float32 values widened, bit for bit
            assert np.array_equal(_bits(got[:, 0]), _bits(x)) and np.array_equal(_bits(got[:, 1]), _bits(y))
            continue
        a = np.radians(float(angle))
        c, s = np.cos(a), np.sin(a)
        # points @ [[c, -s, 0], [s, c, 0], [0, 0, 1]] written out: numpy's elementwise products and sums do not fuse
        want_x, want_y = (x * c + y * s) + z * 0.0, (x * (-s) + y * c) + z * 0.0
        assert np.array_equal(_bits(got[:, 0]), _bits(want_x)) and np.array_equal(_bits(got[:, 1]), _bits(want_y)), angle
        # the reference's np.dot goes through BLAS, which may fuse: 2 ulp of |x| + |y|
        ref = okitti.rotate_z(xyzi[:, :3].astype(np.float64), float(angle))
        bound = 2.0 * np.spacing(np.abs(x) + np.abs(y))
        assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= bound) and np.all(np.abs(got[:, 1] - ref[:, 1]) <= bound), angle
        assert np.array_equal(_bits(got[:, 2]), _bits(ref[:, 2]))


# ---------------------------------------------------------------------------------------------------------------------
# range_image_split
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("c", [5, 8])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 85), (16, 16), (5, 103)])
def test_range_image_split(cuda, h, w, c, with_normals):
    rs = np.random.default_rng(h * 1000 + w + c)
    img = rs.uniform(-50, 50, (h, w, c)).astype(np.float32)
    img[..., 4] = rs.integers(0, 260, (h, w))
    img[rs.random((h, w)) < 0.2] = 0.0                                     # empty pixels
    nrm = rs.normal(size=(h, w, 3)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    rng, refl = torch.full((1, h, w), 7.0, device=cuda), torch.full((1, h, w), 7.0, device=cuda)
    xyz, nout = torch.full((3, h, w), 7.0, device=cuda), torch.full((3, h, w), 7.0, device=cuda)
    lab = torch.full((1, h, w), 7, dtype=torch.int64, device=cuda)
    ops.range_image_split(dev(img), dev(nrm) if with_normals else None, rng, refl, xyz, nout, lab)
    x, y, z = img[..., 0], img[..., 1], img[..., 2]
    assert np.array_equal(_bits(rng.cpu().numpy()[0]), _bits(np.sqrt((x * x + y * y) + z * z)))            # float32, in that order
    assert np.array_equal(_bits(refl.cpu().numpy()[0]), _bits(img[..., 3]))
    assert np.array_equal(_bits(xyz.cpu().numpy()), _bits(img[..., :3].transpose(2, 0, 1)))
    assert np.array_equal(lab.cpu().numpy()[0], img[..., 4].astype(np.int64))
    want_n = nrm.transpose(2, 0, 1) if with_normals else np.full((3, h, w), 7.0, np.float32)             # untouched without normals
    assert np.array_equal(_bits(nout.cpu().numpy()), _bits(want_n))


# ---------------------------------------------------------------------------------------------------------------------
# resize_nearest_hwc
# ---------------------------------------------------------------------------------------------------------------------
def _coded(h, w, c):
    """Every element names its own (row, column, channel); exact in float32 (< 2^24), never 0 in channel 1."""
    r, q, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((r * 4096 + q) * 8 + k + 1).astype(np.float32)


def _flipped(img):
    out = img[:, ::-1].copy()
    out[..., 1] = -out[..., 1]
    return out


@pytest.mark.parametrize("c,flip", [(5, False), (5, True), (1, False), (2, True)])
@pytest.mark.parametrize("src,dst", [((3, 5), (7, 11)), ((7, 11), (3, 5)), ((7, 11), (7, 11)), ((1, 1), (4, 4)), ((4, 4), (1, 1)),
                                     ((32, 256), (128, 2048)), ((4, 6), (4, 34)), ((6, 4), (34, 4))])
def test_resize_nearest(cuda, src, dst, c, flip):
    img = _coded(src[0], src[1], c)
    want = okitti.resize_nearest(img, dst[0], dst[1])
    want = _flipped(want) if flip else want
    got = ops.resize_nearest_hwc(torch.from_numpy(img).to(cuda), dst[0], dst[1], flip=flip).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    if c == 1:
        with pytest.raises(RuntimeError):                                   # the flip negates channel 1
            ops.resize_nearest_hwc(torch.from_numpy(img).to(cuda), dst[0], dst[1], flip=True)


@pytest.mark.parametrize("flip", [False, True], ids=["asis", "flip"])
def test_resize_nearest_second_round_of_the_grid_stride_loop(cuda, flip):
    """2048 x 2048 x 5 outputs = 81 920 blocks' worth for a grid capped at 65 535: the only size at which the loop runs twice.  84 MB, so
    the comparison stays on the device, against a tensor built from the oracle's index tables."""
    h = w = 64
    oh = ow = 2048
    src = torch.from_numpy(_coded(h, w, 5)).to(cuda)
    assert (oh * ow * 5 + 255) // 256 > 65535
    ys = torch.from_numpy(np.minimum(np.floor(np.arange(oh) * (h / oh)).astype(np.int64), h - 1)).to(cuda)
    xs = np.minimum(np.floor(np.arange(ow) * (w / ow)).astype(np.int64), w - 1)
    xs = torch.from_numpy(xs[::-1].copy() if flip else xs).to(cuda)
    want = src[ys][:, xs]
    if flip:
        want[..., 1] = -want[..., 1]
    got = ops.resize_nearest_hwc(src, oh, ow, flip=flip)
    assert got.shape == (oh, ow, 5) and torch.equal(got, want)
    probe = okitti.resize_nearest(src.cpu().numpy(), oh, ow)[2040:]         # the oracle itself on the rows the second round writes
    assert np.array_equal(got[2040:].cpu().numpy(), _flipped(probe) if flip else probe)
