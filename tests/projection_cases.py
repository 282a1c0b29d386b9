"""Test helpers for the range-image input kernels (csrc/projection.hip): an independent per-pixel reference of the spherical
projection, the input preconditions under which a device image may be compared with ``==``, the mutations the constructed cases
must catch, and the constructed cases themselves.  Plain numpy, no GPU; ``tests/test_projection_cases_cpu.py`` pins it to
``oracle.projection`` and ``tests/test_gpu_projection_exact.py`` holds the kernel to it.

Why ``==``: the device evaluates atan2 / sqrt in fp64 like numpy.  Two correctly written fp64 math libraries differ by a few ulps of
pi (about 1e-15 rad), so a point can change its pixel only if it lies that close to a bin edge.  ``edge_report`` measures the
distance of every point to its nearest row and column edge; an input whose closest point is further than EPS = 2^-40 rad (9e-13,
more than 2000 ulps of pi; a 1-ulp theta_min / theta_max moves an edge by about an ulp as well) away is entitled to no differing
pixel.  Points put on an edge on purpose have exactly representable angles (phi = 0, +-pi; theta = 0; the theta extremes
themselves), where both libraries return the same double.

``winners`` shares the angles and ``np.digitize`` with the oracle and nothing else: the survivor of a pixel is found by one scan
over the points (no argsort, no fancy-index assignment).  Nearest mode keeps the minimum range and among equal ranges the smallest
index, farthest mode the maximum range and the largest index -- what a stable sort in the reference's write order yields, and what
``winner_kernel`` documents.
"""
from __future__ import annotations

import functools
from fractions import Fraction
from typing import NamedTuple, Optional, Tuple

import numpy as np

from oracle import projection as oproj

EPS = 2.0 ** -40
STRIDE = 65536                  # lanes of theta_minmax_kernel's grid: 256 blocks of 256

MUTATIONS = ("ge_to_gt_decreasing", "le_to_lt_increasing", "clamp_minus_one", "tie_other_index", "swap_nearest_farthest",
             "fused_linspace", "fused_sum_of_squares", "extremes_first_stride_only", "flip_without_y_negation", "flip_rows")


# ---------------------------------------------------------------------------------------------------------------------
# angles, bins, pixels
# ---------------------------------------------------------------------------------------------------------------------
def angles(cloud):
    """(phi, theta, r) in fp64 as the oracle computes them."""
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    phi, theta = oproj.deflection(x, y, z)
    return phi, theta, np.sqrt(x ** 2 + y ** 2 + z ** 2)


def _fused_range(cloud):
    """r = sqrt(fma(z, z, fma(x, x, y * y))): what a compiler that contracts (x^2 + y^2) + z^2 evaluates, in exact rational arithmetic."""
    out = []
    for x, y, z in cloud[:, :3].tolist():
        xy = float(Fraction(x) * Fraction(x) + Fraction(y * y))
        out.append(float(Fraction(z) * Fraction(z) + Fraction(xy)))
    return np.sqrt(np.array(out))


def _fused_linspace(start, stop, n):
    """linspace whose samples are i * step + start rounded ONCE (a fused multiply-add), in exact rational arithmetic."""
    if n == 1:
        return np.array([float(start)])
    step = (float(stop) - float(start)) / (n - 1)
    out = [float(Fraction(i) * Fraction(step) + Fraction(float(start))) for i in range(n)]
    out[-1] = float(stop)
    return np.array(out)


def _linspace(start, stop, n, mutation):
    return _fused_linspace(start, stop, n) if mutation == "fused_linspace" else np.linspace(start, stop, n)


def theta_extremes(theta, mutation=None):
    t = theta[:STRIDE] if mutation == "extremes_first_stride_only" else theta
    return t.min(), t.max()


def row_bins(theta, H, theta_range=None, bins_h=None, mutation=None):
    if bins_h is not None:
        return np.asarray(bins_h, dtype=np.float64)
    lo, hi = theta_extremes(theta, mutation) if theta_range is None else theta_range
    return _linspace(lo, hi, H, mutation)[::-1]


def col_bins(W, mutation=None):
    return _linspace(-np.pi, np.pi, W, mutation)[::-1]


def _digitize(v, bins, mutation):
    increasing = bins.size > 1 and bins[-1] > bins[0]
    right = (mutation == "le_to_lt_increasing" and increasing) or (mutation == "ge_to_gt_decreasing" and not increasing)
    idx = np.digitize(v, bins, right=bool(right)) - 1
    if mutation == "clamp_minus_one":
        return np.where(idx < 0, 0, idx)
    return np.where(idx < 0, idx + bins.size, idx)          # -1 is numpy's negative index: the last row / column


def pixels(cloud, H, W, theta_range=None, bins_h=None, mutation=None):
    phi, theta, r = angles(cloud)
    rows = _digitize(theta, row_bins(theta, H, theta_range, bins_h, mutation), mutation)
    cols = _digitize(phi, col_bins(W, mutation), mutation)
    return rows, cols, _fused_range(cloud) if mutation == "fused_sum_of_squares" else r


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def winners(cloud, H, W, theta_range=None, bins_h=None, keep_farthest=False, mutation=None):
    """int64 [H, W]: index of the surviving point of every pixel, -1 where no point fell."""
    rows, cols, r = pixels(cloud, H, W, theta_range, bins_h, mutation)
    if mutation == "swap_nearest_farthest":
        keep_farthest = not keep_farthest
    later_wins_tie = keep_farthest != (mutation == "tie_other_index")
    win = [-1] * (H * W)
    best = [0.0] * (H * W)
    for i, (px, ri) in enumerate(zip((rows * W + cols).tolist(), r.tolist())):        # ascending index
        if win[px] < 0:
            better = True
        elif ri == best[px]:
            better = later_wins_tie
        else:
            better = ri > best[px] if keep_farthest else ri < best[px]
        if better:
            win[px], best[px] = i, ri
    return np.array(win, dtype=np.int64).reshape(H, W)


def image(cloud, win, flip=False, mutation=None):
    """float32 [H, W, C]: the winner's channels, zeros in empty pixels; flip = columns reversed, y negated."""
    img = np.where((win >= 0)[..., None], cloud[np.maximum(win, 0)], 0.0).astype(np.float32)
    if flip:
        img = img[::-1] if mutation == "flip_rows" else img[:, ::-1]
        img = img.copy()
        if mutation != "flip_without_y_negation":
            img[..., 1] = -img[..., 1]
    return img


# ---------------------------------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------------------------------
class EdgeReport(NamedTuple):
    near: np.ndarray            # indices of points within eps of a row or column edge (exempt points left out)
    row_dist: float             # distance of the closest non-exempt point to a row edge, rad
    col_dist: float             # ... to a column edge
    extreme_sep: float          # data-range mode: distance of the theta extremes to the next theta (inf otherwise)
    tie_pixels: np.ndarray      # flat indices of pixels that hold two points of equal range


def _edge_distance(v, bins):
    b = np.sort(bins)
    k = np.clip(np.searchsorted(b, v), 1, b.size - 1) if b.size > 1 else np.zeros(v.shape, dtype=np.int64)
    lo = b[k - 1] if b.size > 1 else b[k]
    return np.minimum(np.abs(v - lo), np.abs(v - b[k]))


def edge_report(cloud, H, W, theta_range=None, bins_h=None, eps=EPS, exempt=()):
    """Raises ValueError when the bins themselves are not robust: data-range mode with a theta extreme that is shared by, or within
    eps of, another point (points listed in `exempt` -- placed on purpose -- may share it)."""
    phi, theta, r = angles(cloud)
    n = theta.size
    skip = np.zeros(n, dtype=bool)
    skip[np.asarray(list(exempt), dtype=np.int64)] = True
    sep = np.inf
    if theta_range is None and bins_h is None:
        lo, hi = theta.min(), theta.max()
        at_end = (theta == lo) | (theta == hi)
        for end, name in ((lo, "theta_min"), (hi, "theta_max")):
            idx = np.flatnonzero(theta == end)
            if idx.size > 1 and not skip[idx].all():
                raise ValueError(f"{name} is shared by points {idx.tolist()}")
        rest = theta[~at_end]
        if rest.size:
            sep = float(min(rest.min() - lo, hi - rest.max()))
            if not sep > eps:
                raise ValueError(f"a theta extreme is within {sep} rad of the next theta")
        elif not skip.all():
            raise ValueError("all points share one theta")
        skip = skip | at_end                                # each extreme sits on an edge by construction, on both sides
    d_row = _edge_distance(theta, row_bins(theta, H, theta_range, bins_h))
    d_col = _edge_distance(phi, col_bins(W))
    keep = ~skip
    near = np.flatnonzero(keep & ((d_row <= eps) | (d_col <= eps)))
    rows, cols, _ = pixels(cloud, H, W, theta_range, bins_h)
    px = rows * W + cols
    order = np.lexsort((r, px))
    same = (px[order][1:] == px[order][:-1]) & (r[order][1:] == r[order][:-1])
    return EdgeReport(near, float(d_row[keep].min()) if keep.any() else np.inf, float(d_col[keep].min()) if keep.any() else np.inf,
                      sep, np.unique(px[order][1:][same]))


def drop_edge_near(cloud, H, W, theta_range=None, bins_h=None, eps=EPS, max_share=1e-4):
    """The cloud both sides of an exact comparison receive: edge-near points removed, at most `max_share` of them."""
    rep = edge_report(cloud, H, W, theta_range, bins_h, eps)
    if rep.near.size > max_share * cloud.shape[0]:
        raise ValueError(f"{rep.near.size} of {cloud.shape[0]} points are within {eps} rad of a bin edge")
    return np.delete(cloud, rep.near, axis=0) if rep.near.size else cloud


# ---------------------------------------------------------------------------------------------------------------------
# fixtures of the existing tests
# ---------------------------------------------------------------------------------------------------------------------
def full_size_scan():
    """The seed-5 scan of tests/test_gpu_projection.py: 123 457 points for a 64 x 2048 image."""
    rs = np.random.default_rng(5)
    n = 123_457
    az, el, r = rs.uniform(-np.pi, np.pi, n), rs.uniform(-0.43, 0.05, n), rs.uniform(1.0, 90.0, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)
    return np.concatenate([xyz, rs.uniform(0, 1, (n, 1)).astype(np.float32), rs.integers(0, 20, (n, 1))], axis=-1)


def kitti_cloud(g, id_map, angle=None):
    from oracle import kitti as okitti
    cloud = okitti.decode(g["xyzi"].tobytes(), g["label"].tobytes(), id_map)
    if angle is not None:
        cloud[:, 0:3] = okitti.rotate_z(cloud[:, 0:3].reshape(-1, 3), float(angle))
    return cloud


def fixtures(golden, id_map):
    """(name, cloud, H, W, theta_range, bins_h) of every cloud the pre-existing projection / pipeline tests project."""
    g, k = golden("spherical_projection_30000x5_32x256"), golden("kitti_sample_16000_32x256")
    out = [("golden data range", g["cloud"], 32, 256, None, None),
           ("golden fixed range", g["cloud"], 32, 256, (-np.pi / 8, np.pi / 8), None)]
    for tag in ("plain", "rot", "rotflip"):
        a = float(k[f"{tag}:angle"])
        out.append((f"kitti {tag}", kitti_cloud(k, id_map, None if np.isnan(a) else a), 32, 256, None, None))
    out.append(("kitti beams", kitti_cloud(k, id_map), 32, 256, None, k["beams"]))
    out.append(("kitti beams increasing, range given", kitti_cloud(k, id_map), 32, 256, (-0.45, 0.05), k["beams"][::-1].copy()))
    out.append(("seed-5 scan", full_size_scan(), 64, 2048, None, None))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# constructed cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cloud: np.ndarray
    H: int
    W: int
    theta_range: Optional[Tuple[float, float]] = None
    bins_h: Optional[np.ndarray] = None
    keep_farthest: bool = False
    placed: Tuple[int, ...] = ()            # points put on an edge on purpose (exactly representable angles)
    ties: bool = False                      # the case is about equal ranges

    @property
    def kw(self):
        return dict(theta_range=self.theta_range, bins_h=self.bins_h)


def _xyz(phi, theta, r):
    return np.stack([r * np.cos(theta) * np.cos(phi), r * np.cos(theta) * np.sin(phi), r * np.sin(theta)], axis=-1)


def _finish(xyz, C, rs):
    """[N, C] float64: x, y, z, then (C >= 4) the point index, then values float32 has to round."""
    n = xyz.shape[0]
    extra = [np.arange(n, dtype=np.float64)[:, None]] if C >= 4 else []
    if C > 4:
        extra.append(rs.uniform(-3.0, 3.0, (n, C - 4)))
    return np.ascontiguousarray(np.concatenate([xyz] + extra, axis=1))


def _centres(edges):
    e = np.sort(np.asarray(edges, dtype=np.float64))
    return (e[:-1] + e[1:]) / 2, np.diff(e)


def _interior(name, H, W, C, n, seed, mode, keep_farthest=False):
    """Points at bin centres + up to 0.35 of a bin, 1 to 4 per pixel with distinct ranges, some pixels empty."""
    rs = np.random.default_rng(seed)
    lo, hi = -0.42, 0.07
    bins_h = None
    if mode in ("bins_decreasing", "bins_increasing"):
        inc = np.cumsum(rs.uniform(0.5, 1.5, H))                                  # uneven beams from lo to hi
        inc = lo + (inc - inc[0]) / (inc[-1] - inc[0]) * (hi - lo) if H > 1 else np.array([lo])
        bins_h = inc.copy() if mode == "bins_increasing" else inc[::-1].copy()
    row_c, row_w = _centres(bins_h if bins_h is not None else np.linspace(lo, hi, H)) if H > 1 else (np.array([-0.2]), np.array([0.3]))
    col_c, col_w = _centres(np.linspace(-np.pi, np.pi, W)) if W > 1 else (np.array([0.3]), np.array([3.0]))
    cells = [(a, b) for a in range(row_c.size) for b in range(col_c.size)]
    ends = 2 if mode == "data_range" and H > 1 else 0
    n = min(n, 4 * len(cells) + ends)
    take = rs.permutation(np.repeat(np.arange(len(cells)), 4))[:n - ends]           # up to 4 points per pixel, some pixels none
    a, b = np.array([cells[t][0] for t in take]), np.array([cells[t][1] for t in take])
    theta = row_c[a] + rs.uniform(-0.35, 0.35, take.size) * row_w[a]
    phi = col_c[b] + rs.uniform(-0.35, 0.35, take.size) * col_w[b]
    if ends:                                # the two points that define the data range
        theta, phi = np.concatenate([theta, [hi, lo]]), np.concatenate([phi, rs.uniform(-3.0, 3.0, 2)])
        p = rs.permutation(theta.size)
        theta, phi = theta[p], phi[p]
    r = rs.permutation(np.linspace(2.0, 60.0, theta.size))
    return Case(name, _finish(_xyz(phi, theta, r), C, rs), H, W, (lo, hi) if mode == "fixed_range" else None, bins_h, keep_farthest)


def _seam(W):
    """phi = +pi, -pi and 0 exactly, three rows each, among interior points."""
    rs = np.random.default_rng(W)
    H, tr = 5, (-0.5, 0.5)
    base = _interior("", H, W, 5, 200, 1000 + W, "fixed_range").cloud[:, :3]
    z = np.array([-2.0, 0.7, 3.0])
    pts = np.concatenate([np.stack([np.full(3, -9.0), np.full(3, 0.0), z], 1), np.stack([np.full(3, -11.0), np.full(3, -0.0), z], 1),
                          np.stack([np.full(3, 10.0), np.full(3, 0.0), z], 1), np.stack([np.full(3, 12.0), np.full(3, -0.0), z], 1)])
    at = rs.choice(base.shape[0] + 12, 12, replace=False)
    xyz = np.empty((base.shape[0] + 12, 3))
    mask = np.zeros(xyz.shape[0], dtype=bool)
    mask[at] = True
    xyz[mask], xyz[~mask] = pts, base
    return Case(f"seam W={W}", _finish(xyz, 5, rs), H, W, tr, None, False, tuple(np.flatnonzero(mask).tolist()))


def _row_edge_cases():
    rs = np.random.default_rng(77)
    out = []
    # data range: the unique max-theta point wraps to row H-1 (nothing else there), the unique min-theta point lands in row H-2
    out.append(_interior("row edges: data range extremes", 6, 17, 5, 120, 31, "data_range"))
    # theta = 0 exactly (z = 0) on the middle edge of a symmetric range with odd H, and on a 0.0 of explicit bins in either order
    phi = rs.uniform(-3.1, 3.1, 24)
    ring = np.stack([7.0 * np.cos(phi), 7.0 * np.sin(phi), np.zeros(24)], 1) * rs.uniform(0.5, 3.0, (24, 1))
    fill = _interior("", 5, 12, 5, 60, 32, "fixed_range").cloud[:, :3]
    xyz = np.concatenate([fill[:30], ring, fill[30:]])
    placed = tuple(range(30, 54))
    out.append(Case("row edges: theta 0 on the middle edge", _finish(xyz, 5, rs), 5, 12, (-0.4, 0.4), None, False, placed))
    bins = np.array([0.3, 0.1, 0.0, -0.15, -0.4])
    out.append(Case("row edges: theta 0 on decreasing bins_h", _finish(xyz, 6, rs), 5, 12, None, bins, False, placed))
    out.append(Case("row edges: theta 0 on increasing bins_h", _finish(xyz, 6, rs), 5, 12, None, bins[::-1].copy(), True, placed))
    # fixed range narrower than the data: points above theta_max and below theta_min share the last row
    wide = _interior("", 9, 12, 5, 150, 33, "fixed_range")
    out.append(Case("row edges: outside a fixed range", wide.cloud, 5, 12, (-0.2, -0.05), None, False))
    out.append(Case("row edges: outside a fixed range, farthest", wide.cloud, 5, 12, (-0.2, -0.05), None, True))
    return out


def _degenerate_cases():
    rs = np.random.default_rng(78)
    out = []
    for far in (False, True):
        tag = ", farthest" if far else ""
        out.append(Case("degenerate: one point" + tag, _finish(np.array([[3.0, -2.0, 0.5]]), 5, rs), 4, 9, None, None, far, (0,)))
        # p = 5 exactly for every point: one theta, theta_min == theta_max, all row bins equal
        one = np.array([[3.0, 4.0, 1.5], [4.0, 3.0, 1.5], [-3.0, 4.0, 1.5], [5.0, 0.0, 1.5], [0.0, -5.0, 1.5], [-4.0, -3.0, 1.5], [-5.0, 0.0, 1.5],
                        [3.0, -4.0, 1.5], [0.0, 5.0, 1.5]])
        out.append(Case("degenerate: one elevation" + tag, _finish(one, 5, rs), 4, 9, None, None, far, tuple(range(9)), True))
        # empty returns (0, 0, 0): r = 0, phi = 0, theta = pi / 2 = theta_max; farthest mode starts its best range at 0
        fill = _interior("", 4, 9, 5, 40, 34, "fixed_range").cloud[:, :3]
        xyz = np.concatenate([fill[:7], np.zeros((1, 3)), fill[7:20], [[2.0, 0.0, 1.0]], fill[20:]])
        out.append(Case("degenerate: one empty return" + tag, _finish(xyz, 5, rs), 4, 9, None, None, far, (7, 21)))
        xyz = np.concatenate([fill[:7], np.zeros((1, 3)), fill[7:20], np.zeros((2, 3)), [[2.0, 0.0, 1.0]], fill[20:]])
        out.append(Case("degenerate: three empty returns" + tag, _finish(xyz, 5, rs), 4, 9, None, None, far, (7, 21, 22, 23), True))
        out.append(Case("degenerate: empty returns, fixed range" + tag, _finish(xyz, 5, rs), 4, 9, (-0.42, 0.07), None, far, (7, 21, 22, 23), True))
    return out


def _tie_cases():
    """Bit-equal ranges in one pixel: squares of small integers sum exactly, so every permutation of (1, 2, 3) has r = sqrt(14).
    H = 2, W = 3 and the range +-1.5: y > 0 is column 0, y < 0 column 1, every theta used here row 0."""
    rs = np.random.default_rng(79)
    out = []
    five = [[1, 2, 3], [2, 1, 3], [3, 1, 2], [1, 3, 2], [2, 3, 1]]              # column 0: 5 points at sqrt(14)
    two = [[-1, -2, 3], [-2, -1, 3]]                                           # column 1: 2 points at sqrt(14)
    near, far = [[0.5, 1, 1], [0.5, -1, 1]], [[4, 8, 6], [4, -8, 6]]
    for keep in (False, True):
        tag = ", farthest" if keep else ""
        # the tied points hold the winning range of their pixel in either mode: the others are farther (nearest) / nearer (farthest)
        others = far if not keep else near
        xyz = np.array([others[0]] + five[:2] + [others[1]] + two[:1] + five[2:] + two[1:], dtype=np.float64)
        out.append(Case("ties: 5 and 2 permuted points" + tag, _finish(xyz, 6, rs), 2, 3, (-1.5, 1.5), None, keep, (), True))
        # candidates in different 256-lane blocks: indices 3, 300 and 600 (3-way), 255 and 256 (2-way, across one block edge)
        fill = np.array(others * 305, dtype=np.float64) * rs.uniform(1.0, 1.3, (610, 1)) if not keep else \
            np.array(others * 305, dtype=np.float64) * rs.uniform(0.7, 1.0, (610, 1))
        xyz = fill.copy()
        xyz[[3, 300, 600]] = [[3, 2, 1], [2, 3, 1], [1, 3, 2]]
        xyz[[255, 256]] = [[-3, -2, 1], [-2, -3, 1]]
        out.append(Case("ties: candidates in different blocks" + tag, _finish(xyz, 5, rs), 2, 3, (-1.5, 1.5), None, keep, (), True))
        # coordinates that are no small integers: (x, y, z) and (y, x, z) have bit-equal ranges only if x^2 + y^2 is summed without a
        # fused multiply-add (fma(x, x, y * y) != fma(y, y, x * x) for one pair in ten).  W = 64 has +-pi/4 and +-3pi/4 inside a column,
        # so 128 pairs mirrored at those diagonals -- 4 quadrants x 32 rows -- share a pixel each, in random index order, with a loser
        q, row = np.arange(128) % 4, np.arange(128) // 4
        d, p = rs.uniform(0.001, 0.008, 128), rs.uniform(3.0, 9.0, 128)
        a, b = p * np.cos(np.pi / 4 + d), p * np.sin(np.pi / 4 + d)
        z = p * np.tan(_centres(np.linspace(-1.2, 1.2, 33))[0][row] + rs.uniform(-0.01, 0.01, 128))
        sx, sy = np.array([1.0, -1.0, -1.0, 1.0])[q], np.array([1.0, 1.0, -1.0, -1.0])[q]
        swap = sx * sy                                   # quadrants 2 and 4: (x, y) -> (-y, -x) stays in the quadrant
        first, second = np.stack([sx * a, sy * b, z], 1), np.stack([swap * sy * b, swap * sx * a, z], 1)
        loser = first * (0.8 if keep else 1.3)
        xyz = np.concatenate([first, second, loser])[rs.permutation(384)]
        out.append(Case("ties: swapped generic coordinates" + tag, _finish(xyz, 5, rs), 33, 64, (-1.2, 1.2), None, keep, (), True))
    return out


def _late(name, n, first_late, seed, keep_farthest=False):
    """Both theta extremes at indices >= first_late: only theta_minmax_kernel's grid-stride loop visits them."""
    rs = np.random.default_rng(seed)
    theta, phi = rs.uniform(-0.40, 0.05, n), rs.uniform(-np.pi, np.pi, n)
    theta[first_late + 1], theta[n - 1] = 0.07, -0.42
    return Case(name, _finish(_xyz(phi, theta, rs.uniform(2.0, 80.0, n)), 4, rs), 8, 64, None, None, keep_farthest)


@functools.lru_cache(maxsize=None)
def constructed_cases():
    cases = [
        _interior("interior 5x23 C5 n257 data range", 5, 23, 5, 257, 1, "data_range"),
        _interior("interior 5x23 C3 n257 fixed range, farthest", 5, 23, 3, 257, 2, "fixed_range", True),
        _interior("interior 8x64 C7 n256 data range, farthest", 8, 64, 7, 256, 3, "data_range", True),
        _interior("interior 8x64 C5 n1500 decreasing bins_h", 8, 64, 5, 1500, 4, "bins_decreasing"),
        _interior("interior 8x64 C3 n255 increasing bins_h, farthest", 8, 64, 3, 255, 5, "bins_increasing", True),
        _interior("interior 3x3 C5 n12 data range", 3, 3, 5, 12, 6, "data_range"),
        _interior("interior 3x3 C7 n16 fixed range, farthest", 3, 3, 7, 16, 7, "fixed_range", True),
        _interior("interior 1x9 C5 n20 data range", 1, 9, 5, 20, 8, "data_range"),
        _interior("interior 1x9 C3 n20 fixed range, farthest", 1, 9, 3, 20, 9, "fixed_range", True),
        _interior("interior 7x1 C5 n15 data range", 7, 1, 5, 15, 10, "data_range"),
        _interior("interior 7x1 C7 n15 increasing bins_h", 7, 1, 7, 15, 11, "bins_increasing"),
        _interior("interior 64x300 C5 n5000 data range", 64, 300, 5, 5000, 12, "data_range"),
        _interior("interior 64x300 C7 n4000 decreasing bins_h, farthest", 64, 300, 7, 4000, 13, "bins_decreasing", True),
        _interior("interior 64x300 C3 n3000 fixed range", 64, 300, 3, 3000, 14, "fixed_range"),
    ]
    cases += [_seam(w) for w in (23, 35, 43, 64, 2048)]
    cases += _row_edge_cases() + _degenerate_cases() + _tie_cases()
    cases += [_late("late extremes n=65836", STRIDE + 300, STRIDE, 15), _late("late extremes n=131077, farthest", 2 * STRIDE + 5, 2 * STRIDE, 16, True)]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def case(name):
    return next(c for c in constructed_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name, flip=False, mutation=None):
    """(image, winners, (theta_min, theta_max)) of a constructed case by the reference [with one mutation applied]."""
    c = case(name)
    win = winners(c.cloud, c.H, c.W, keep_farthest=c.keep_farthest, mutation=mutation, **c.kw)
    theta = angles(c.cloud)[1]
    tr = (theta.min(), theta.max()) if c.theta_range is None else c.theta_range
    return image(c.cloud, win, flip, mutation), win, tr


def check_preconditions(c: Case):
    """What entitles a constructed case to ``==``: no edge-near point but the placed ones, equal ranges only where it is about ties."""
    if len(c.placed) == c.cloud.shape[0]:
        return                                                # every point is placed on purpose (one point, one elevation)
    rep = edge_report(c.cloud, c.H, c.W, c.theta_range, c.bins_h, exempt=c.placed)
    assert rep.near.size == 0, (c.name, rep.near.tolist())
    assert c.ties or rep.tie_pixels.size == 0, (c.name, rep.tie_pixels.tolist())
