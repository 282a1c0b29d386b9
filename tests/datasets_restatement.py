"""Test infrastructure, in the spirit of ``oracle/kitti.py``: one sample of each of the four other dataloaders of the reference
(``src/dataset/dataloader_semantic_{STF,THAB,CUDAL,WADS}.py``, ``__getitem__``), restated in numpy from the file contents to the five
arrays, with the augmentation draws (yaw angle in degrees or None, flip decision) as explicit arguments.  The projection, the normals,
the nearest resize and ``rotate_z`` are the oracle's.  ``tools/gen_golden_datasets.py`` pins every function here to the reference class
(bit for bit; xyz / range within 1 float32 ulp where a yaw went through BLAS); cv2 is absent from the build image, so the normals and
the resize are "parity unpinned" like SemanticKITTI's.

Also the pieces the kernel-level GPU tests compare with (``clip_keep``, ``organised_image``, ``nonempty_rows``, ``resize_rows``), and the
synthetic scans of the fixtures, built so that each loader's special rule has something to get wrong."""
from __future__ import annotations

import numpy as np

from oracle import kitti as okitti
from oracle import normals as onormals
from oracle import projection as oproj

NAMES = ("range", "reflectivity", "xyz", "normals", "semantics")
LOCAL_SENSOR_CLIP = 1.8


# ---------------------------------------------------------------------------------------------------------------------
# shared ends
# ---------------------------------------------------------------------------------------------------------------------
def _flip(img):
    img = img[:, ::-1, :]
    img[..., 1] = -img[..., 1]
    return img


def _outputs(img, refl=None, with_normals=True):
    """image [H, W, 5] (float32 after a projection, float64 for the organised scan) -> the five arrays; the norm runs in the image's dtype."""
    label_img, xyz = img[..., 4:5], img[..., 0:3]
    refl = img[..., 3] if refl is None else refl
    rng = np.linalg.norm(xyz, axis=-1)
    nrm = onormals.build_normal_xyz(xyz) if with_normals else np.zeros(xyz.shape, np.float32)
    return (rng[..., None].transpose(2, 0, 1).astype("float32"), refl[..., None].transpose(2, 0, 1).astype("float32"),
            xyz.transpose(2, 0, 1).astype("float32"), nrm.transpose(2, 0, 1).astype("float32"), label_img.transpose(2, 0, 1).astype("int64"))


def _labels(label_bytes):
    return np.frombuffer(label_bytes, dtype=np.uint32).reshape(-1)


def _mapped(label_bytes, id_map):
    return np.array([id_map[int(l)] for l in _labels(label_bytes) & 0xFFFF])


# ---------------------------------------------------------------------------------------------------------------------
# STF
# ---------------------------------------------------------------------------------------------------------------------
def clip_keep(xyz_f32, clip_min=LOCAL_SENSOR_CLIP):
    """Which points the range clip keeps: numpy's float32 norm against the Python float (dataloader_semantic_STF.py:51-52)."""
    return np.linalg.norm(xyz_f32, axis=-1) >= clip_min


def stf_cloud(bin_bytes, label_bytes, remap_adverse_label=False, clip=True):
    """-> float64 [N', 5]: :37-58."""
    xyzi = np.frombuffer(bin_bytes, dtype=np.float32).reshape(-1, 5)[:, :4].copy()
    xyzi[:, 3] /= 255.
    sem = _labels(label_bytes)
    if clip:
        keep = np.where(clip_keep(xyzi[:, 0:3]))
        sem, xyzi = sem[keep], xyzi[keep]
    if remap_adverse_label:
        sem = np.where(sem == 20, 0, sem)
    return np.concatenate([xyzi, sem[..., np.newaxis]], axis=-1)


def stf_sample(bin_bytes, label_bytes, projection=(64, 2048), rotate_angle=None, flip=False, resize=True, remap_adverse_label=False, clip=True):
    xyzil = stf_cloud(bin_bytes, label_bytes, remap_adverse_label, clip)
    if rotate_angle is not None:
        xyzil[..., 0:3] = okitti.rotate_z(xyzil[..., 0:3].reshape(-1, 3), rotate_angle)
    img, _, _, _ = oproj.spherical_projection(xyzil, projection[0], projection[1])
    if resize:
        img = okitti.resize_nearest(img, 128, 2048)
    if flip:
        img = _flip(img)
    return _outputs(img)


# ---------------------------------------------------------------------------------------------------------------------
# THAB
# ---------------------------------------------------------------------------------------------------------------------
def roll_shift(angle, width):
    """rotate_equirectangular_image's shift (dataset/utils.py:23): the angle is in degrees and is divided by 2 pi, as written there."""
    return int(round((angle / (2 * np.pi)) * width))


def organised_image(xyzi, mapped, height, width, flip=False, shift=0, rotate_angle=None):
    """float64 [H, W, 5] in the loader's order (dataloader_semantic_THAB.py:49-59): concatenate, flip, roll, rotate_z."""
    img = np.concatenate((xyzi.reshape((height, width, 4)), np.asarray(mapped).reshape((height, width, 1))), axis=-1)
    if flip:
        img = _flip(img)
    img = np.roll(img, shift, axis=1)
    if rotate_angle is not None:
        img[..., 0:3] = okitti.rotate_z(img[..., 0:3].reshape(-1, 3), rotate_angle).reshape(img[..., 0:3].shape)
    return img


def thab_sample(bin_bytes, label_bytes, id_map, rotate_angle=None, flip=False, shape=(128, 2048), with_normals=True):
    xyzi = np.frombuffer(bin_bytes, dtype=np.float32).reshape(-1, 4)
    shift = 0 if rotate_angle is None else roll_shift(rotate_angle, shape[1])
    img = organised_image(xyzi, _mapped(label_bytes, id_map), shape[0], shape[1], flip, shift, rotate_angle)
    return _outputs(img, with_normals=with_normals)


# ---------------------------------------------------------------------------------------------------------------------
# CUDAL
# ---------------------------------------------------------------------------------------------------------------------
CUDAL_THETA = (-np.pi / 8, np.pi / 8)


def cudal_sample(bin_bytes, label_bytes, id_map, projection=(128, 2048), rotate_angle=None, flip=False, resize=True):
    xyzil = okitti.decode(bin_bytes, label_bytes, id_map)
    if rotate_angle is not None:
        xyzil[..., 0:3] = okitti.rotate_z(xyzil[..., 0:3].reshape(-1, 3), rotate_angle)
    img, _, _, _ = oproj.spherical_projection(xyzil, projection[0], projection[1], theta_range=list(CUDAL_THETA))
    if resize:
        img = okitti.resize_nearest(img, 128, 2048)
    if flip:
        img = _flip(img)
    refl = img[..., 3] / np.maximum(img[..., 3].max(), 1.0)          # :107
    return _outputs(img, refl=refl)


# ---------------------------------------------------------------------------------------------------------------------
# WADS
# ---------------------------------------------------------------------------------------------------------------------
WADS_THETA = (-np.pi / 2, np.pi / 2)
WADS_FULL_PLACED = (0,)          # synth_wads(bands=None): the point put on the top row edge on purpose (an exactly representable angle)


def nonempty_rows(img):
    """Indices of the rows that survive ``img[~np.all(np.linalg.norm(img, axis=-1) == 0, axis=1)]`` (dataloader_semantic_WADS.py:125)."""
    return np.flatnonzero(~np.all(np.linalg.norm(img, axis=-1) == 0, axis=1))


def resize_rows(img, out_h, out_w, flip=False):
    """Row deletion + nearest resize + flip; ValueError when no row is left (cv2.resize raises on an empty image)."""
    rows = nonempty_rows(img)
    if rows.size == 0:
        raise ValueError("no image row left")
    out = okitti.resize_nearest(img[rows], out_h, out_w)
    return _flip(out) if flip else out


def wads_sample(bin_bytes, label_bytes, id_map, projection=(64, 2048), rotate_angle=None, flip=False, resize=True):
    xyzil = okitti.decode(bin_bytes, label_bytes, id_map)
    if rotate_angle is not None:
        xyzil[..., 0:3] = okitti.rotate_z(xyzil[..., 0:3].reshape(-1, 3), rotate_angle)
    img, _, _, _ = oproj.spherical_projection(xyzil, projection[0], projection[1], theta_range=list(WADS_THETA))
    img = img[nonempty_rows(img)]
    if resize:
        if img.shape[0] == 0:
            raise ValueError("no image row left")
        img = okitti.resize_nearest(img, 64, 1024)
    if flip:
        img = _flip(img)
    return _outputs(img)


# ---------------------------------------------------------------------------------------------------------------------
# the clouds the exactness preconditions are asserted on (tests/projection_cases.py: edge_report)
# ---------------------------------------------------------------------------------------------------------------------
def projected_cloud(name, bin_bytes, label_bytes, id_map, rotate_angle=None, **kw):
    """(cloud float64 [N, 5] as the projection receives it, theta_range or None) of the three projected datasets."""
    if name == "stf":
        cloud, tr = stf_cloud(bin_bytes, label_bytes, kw.get("remap_adverse_label", False), kw.get("clip", True)), None
    else:
        cloud, tr = okitti.decode(bin_bytes, label_bytes, id_map), CUDAL_THETA if name == "cudal" else WADS_THETA
    if rotate_angle is not None:
        cloud[:, 0:3] = okitti.rotate_z(cloud[:, 0:3].reshape(-1, 3), rotate_angle)
    return cloud, tr


# ---------------------------------------------------------------------------------------------------------------------
# synthetic scans: the generator stores what these return; tests read the stored bytes
# ---------------------------------------------------------------------------------------------------------------------
def _sphere(g, n, el_lo, el_hi, r_lo, r_hi):
    az, el, r = g.uniform(-np.pi, np.pi, n), g.uniform(el_lo, el_hi, n), g.uniform(r_lo, r_hi, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1)


def _keyed_labels(g, id_map, n):
    keys = np.array(sorted(id_map), dtype=np.uint32)
    return (keys[g.integers(0, len(keys), n)] | (g.integers(0, 500, n).astype(np.uint32) << 16)).astype(np.uint32)


def synth_stf(n=16000, seed=11):
    """5-float records; intensities up to 255; labels: classes 0..22 (20 among them), some above 0xFFFF; 300 points inside the 1.8 m clip
    sphere that hold BOTH theta extremes of the file (a wrong data range moves every row); norms at np.float32(1.8) and its float32
    neighbours, and squares sums that round differently in float32 and float64 around 1.8^2."""
    g = np.random.default_rng(seed)
    far = _sphere(g, n - 320, np.radians(-24.0), np.radians(2.0), 2.5, 80.0)
    near = _sphere(g, 300, np.radians(-60.0), np.radians(40.0), 0.3, 1.75)
    near[0], near[1] = [0.2, 0.1, 1.2], [0.3, -0.1, -1.5]                  # steep up / down: the theta extremes, both clipped
    t = np.float32(1.8)
    lo, hi = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(4))
    az, el = g.uniform(-3, 3, 20), g.uniform(-0.3, 0.0, 20)
    shell_r = np.array([lo, t, hi, lo, t, hi, 1.7999, 1.8001, 1.79999, 1.80001] * 2, dtype=np.float64)
    shell = np.stack([shell_r * np.cos(el) * np.cos(az), shell_r * np.cos(el) * np.sin(az), shell_r * np.sin(el)], -1)
    shell[0], shell[1], shell[2] = [float(lo), 0, 0], [float(t), 0, 0], [0, -float(hi), 0]      # norms exactly at the threshold's neighbours
    xyz = np.concatenate([far, near, shell])
    p = g.permutation(xyz.shape[0])
    xyz = xyz[p]
    rec = np.concatenate([xyz, g.uniform(0, 255, (n, 1)), g.uniform(0, 1, (n, 1))], -1).astype(np.float32)
    label = g.integers(0, 23, n).astype(np.uint32)
    label[::37] = 20
    label[5::41] = np.uint32(70000) + g.integers(0, 1000, label[5::41].size).astype(np.uint32)
    label[7::43] = np.uint32(0x140014)                                     # low 16 bits are 20: stays as it is without a mask
    return rec, label


def synth_thab(id_map, seed=12, shape=(128, 2048)):
    """A sparse organised scan: three row bands and two column bands, one of them across the wrap-around; zeros elsewhere."""
    g = np.random.default_rng(seed)
    h, w = shape
    occ = np.zeros((h, w), dtype=bool)
    for r0, r1 in ((0, 3), (60, 64), (126, 128)):
        occ[r0:r1, :] = g.uniform(size=(r1 - r0, w)) < 0.5
    occ[:, 2040:] |= g.uniform(size=(h, w - 2040)) < 0.6
    occ[:, :6] |= g.uniform(size=(h, 6)) < 0.6
    occ[:, 1000:1003] = True
    rows, cols = np.nonzero(occ)
    az = np.pi - (cols + 0.5) * (2 * np.pi / w)
    el = np.radians(22.5) - rows * (np.radians(45.0) / (h - 1))
    r = g.uniform(1.0, 60.0, rows.size)
    rec = np.zeros((h, w, 4), dtype=np.float32)
    rec[rows, cols] = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), g.uniform(0, 1, rows.size)], -1)
    label = np.zeros((h, w), dtype=np.uint32)
    label[rows, cols] = _keyed_labels(g, id_map, rows.size)
    return rec.reshape(-1, 4), label.reshape(-1)


def synth_cudal(id_map, n=16000, seed=13, max_intensity=37.0):
    """Elevations beyond +-pi/8 on both sides (they share the last row); intensity maximum above or below 1."""
    g = np.random.default_rng(seed)
    xyz = _sphere(g, n, np.radians(-35.0), np.radians(35.0), 1.5, 80.0)
    rec = np.concatenate([xyz, g.uniform(0, max_intensity, (n, 1))], -1).astype(np.float32)
    return rec, _keyed_labels(g, id_map, n)


def synth_wads(id_map, n=16000, seed=14, bands=((-0.60, -0.35), (-0.20, 0.05), (0.30, 0.45))):
    """Elevation bands inside [-pi/2, pi/2] -> 32 rows of about 0.1 rad: leading, interior and trailing rows stay empty.  bands=None: every
    row receives points."""
    g = np.random.default_rng(seed)
    if bands is None:
        xyz = _sphere(g, n, -1.5, 1.5, 1.5, 80.0)
        # the last row holds only theta >= pi/2 (the -1 of digitize) or < -pi/2: the zenith point, theta = pi/2 exactly, fills it (WADS_FULL_PLACED)
        xyz[0] = [0.0, 0.0, 5.0]
    else:
        k = n // len(bands)
        xyz = np.concatenate([_sphere(g, k if i else n - k * (len(bands) - 1), lo, hi, 1.5, 80.0) for i, (lo, hi) in enumerate(bands)])
        xyz = xyz[g.permutation(n)]
    rec = np.concatenate([xyz, g.uniform(0, 1, (n, 1))], -1).astype(np.float32)
    return rec, _keyed_labels(g, id_map, n)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture cases: (tag, scan, constructor keywords on top of BASE_KW, rotate, flip); generator and tests walk the same table
# ---------------------------------------------------------------------------------------------------------------------
BASE_KW = {"stf": dict(projection=(32, 256), resize=False), "cudal": dict(projection=(32, 256), resize=False),
           "wads": dict(projection=(32, 256), resize=True), "thab": dict()}
_FOUR = [("plain", "a", {}, False, False), ("rot", "a", {}, True, False), ("flip", "a", {}, False, True), ("rotflip", "a", {}, True, True)]
CASES = {
    "stf": _FOUR + [("plain_remap", "a", {"remap_adverse_label": True}, False, False), ("plain_noclip", "a", {"clip": False}, False, False)],
    "thab": _FOUR,
    "cudal": _FOUR + [("plain_dim", "b", {}, False, False)],                       # scan b: intensity maximum below 1
    "wads": _FOUR + [("plain_noresize", "a", {"resize": False}, False, False), ("plain_full", "b", {}, False, False)],   # scan b: no empty row
}
CLASS_OF = {"stf": "SemanticSTF", "thab": "SemanticTHAB", "cudal": "SemanticCUDAL", "wads": "SemanticWADS"}
STORES_NORMALS = {"stf": True, "cudal": True, "thab": False, "wads": False}


def restate(name, bin_bytes, label_bytes, id_map, kw, angle, flip):
    """The five arrays of dataset `name` for constructor keywords `kw` (BASE_KW merged in) and the given draws."""
    kw = {**BASE_KW[name], **kw}
    if name == "stf":
        return stf_sample(bin_bytes, label_bytes, kw["projection"], angle, flip, kw["resize"], kw.get("remap_adverse_label", False), kw.get("clip", True))
    if name == "thab":
        return thab_sample(bin_bytes, label_bytes, id_map, angle, flip)
    if name == "cudal":
        return cudal_sample(bin_bytes, label_bytes, id_map, kw["projection"], angle, flip, kw["resize"])
    return wads_sample(bin_bytes, label_bytes, id_map, kw["projection"], angle, flip, kw["resize"])


# ---------------------------------------------------------------------------------------------------------------------
# fixture access shared by the CPU and the GPU test file
# ---------------------------------------------------------------------------------------------------------------------
import functools                                                             # noqa: E402
import json                                                                  # noqa: E402
import os                                                                    # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATASETS = ("stf", "thab", "cudal", "wads")
ALL_CASES = [(n, c[0]) for n in DATASETS for c in CASES[n]]


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def mirror_class(name):
    """(the drop-in class of this repository, its module)."""
    mod = __import__(f"semanticlidarunc_amd.dataset.dataloader_semantic_{name.upper()}", fromlist=["x"])
    return getattr(mod, CLASS_OF[name]), mod


@functools.lru_cache(maxsize=None)
def inputs(name):
    """({records_<scan>, label_<scan>}, meta) of dataset_<name>_input.npz."""
    g = load(f"dataset_{name}_input")
    return {k: g[k] for k in g.files if k != "meta"}, json.loads(str(g["meta"]))


@functools.lru_cache(maxsize=None)
def id_maps():
    with open(os.path.join(GOLDEN, "dataset_id_maps.json")) as f:
        return {n: {int(k): int(v) for k, v in t.items()} for n, t in json.load(f).items()}


def table_of(name):
    """The label table the reference class of `name` applies (None: raw labels)."""
    from semanticlidarunc_amd.dataset.definitions import id_map as kitti_id_map
    return {"stf": None, "thab": kitti_id_map, "cudal": id_maps()["cudal"], "wads": id_maps()["wads"]}[name]
