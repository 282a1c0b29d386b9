"""The input side of the hot path on the GPU, in a form that still runs under ``DataLoader(num_workers > 0)``
(reference ``dataset/dataloader_semantic_KITTI.py:31-99``).

The reference does everything of a sample -- file decode, ``id_map`` lookup, yaw rotation, spherical projection, flip, range,
normals -- in numpy / cv2 inside forked DataLoader workers, which must not touch the GPU.  Here the workers only READ THE FILES
(``RawScanDataset``: two ``np.fromfile`` calls per sample, returned as CPU tensors the loader can pin), and the main process turns a
whole batch of raw scans into the five tensors the Trainer consumes with HIP kernels (``ScanProjector``: ``slu_kitti_decode`` ->
``slu_spherical_projection_ex`` (flip folded in) -> ``slu_build_normals`` -> ``slu_range_image_split``), written straight into the
batch tensors on the device.  ``projecting_loader_class`` packages both as a ``DataLoader`` subclass with the reference's constructor
signature, so a launcher can put it in the training script's namespace (tools/dp_launch.py does) and the script stays unchanged.

Random augmentation draws follow the reference: per sample ``np.random.randint(-180, 180)`` when ``rotate`` and then
``np.random.rand() < 0.5`` when ``flip`` (dataloader :53-54,72), from numpy's global generator -- of the main process here.

The other four datasets of ``train_semantics.py`` (SemanticSTF, SemanticTHAB, Panoptic-CUDAL, SemanticWADS) go through the same projector
with a ``DatasetSpec`` that names what their ``__getitem__`` does differently: record width, intensity division, label mask / table /
remap, range clip (``slu_point_decode`` + ``slu_spherical_projection_valid``), an organised file without projection
(``slu_organised_scan``), a fixed theta range, deleted empty rows (``slu_nonempty_rows`` + ``slu_resize_nearest_rows_hwc``), the
max-normalised reflectivity (``slu_channel_max`` + ``slu_range_image_split_ex``), and each loader's own random draws.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data as tud

from semanticlidarunc_amd import ops


def id_map_lut(id_map: dict) -> torch.Tensor:
    """Dense int32 table of ``dataset.definitions.id_map`` (-1 where the dict has no key: the reference raises KeyError there)."""
    lut = np.full(max(id_map) + 1, -1, dtype=np.int32)
    for k, v in id_map.items():
        lut[int(k)] = int(v)
    return torch.from_numpy(lut)


@dataclass(frozen=True)
class DatasetSpec:
    """What one dataset's ``__getitem__`` of the reference does between the two files and the five tensors.  ``None`` as a projector's spec is
    SemanticKITTI: the projector then runs the kernels it always ran.  The four others are built by the mirror modules
    ``dataloader_semantic_{STF,THAB,CUDAL,WADS}.py``."""
    record: int = 4                                        # floats per point in the .bin file; the first 4 are used
    intensity_div: float = 0.0                             # intensity /= this as a float32 division; 0: untouched
    label_mask: bool = True                                # label & 0xFFFF before the lookup
    id_map: Optional[Tuple[Tuple[int, int], ...]] = None   # sorted (key, class) pairs; None: the raw label is the class
    remap: Optional[Tuple[int, int]] = None                # (from, to) applied to the class
    clip: Optional[float] = None                           # points with a float32 |xyz| below it are removed before the rotation
    organised: Optional[Tuple[int, int]] = None            # (rows, columns) of a file that already is the image: no projection
    theta_range: Optional[Tuple[float, float]] = None      # fixed row range; None: the kept points' theta minimum / maximum
    drop_empty_rows: bool = False                          # image rows without any return are deleted before the resize
    refl_max_norm: bool = False                            # reflectivity / max(image maximum, 1)
    rotation: str = "yaw"                                  # "yaw": rotate_z of the cloud; "roll_yaw": column roll, then rotate_z of the image
    flip_draw: str = "choice"                              # "rand": np.random.rand() < 0.5; "choice": np.random.choice([True, False])
    draw_order: str = "rotate_first"                       # or "flip_first"

    def __post_init__(self):
        if self.record not in (4, 5) or self.rotation not in ("yaw", "roll_yaw") or self.flip_draw not in ("rand", "choice") or \
                self.draw_order not in ("rotate_first", "flip_first") or not self.intensity_div >= 0.0:
            raise ValueError(f"DatasetSpec: unsupported field value in {self!r}")
        if (self.organised is not None) != (self.rotation == "roll_yaw"):
            raise ValueError("DatasetSpec: the column roll belongs to an organised scan, and an organised scan has no other rotation")
        if self.organised is not None and (self.id_map is None or self.clip is not None or self.drop_empty_rows or self.record != 4):
            raise ValueError("DatasetSpec: an organised scan takes 4-float records and an id_map, no clip and no row deletion")

    @staticmethod
    def table(id_map: Optional[dict]):
        return None if id_map is None else tuple(sorted((int(k), int(v)) for k, v in id_map.items()))


class RawScanDataset(tud.Dataset):
    """Worker side: sample idx -> (records fp32 [N, record], label int32 [N]) exactly as the two files hold them (dataloader :35-38)."""

    def __init__(self, data_path: Sequence[Tuple[str, str]], record: int = 4):
        self.data_path = list(data_path)
        self.record = int(record)

    def __len__(self) -> int:
        return len(self.data_path)

    def __getitem__(self, idx):
        frame_path, label_path = self.data_path[idx]
        xyzi = np.fromfile(frame_path, dtype=np.float32).reshape(-1, self.record)
        label = np.fromfile(label_path, dtype=np.uint32).reshape(-1).view(np.int32)
        return torch.from_numpy(xyzi), torch.from_numpy(label)


def raw_collate(samples):
    """Scans have different point counts: keep the batch as two lists (the default collate of lists of tensors would try to stack)."""
    return [s[0] for s in samples], [s[1] for s in samples]


# slots of the per-batch error counters, read once per batch
_BAD_LABEL, _BAD_NO_ROW, _BAD_EMPTY = 0, 1, 2


class ScanProjector:
    """Main-process side: a batch of raw scans -> (range [B,1,H,W], reflectivity [B,1,H,W], xyz [B,3,H,W], normals [B,3,H,W],
    semantics int64 [B,1,H,W]) on `device`, the tuple the reference's default-collated dataset yields (dataloader :90-99)."""

    def __init__(self, id_map: Optional[dict], projection=(64, 2048), rotate: bool = False, flip: bool = False, device="cuda", norm_factor: float = 0.25,
                 resize=None, spec: Optional[DatasetSpec] = None):
        """resize: None, or (rows, columns) of the nearest-neighbour resize between projection and flip (SemanticKitti(resize=True) fixes it
        to (128, 2048), dataloader_semantic_KITTI.py:61-62); the five outputs then have that size.  spec: None = SemanticKITTI; otherwise
        the dataset's ``DatasetSpec`` -- its id_map is the one used, `id_map` may then be None; an organised spec ignores projection / resize."""
        self.height, self.width = int(projection[0]), int(projection[1])
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))
        self.rotate, self.flip, self.device, self.norm_factor = bool(rotate), bool(flip), torch.device(device), float(norm_factor)
        self.spec = spec
        if spec is not None:
            id_map = None if spec.id_map is None else dict(spec.id_map)
            if spec.organised is not None:
                self.height, self.width = int(spec.organised[0]), int(spec.organised[1])
                self.resize = None
        elif id_map is None:
            raise ValueError("ScanProjector: an id_map is needed without a spec")
        self._lut_cpu = None if id_map is None else id_map_lut(id_map)
        self._lut = None

    def draw_augmentation(self):
        """(yaw angle in degrees or None, flip decision) for one sample: the loader's own calls on numpy's global generator, in its order
        (dataloader_semantic_KITTI.py:53-54,72; _STF / _CUDAL / _WADS: randint, then choice; _THAB.py:52-57: choice, then randint)."""
        spec = self.spec
        if spec is None:
            angle = float(np.random.randint(-180, 180)) if self.rotate else None
            do_flip = bool(self.flip and np.random.rand() < 0.5)
            return angle, do_flip

        def draw_flip():
            if not self.flip:
                return False
            return bool(np.random.rand() < 0.5) if spec.flip_draw == "rand" else bool(np.random.choice([True, False]))

        def draw_angle():
            return np.random.randint(-180, 180) if self.rotate else None

        if spec.draw_order == "flip_first":
            do_flip = draw_flip()
            angle = draw_angle()
        else:
            angle = draw_angle()
            do_flip = draw_flip()
        return angle, do_flip

    def _image(self, pts, lab, angle, do_flip, bad, h, w):
        """One scan -> (img [h, w, 5] or, rows deleted and not resized, [H', W, 5]; range [h, w] or None)."""
        spec, dev = self.spec, self.device
        if spec.organised is not None:
            shift = 0
            if angle is not None:           # rotate_equirectangular_image (dataset/utils.py:21-28), the angle taken as the reference takes it
                shift = int(round((angle / (2 * np.pi)) * self.width))
            return ops.organised_scan(pts, lab, self._lut, bad[_BAD_LABEL:], self.height, self.width, do_flip, shift, angle)
        pc, valid = ops.point_decode(pts, lab, bad[_BAD_LABEL:], self._lut, spec.intensity_div, spec.label_mask, spec.remap, spec.clip, angle)
        fold = do_flip and self.resize is None and not spec.drop_empty_rows        # the flip rides on the last kernel that writes the image
        if valid is None:
            img, _ = ops.spherical_projection(pc, self.height, self.width, theta_range=spec.theta_range, flip=fold)
        else:
            img = ops.spherical_projection_valid(pc, valid, self.height, self.width, spec.theta_range, fold, bad[_BAD_EMPTY:])
        if spec.drop_empty_rows:
            rows = ops.nonempty_rows(img)
            if self.resize is None:         # the height depends on the data: one more host read (single samples only, see __call__)
                kept = int(rows[0].item())
                if kept == 0:
                    raise RuntimeError("ScanProjector: every image row of this scan is empty")
                h = kept
            img = ops.resize_nearest_rows_hwc(img, rows, h, w, bad[_BAD_NO_ROW:], do_flip)
        elif self.resize is not None:       # the reference order: project, resize, flip
            img = ops.resize_nearest_hwc(img, h, w, flip=do_flip)
        return img, None

    @torch.no_grad()
    def __call__(self, xyzi_list, label_list, augmentation: Optional[Sequence[Tuple[Optional[float], bool]]] = None):
        b, dev = len(xyzi_list), self.device
        h, w = self.resize if self.resize is not None else (self.height, self.width)
        if b == 0 or b != len(label_list):
            raise RuntimeError("ScanProjector: a non-empty batch of (xyzi, label) pairs expected")
        if self._lut_cpu is not None and (self._lut is None or self._lut.device != dev):
            self._lut = self._lut_cpu.to(dev)
        spec = self.spec
        if spec is not None and spec.drop_empty_rows and self.resize is None:
            if b != 1:
                raise RuntimeError("ScanProjector: without a resize the image height of this dataset depends on the scan (empty rows are "
                                   "deleted), so scans cannot be stacked into a batch; use resize, or batch_size = 1")
            bad = torch.zeros(4, dtype=torch.int32, device=dev)
            angle, do_flip = augmentation[0] if augmentation is not None else self.draw_augmentation()
            img, _ = self._image(xyzi_list[0].to(dev).contiguous(), label_list[0].to(dev).contiguous(), angle, do_flip, bad, h, w)
            h = img.shape[0]
            out = self._outputs(1, h, w, dev)
            ops.range_image_split_ex(img, ops.build_normals(img, self.norm_factor), *[t[0] for t in out],
                                     refl_max_key=ops.channel_max(img, 3) if spec.refl_max_norm else None)
            self._raise_if_bad(bad)
            return out
        rng, refl, xyz, nrm, sem = out = self._outputs(b, h, w, dev)
        bad = torch.zeros(1 if spec is None else 4, dtype=torch.int32, device=dev)
        for i in range(b):
            angle, do_flip = augmentation[i] if augmentation is not None else self.draw_augmentation()
            pts = xyzi_list[i].to(dev, non_blocking=True).contiguous()
            lab = label_list[i].to(dev, non_blocking=True).contiguous()
            if spec is not None:
                img, range_in = self._image(pts, lab, angle, do_flip, bad, h, w)
                normals = ops.build_normals(img, self.norm_factor)
                ops.range_image_split_ex(img, normals, rng[i], refl[i], xyz[i], nrm[i], sem[i], range_in=range_in,
                                         refl_max_key=ops.channel_max(img, 3) if spec.refl_max_norm else None)
                continue
            pc = ops.kitti_decode(pts, lab, self._lut, bad, angle)
            if self.resize is None:
                img, _ = ops.spherical_projection(pc, h, w, flip=do_flip)
            else:       # the reference order: project, resize, flip
                img, _ = ops.spherical_projection(pc, self.height, self.width)
                img = ops.resize_nearest_hwc(img, h, w, flip=do_flip)
            normals = ops.build_normals(img, self.norm_factor)
            ops.range_image_split(img, normals, rng[i], refl[i], xyz[i], nrm[i], sem[i])
        self._raise_if_bad(bad)
        return out

    @staticmethod
    def _outputs(b, h, w, dev):
        return (torch.empty((b, 1, h, w), dtype=torch.float32, device=dev), torch.empty((b, 1, h, w), dtype=torch.float32, device=dev),
                torch.empty((b, 3, h, w), dtype=torch.float32, device=dev), torch.empty((b, 3, h, w), dtype=torch.float32, device=dev),
                torch.empty((b, 1, h, w), dtype=torch.int64, device=dev))

    @staticmethod
    def _raise_if_bad(bad):
        """The one host read per batch: what the reference would have raised inside __getitem__."""
        counts = bad.tolist() + [0, 0, 0]
        if counts[_BAD_LABEL]:              # the reference's dict lookup
            raise KeyError(f"{counts[_BAD_LABEL]} point label(s) of this batch have no entry in id_map")
        if counts[_BAD_EMPTY]:              # theta.min() of an empty array (dataset/utils.py:323)
            raise RuntimeError(f"{counts[_BAD_EMPTY]} scan(s) of this batch have no point left after the range clip")
        if counts[_BAD_NO_ROW]:             # cv2.resize of an image without rows
            raise RuntimeError(f"{counts[_BAD_NO_ROW]} scan(s) of this batch project to an image whose rows are all empty")


def projecting_loader_class(projector_factory, raw_dataset_of):
    """A ``DataLoader`` subclass for a training script's namespace.  ``raw_dataset_of(dataset)`` returns the ``RawScanDataset`` twin of a
    dataset this pipeline can serve (or None: the loader then behaves like the stock one); ``projector_factory(dataset)`` builds its
    ``ScanProjector``.  Iterating yields device-resident batches in the reference's format; ``len`` / sampler / workers / pinning are the
    stock loader's."""

    class ProjectingDataLoader(tud.DataLoader):
        def __init__(self, dataset=None, *args, **kwargs):
            if dataset is None:
                dataset = kwargs.pop("dataset")
            raw = raw_dataset_of(dataset)
            self._slu_projector = None
            if raw is not None:
                if kwargs.get("collate_fn") is not None:
                    raise RuntimeError("ProjectingDataLoader: a custom collate_fn cannot be combined with the device-side projection")
                kwargs["collate_fn"] = raw_collate
                self._slu_projector = projector_factory(dataset)
                dataset = raw
            if kwargs.get("num_workers", 0) == 0:
                kwargs.pop("prefetch_factor", None)
                kwargs.pop("persistent_workers", None)
            super().__init__(dataset, *args, **kwargs)

        def __iter__(self):
            it = super().__iter__()
            if self._slu_projector is None:
                yield from it
                return
            for xyzi_list, label_list in it:
                yield self._slu_projector(xyzi_list, label_list)

    return ProjectingDataLoader
