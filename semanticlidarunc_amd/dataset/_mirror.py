"""What the drop-in dataset classes of the STF / THAB / CUDAL / WADS loaders share: ``dataloader_semantic_KITTI.py``'s scheme -- the HIP
path in the main process, delegation to the shadowed reference class inside a DataLoader worker (which must not touch the GPU), and
``gpu_loader`` for ``num_workers > 0`` with the device path.  A subclass states its constructor, ``_NAME``, ``_spec()``, ``_resize()``
and ``_ref_args()``; its module sets ``_SHADOWED`` to the reference module it shadows (or None)."""
from __future__ import annotations

import torch
import torch.utils.data
from torch.utils.data import Dataset

from semanticlidarunc_amd.dataset import gpu_pipeline


class MirrorDataset(Dataset):
    _NAME = ""
    _SHADOWED = None

    def _init_mirror(self, record=4):
        self._raw = gpu_pipeline.RawScanDataset(self.data_path, record=record)
        self._projector = None
        self._projector_key = None
        self._ref = None

    def __len__(self):
        return len(self.data_path)

    def _spec(self) -> gpu_pipeline.DatasetSpec:
        raise NotImplementedError

    def _resize(self):
        return None

    def _ref_args(self):
        raise NotImplementedError

    def projector(self, device="cuda") -> gpu_pipeline.ScanProjector:
        return gpu_pipeline.ScanProjector(None, self.projection if self.projection is not None else (0, 0), self.rotate, self.flip, device,
                                          resize=self._resize(), spec=self._spec())

    def __getitem__(self, idx):
        if torch.utils.data.get_worker_info() is not None:
            shadowed = type(self)._SHADOWED
            if shadowed is None:
                raise RuntimeError(f"{self._NAME}: the HIP path cannot run inside a DataLoader worker; use {self._NAME}.gpu_loader(...) "
                                   "(workers read files, the main process projects) or keep the reference's dataset package on sys.path")
            if self._ref is None:
                from .utils import _warn_delegation
                _warn_delegation(f"{self._NAME}.__getitem__")
                self._ref = getattr(shadowed, self._NAME)(*self._ref_args())
            for name in ("remap_adverse_label",):           # train_semantics.py sets it after construction
                if hasattr(self, name):
                    setattr(self._ref, name, getattr(self, name))
            return self._ref[idx]
        key = (self._spec(), self._resize(), self.rotate, self.flip)       # attributes set after construction are read at call time
        if self._projector is None or key != self._projector_key:
            self._projector, self._projector_key = self.projector(), key
        xyzi, label = self._raw[idx]
        out = self._projector([xyzi], [label])
        return tuple(t[0].cpu() for t in out)          # CPU tensors like the reference (a loader with pin_memory=True pins them)

    def gpu_loader(self, device="cuda", **loader_kwargs):
        """DataLoader(num_workers > 0)-compatible device pipeline over this dataset: yields (range, reflectivity, xyz, normals, semantics)
        batches that already live on `device`."""
        cls = gpu_pipeline.projecting_loader_class(lambda ds: ds.projector(device), lambda ds: getattr(ds, "_raw", None) if hasattr(ds, "projector") else None)
        return cls(self, **loader_kwargs)
