"""Drop-in for ``dataset.dataloader_semantic_WADS.SemanticWADS`` of the reference (``src/dataset/dataloader_semantic_WADS.py:79-155``):
same constructor and attributes, the same five tensors per sample, computed by HIP kernels in the main process; inside a DataLoader worker
the call goes to the reference class this module shadows; ``gpu_loader`` serves ``num_workers > 0`` with the device path.

What differs from SemanticKitti: the module's own 21-class ``id_map``, a fixed ``theta_range = [-pi/2, pi/2]``, image rows without any
return deleted after the projection, then the nearest resize to (64, 1024), flip drawn with ``np.random.choice``.
``remap_adverse_label`` is stored and never read (:114-115 are comments).  With ``resize=False`` the image height depends on the scan: one
sample at a time is served (one extra host read sizes the output), a batch is refused -- the reference's default collate cannot stack
such samples either, unless their row counts happen to agree."""
from __future__ import annotations

import math

from semanticlidarunc_amd.dataset import gpu_pipeline
from semanticlidarunc_amd.dataset._mirror import MirrorDataset
from semanticlidarunc_amd.dataset.definitions import id_map as _kitti_id_map

# the module's own table (:13-51): SemanticKITTI's, plus class 20 for falling (110) and accumulated (111) snow; tests pin it to the
# fixture that was generated from the reference module
id_map = {**_kitti_id_map, 110: 20, 111: 20}

THETA_RANGE = (-math.pi / 2, math.pi / 2)


class SemanticWADS(MirrorDataset):
    _NAME = "SemanticWADS"

    def __init__(self, data_path, rotate=False, flip=False, resolution=(2048, 128), projection=(64, 2048), resize=True, remap_adverse_label=False):
        self.data_path = data_path
        self.rotate, self.flip = rotate, flip
        self.resolution, self.projection = resolution, projection
        self.remap_adverse_label = remap_adverse_label
        self.resize = resize
        self._init_mirror(record=4)

    def _spec(self):
        return gpu_pipeline.DatasetSpec(id_map=gpu_pipeline.DatasetSpec.table(id_map), theta_range=THETA_RANGE, drop_empty_rows=True)

    def _resize(self):
        return (64, 1024) if self.resize else None          # cv2.resize(..., (1024, 64), INTER_NEAREST) whatever `resolution` says (:126-127)

    def _ref_args(self):
        return (self.data_path, self.rotate, self.flip, self.resolution, self.projection, self.resize, self.remap_adverse_label)


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import shadowed_module as _shadowed_module  # noqa: E402

_shadowed = SemanticWADS._SHADOWED = _shadowed_module(__name__, __file__)
