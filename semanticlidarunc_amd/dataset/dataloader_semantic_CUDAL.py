"""Drop-in for ``dataset.dataloader_semantic_CUDAL.SemanticCUDAL`` of the reference (``src/dataset/dataloader_semantic_CUDAL.py:54-125``):
same constructor and attributes, the same five tensors per sample, computed by HIP kernels in the main process; inside a DataLoader worker
the call goes to the reference class this module shadows; ``gpu_loader`` serves ``num_workers > 0`` with the device path.

What differs from SemanticKitti: the module's own ``id_map``, a fixed ``theta_range = [-pi/8, pi/8]`` (points outside share the last
row), projection default (128, 2048), reflectivity divided by ``max(image maximum, 1)`` in float32, flip drawn with ``np.random.choice``."""
from __future__ import annotations

import math

from semanticlidarunc_amd.dataset import gpu_pipeline
from semanticlidarunc_amd.dataset._mirror import MirrorDataset
from semanticlidarunc_amd.dataset.definitions import id_map as _kitti_id_map

# the module's own table (:14-51): SemanticKITTI's, plus raw id 2 folded into class 12 (other-ground); tests pin it to the fixture that
# was generated from the reference module
id_map = {**_kitti_id_map, 2: 12}

THETA_RANGE = (-math.pi / 8, math.pi / 8)


class SemanticCUDAL(MirrorDataset):
    _NAME = "SemanticCUDAL"

    def __init__(self, data_path, rotate=False, flip=False, resolution=(2048, 128), projection=(128, 2048), resize=True):
        self.data_path = data_path
        self.rotate, self.flip = rotate, flip
        self.resolution, self.projection, self.resize = resolution, projection, resize
        self._init_mirror(record=4)

    def _spec(self):
        return gpu_pipeline.DatasetSpec(id_map=gpu_pipeline.DatasetSpec.table(id_map), theta_range=THETA_RANGE, refl_max_norm=True)

    def _resize(self):
        return (128, 2048) if self.resize else None         # cv2.resize(..., (2048, 128), INTER_NEAREST) whatever `resolution` says (:96-97)

    def _ref_args(self):
        return (self.data_path, self.rotate, self.flip, self.resolution, self.projection, self.resize)


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import shadowed_module as _shadowed_module  # noqa: E402

_shadowed = SemanticCUDAL._SHADOWED = _shadowed_module(__name__, __file__)
