"""Drop-in for ``dataset.dataloader_semantic_THAB.SemanticTHAB`` of the reference (``src/dataset/dataloader_semantic_THAB.py:13-84``): same
constructor and attributes, the same five tensors per sample, computed by HIP kernels in the main process; inside a DataLoader worker the
call goes to the reference class this module shadows; ``gpu_loader`` serves ``num_workers > 0`` with the device path.

What differs from SemanticKitti: no projection -- the file is an organised 128 x 2048 scan (the reshape is hard-coded, ``projection`` and
``resize`` are stored / accepted and never read); the image is float64; flip comes first and is drawn first, with ``np.random.choice``;
rotation is a column roll by ``int(round(angle / (2 pi) * W))`` (the angle in degrees, as written there) followed by ``rotate_z`` of the
image's xyz; the range is the float64 norm rounded to float32."""
from __future__ import annotations

from semanticlidarunc_amd.dataset import gpu_pipeline
from semanticlidarunc_amd.dataset._mirror import MirrorDataset
from semanticlidarunc_amd.dataset.definitions import id_map

ORGANISED_SHAPE = (128, 2048)


class SemanticTHAB(MirrorDataset):
    _NAME = "SemanticTHAB"

    def __init__(self, data_path, rotate=False, flip=False, id_map=id_map, projection=None, resize=False):
        self.id_map = id_map
        self.data_path = data_path
        self.rotate, self.flip = rotate, flip
        self.projection = projection
        self._init_mirror(record=4)

    def _spec(self):
        # the lookup goes through the MODULE's id_map, not self.id_map (:48)
        return gpu_pipeline.DatasetSpec(id_map=gpu_pipeline.DatasetSpec.table(id_map), organised=ORGANISED_SHAPE, rotation="roll_yaw",
                                        draw_order="flip_first")

    def _ref_args(self):
        return (self.data_path, self.rotate, self.flip, self.id_map, self.projection)


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import shadowed_module as _shadowed_module  # noqa: E402

_shadowed = SemanticTHAB._SHADOWED = _shadowed_module(__name__, __file__)
