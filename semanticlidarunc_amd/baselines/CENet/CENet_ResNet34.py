"""Import-path mirror of the reference's ``baselines/CENet/CENet_ResNet34.py`` (``from CENet_ResNet34 import ResNet_34``).
The implementation lives in ``semanticlidarunc_amd.cenet``."""
from semanticlidarunc_amd.cenet import BasicBlock, BasicConv2d, ResNet_34, conv1x1, conv3x3  # noqa: F401

__all__ = ["ResNet_34", "BasicBlock", "BasicConv2d", "conv3x3", "conv1x1"]


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(__name__, __file__, globals())
