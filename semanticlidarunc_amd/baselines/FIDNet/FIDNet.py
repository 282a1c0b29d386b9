"""Import-path mirror of the reference's ``baselines/FIDNet/FIDNet.py`` (``from FIDNet import FIDNet``).
The implementation lives in ``semanticlidarunc_amd.fidnet``; only ``backbone="ResNet34_point"`` runs, the two ASPP backbones raise
NotImplementedError.  Importing this module builds nothing: the reference's file constructs a whole ResNet34_aspp_1 model as a side effect of
being imported (FIDNet.py:3-18), which draws random numbers and is used by nothing -- that is not reproduced, and the reference module is not
re-exported for the same reason."""
from semanticlidarunc_amd.fidnet import FIDNet, Final_Model, SemanticHead, resnet34_point  # noqa: F401

__all__ = ["FIDNet", "Final_Model", "SemanticHead", "resnet34_point"]
