"""Import-path mirror of the reference's ``baselines/CENet/CENet.py`` (``from CENet import CENet``).
The implementation lives in ``semanticlidarunc_amd.cenet``; only ``model="ResNet_34"`` runs, ``model="HarDNet"`` raises NotImplementedError.
The reference module is not re-exported: it imports its HarDNet variant by a flat name that only resolves from inside its own folder."""
from semanticlidarunc_amd.cenet import CENet, ResNet_34  # noqa: F401

__all__ = ["CENet", "ResNet_34"]
