"""Import-path mirror of the reference's ``baselines/FIDNet/ResNet.py`` (``from ResNet import *``): the classes the ResNet34_point backbone is
made of.  The implementation lives in ``semanticlidarunc_amd.fidnet``; the ASPP backbones and the Bottleneck block are not provided."""
from semanticlidarunc_amd.fidnet import BasicBlock, Final_Model, ResNet_34_point, SemanticHead, conv1x1, conv3x3, resnet34_point  # noqa: F401

__all__ = ["BasicBlock", "Final_Model", "ResNet_34_point", "SemanticHead", "conv3x3", "conv1x1", "resnet34_point"]
