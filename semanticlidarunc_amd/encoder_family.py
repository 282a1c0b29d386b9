"""What the two FPN segmenters (fpn.py, fpn_opt.py) need to know about an encoder family: one `EncoderFamily` record per family, defined next to
the family's container and forward (shufflenet.py, squeezenet.py, regnet.py, effnet.py; fpn.py for the ResNets) and looked up by backbone name
with `fpn.family_of`.  A plain record: a new family is one more instance in `fpn.FAMILIES`."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple


class EncoderFamily(NamedTuple):
    backbones: Tuple[str, ...]             # the backbone names the FPN classes accept for this family
    build: Callable                        # (host, backbone, input_channels, meta_channel_dim) -> channel ladder [x4, fpn4 .. fpn1 out]
    encode: Callable                       # (host, x, meta) -> (x1, x2, x3, x4), inference
    head_scales: Tuple[int, int, int]      # transposed-conv / UpsampleBlock scales of x4, x3, x2
    inference_clause: Optional[str]        # why `models.semanticFCN` refuses training / gradients (None: it trains)
    training_refuses: bool                 # does model.train() alone trigger that refusal (without a train-mode BatchNorm or a gradient)
    trains_in_opt: bool                    # `semanticFCN_opt` has a training path for the family
    mc_shared_prefix: bool                 # `semanticFCN_opt` may run MC dropout on the shared-prefix schedule


def run_stages(host, block_forward, h, stages):
    """The outputs of a run of stages: `stages` = ((layer name, blocks, meta_k), ...), `block_forward(host, name, blk, h, meta_k)` the family's
    block on the HIP kernels; meta_k goes to the first block of its stage only."""
    outs = []
    for lname, stage, mk in stages:
        for bi, blk in enumerate(stage):
            h = block_forward(host, f"{lname}.{bi}", blk, h, mk if bi == 0 else None)
        outs.append(h)
    return outs
