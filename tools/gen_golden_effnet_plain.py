#!/usr/bin/env python
"""Pinned fixture of `models/semanticFCN.py` on an EfficientNetV2 encoder: same rules as tools/gen_golden_r03.py (runs ONLY in the build container
on the CPU, imports the reference read-only from /root/reference, writes small data-only fixtures under tests/golden/).

    python tools/gen_golden_effnet_plain.py

The reference's own class is built through the stub torchvision.models of oracle.fpn with the efficientnet_v2_* constructors of oracle.effnet
(a restatement of torchvision's public EfficientNetV2; the published parameter counts of all three models are asserted).  efficientnet_v2_s,
m = 6, attention, 20 classes, B = 1, 32 x 64: the package's class draws the fixture weights (tests/effnet_plain_restatement.py: build), the
reference class must list the same state_dict keys and shapes in the same order and loads them.  The reference class and the functional
restatement are both evaluated in float64 and must agree to 1e-10 of the output scale; the fp64 output is stored as fp32 with the inputs and the
state_dict digest.  The state_dict key -> shape list is written as JSON."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, REF)
for stub in ("seaborn", "cv2"):
    sys.modules.setdefault(stub, types.ModuleType(stub))

import effnet_plain_restatement as R          # noqa: E402
from oracle import effnet as oeff             # noqa: E402
from oracle import fpn as ofpn                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def main():
    for name, n in R.PUBLISHED_PARAMETERS.items():
        got = sum(p.numel() for p in oeff.EfficientNetRef(name).parameters())
        assert got == n, (name, got, n)
    tv = types.ModuleType("torchvision")
    tv.models = oeff.add_to_stub(ofpn.torchvision_models_stub())
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    from models.semanticFCN import SemanticNetworkWithFPN as RefFPN                       # the reference's own wiring
    backbone, config = R.GOLDEN
    m, att = R.CONFIGS[config]
    mine = R.build(R.package_class(), backbone, config, R.GOLDEN_CLASSES)
    sd = {k: v.clone() for k, v in mine.state_dict().items()}
    ref = RefFPN(backbone=backbone, input_channels=2, meta_channel_dim=m, num_classes=R.GOLDEN_CLASSES, attention=att)
    rsd = ref.state_dict()
    assert list(rsd.keys()) == list(sd.keys()), "state_dict key order differs from the reference class"
    assert all(tuple(rsd[k].shape) == tuple(sd[k].shape) for k in sd)
    ref.load_state_dict(sd)
    ref.eval()
    x, meta = R.inputs(config, 1, 32, 64)
    with torch.no_grad():
        want = ref.double()(x.double(), meta.double())
    got = R.forward(sd, x, meta, backbone, config, dtype=torch.float64)
    s = R.scale_of(want)
    err = float((got - want).abs().max())
    assert err <= 1e-10 * s, (err, s)
    path = os.path.join(OUT, R.GOLDEN_NAME + ".npz")
    np.savez_compressed(path, x=x.numpy(), meta=meta.numpy(), out=want.float().numpy(), sd_digest=np.asarray(R.sd_digest(sd)))
    print(f"  wrote {R.GOLDEN_NAME}.npz  {backbone} {config}  S = {s:.3g}  restatement - reference = {err:.1e}  ({os.path.getsize(path) / 1024:.0f} KB)")
    assert os.path.getsize(path) < 200 * 1024
    json.dump({k: list(v.shape) for k, v in rsd.items()}, open(os.path.join(OUT, R.GOLDEN_KEYS), "w"), indent=0)
    print(f"  wrote {R.GOLDEN_KEYS}  ({len(rsd)} keys)")


if __name__ == "__main__":
    main()
