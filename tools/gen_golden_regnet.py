#!/usr/bin/env python
"""Pinned fixtures of the RegNetY encoders: same rules as tools/gen_golden_squeezenet.py (runs ONLY in the build container on the CPU,
imports the reference read-only from /root/reference, writes small data-only fixtures under tests/golden/).

    python tools/gen_golden_regnet.py

The reference's two classes (models/semanticFCN.py, baselines/Reichert/semanticFCN_opt.py) are built through the stub torchvision.models of
oracle.fpn with the regnet_y_* constructors of tests/regnet_restatement.py added -- an independent restatement of torchvision's public RegNetY
(the published parameter and state_dict entry counts of all four models are asserted), not the package's container.  Per class: B = 1,
32 x 64, 5 classes, the He fixture; the plain class on regnet_y_1_6gf with (m = 6, attention, multi-scale meta), the _opt class on
regnet_y_3_2gf with (m = 3, neither).  The reference class and the functional restatement are both evaluated in float64 and must agree to 1e-10
of the output scale; the fp64 output is stored as fp32 with the inputs and the state_dict digest.  The state_dict key -> shape lists of the two
models are written as JSON."""
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

import regnet_restatement as R          # noqa: E402
from oracle import fpn as ofpn              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def main():
    for name in R.PARAMS:
        net = R.RegNetYRef(name)
        assert R.generate(name) == (R.WIDTHS[name], R.DEPTHS[name]), name
        assert sum(p.numel() for p in net.parameters()) == R.PUBLISHED_PARAMETERS[name], name
        assert len(net.state_dict()) == R.STATE_DICT_ENTRIES[name], name
    tv = types.ModuleType("torchvision")
    tv.models = R.add_to_stub(ofpn.torchvision_models_stub())
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    from models.semanticFCN import SemanticNetworkWithFPN as RefFPN                       # the reference's own wiring
    from baselines.Reichert.semanticFCN_opt import SemanticNetworkWithFPN as RefOpt
    for kind, cls in (("plain", RefFPN), ("opt", RefOpt)):
        backbone, config = R.GOLDEN[kind]
        ref = R.build(cls, backbone, config, 5)
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        x, meta = R.inputs(config, 1, 32, 64)
        with torch.no_grad():
            want = ref.double()(x.double(), meta.double())
        got = R.forward(kind, sd, x, meta, config, dtype=torch.float64)
        s = R.scale_of(want)
        err = float((got - want).abs().max())
        assert err <= 1e-10 * s, (kind, err, s)
        name = R.golden_name(kind)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, x=x.numpy(), meta=meta.numpy(), out=want.float().numpy(), sd_digest=np.asarray(R.sd_digest(sd)))
        print(f"  wrote {name}.npz  {backbone} {config}  S = {s:.3g}  restatement - reference = {err:.1e}  ({os.path.getsize(path) / 1024:.0f} KB)")
        assert os.path.getsize(path) < 200 * 1024
        jname = f"{name}_state_dict_keys.json"
        json.dump({k: list(v.shape) for k, v in sd.items()}, open(os.path.join(OUT, jname), "w"), indent=0)
        print(f"  wrote {jname}  ({len(sd)} keys)")


if __name__ == "__main__":
    main()
