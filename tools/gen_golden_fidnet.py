#!/usr/bin/env python
"""Pinned fixtures of the FIDNet ResNet34_point baseline: same rules as tools/gen_golden.py (runs ONLY in the build container on the CPU, imports the
reference read-only from /root/reference, writes small data-only fixtures under tests/golden/).

    python tools/gen_golden_fidnet.py

The reference's own class (baselines/FIDNet/FIDNet.py -- imported by its flat name from inside that folder, as its `from ResNet import *` needs)
is built from each case's seed, its BatchNorm statistics and affines randomised by cenet_restatement.randomise_bn, and run in fp32 on the case's
input.  Importing the reference's FIDNet.py builds a whole model (FIDNet.py:3-18) and so consumes random numbers: every seed is set AFTER the
import.  The randomisation's `gain` is the first of fidnet_restatement.GAINS at which 1 <= max|logit| <= 20 and some logit deviates from its
class's mean over the pixels by at least a quarter of max|logit| (more than 36 chained BatchNorms move the output scale about threefold per 0.05 of
gain, hence the fine grid); it is stored with the seed, the input, the fp32 logits, the digest of the freshly initialised state_dict and, per
channel slice of the backend's 1024-channel output (a forward hook on model.backend), its (sum, abs-sum) and 64 strided samples.  No weights are
stored, and the files regenerate byte for byte (numpy dates the zip members 1980-01-01; the generator checks it).  The state_dict key -> shape
lists of the constructed models are written as JSON."""
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/baselines/FIDNet"
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, REF)

import fidnet_restatement as R          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def main():
    from FIDNet import FIDNet as RefFIDNet                 # builds the reference's module-level model: seeds are set after this line
    keys = {}
    for case in R.CASES:
        name, ncls, _, shape, seed = case
        x = R.case_input(case)
        chosen = None
        for gain in R.GAINS:
            ref = R.construct(case, RefFIDNet).eval()
            sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
            R.randomise_bn(ref, seed, gain)
            mids = []
            hook = ref.model.backend.register_forward_hook(lambda m, i, o: mids.append(o.detach()))
            with torch.no_grad():
                out = ref(x)
            hook.remove()
            scale, dev = R.gain_conditions(out)
            print(f"  {name} gain {gain}: max|logit| {scale:.3g}, deviation / scale {dev / scale:.2f}")
            if R.gain_ok(out):
                chosen = gain
                break
        assert chosen is not None, name
        assert out.shape == (shape[0], ncls) + tuple(shape[2:]) and len(mids) == 1 and mids[0].shape[1] == 1024
        sd = ref.state_dict()
        got, mid = R.forward(sd, x, want_backend=True)
        err = float((got - out).abs().max())
        out64 = R.forward(sd, x, dtype=torch.float64)
        e64 = float((out.double() - out64).abs().max())
        assert err <= 1e-5 * scale and float((mid - mids[0]).abs().max()) <= 1e-5 * float(mids[0].abs().max()), (name, err)
        sums, samples = R.backend_digest(mids[0])
        keys[R.keys_label(case)] = {k: list(v.shape) for k, v in sd.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, seed=np.asarray(seed), gain=np.asarray(chosen), x=x.numpy(), logits=out.numpy(),
                            sd_digest=np.asarray(R.sd_digest(sd0)), backend_sums=sums, backend_samples=samples)
        print(f"  wrote {name}.npz  gain {chosen}  restatement (fp32) - reference = {err:.1e}, reference - fp64 restatement = {e64:.1e} "
              f"({e64 / scale:.1e} of the scale)  ({os.path.getsize(path) / 1024:.0f} KB)")
        assert os.path.getsize(path) < 800 * 1024
        # byte-identical regeneration: numpy writes every zip member with the fixed date 1980-01-01, not the clock
        assert all(i.date_time == (1980, 1, 1, 0, 0, 0) for i in zipfile.ZipFile(path).infolist()), name
    json.dump(keys, open(os.path.join(OUT, R.KEYS_JSON), "w"), indent=0)
    print(f"  wrote {R.KEYS_JSON}  ({[len(v) for v in keys.values()]} keys)")


if __name__ == "__main__":
    main()
