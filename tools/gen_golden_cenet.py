#!/usr/bin/env python
"""Pinned fixtures of the CENet ResNet-34 baseline: same rules as tools/gen_golden.py (runs ONLY in the build container on the CPU, imports the
reference read-only from /root/reference, writes small data-only fixtures under tests/golden/).

    python tools/gen_golden_cenet.py

The reference's own classes (baselines/CENet/CENet.py, CENet_ResNet34.py -- imported by their flat names from inside that folder, as CENet.py
itself does) are built from each case's seed, their BatchNorm statistics and affines randomised by tests/cenet_restatement.randomise_bn, and run
in fp32 on the case's input.  The randomisation's `gain` is the first of GAINS at which every returned map has at least 20 % of its pixels with a
largest class probability below 0.9 AND the main output at least 20 % above 2 / C (a saturated or a uniform softmax would make the parity bar of
the GPU test vacuous); it is stored with the seed, the input, the fp32 outputs and the digest of the freshly initialised state_dict.  No weights
are stored.  The state_dict key -> shape lists of the constructed models are written as JSON."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/baselines/CENet"
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, REF)

import cenet_restatement as R          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GAINS = (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 0.75, 0.5)
torch.set_num_threads(8)


def main():
    from CENet import CENet as RefCENet                    # the reference's own wiring
    from CENet_ResNet34 import ResNet_34 as RefResNet34
    keys = {}
    for case in R.CASES:
        name, _, ncls, _, aux, _, seed = case
        x = R.case_input(case)
        chosen = None
        for gain in GAINS:
            ref = R.construct(case, RefCENet, RefResNet34).eval()
            sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
            R.randomise_bn(ref, seed, gain)
            with torch.no_grad():
                outs = R.as_list(ref(x))
            unsat = [R.unsaturated_fraction(o) for o in outs]
            informative = float((outs[0].max(1).values > 2.0 / ncls).double().mean())
            print(f"  {name} gain {gain}: unsaturated {['%.2f' % u for u in unsat]}, main output above 2/C on {informative:.2f}")
            if min(unsat) >= 0.2 and informative >= 0.2:
                chosen = gain
                break
        assert chosen is not None, name
        assert all(o.shape == (x.shape[0], ncls) + tuple(x.shape[2:]) for o in outs) and len(outs) == (4 if aux else 1)
        sd = ref.state_dict()
        got = R.as_list(R.forward(sd, x, aux, R.prefix_of(case)))
        err = max(float((a - b).abs().max()) for a, b in zip(got, outs))
        assert err <= 1e-5, (name, err)
        keys[R.keys_label(case)] = {k: list(v.shape) for k, v in sd.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, seed=np.asarray(seed), gain=np.asarray(chosen), x=x.numpy(), n_out=np.asarray(len(outs)),
                            sd_digest=np.asarray(R.sd_digest(sd0)), **{f"out{i}": o.numpy() for i, o in enumerate(outs)})
        print(f"  wrote {name}.npz  gain {chosen}  restatement (fp32) - reference = {err:.1e}  ({os.path.getsize(path) / 1024:.0f} KB)")
        assert os.path.getsize(path) < 800 * 1024      # four [2, 20, 16, 64] fp32 maps are 640 KB of the largest
    json.dump(keys, open(os.path.join(OUT, R.KEYS_JSON), "w"), indent=0)
    print(f"  wrote {R.KEYS_JSON}  ({[len(v) for v in keys.values()]} keys)")


if __name__ == "__main__":
    main()
