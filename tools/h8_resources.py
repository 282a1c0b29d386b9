#!/usr/bin/env python
"""Register / scratch summary of the kernels in a `-Rpass-analysis=kernel-resource-usage` log (development aid):
    hipcc ... -Rpass-analysis=kernel-resource-usage -c conv_h8_tiled.hip 2> log ; python tools/h8_resources.py log [name-substring ...]
    python tools/h8_resources.py --diff old.log new.log      every kernel whose resource lines differ between two logs (exit status 1 if any)"""
import collections
import re
import sys



def read(path):
    rows = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        name = b.split("\n")[0].split(" ")[0]
        g = lambda pat: int(re.search(pat, b).group(1))
        rows[name] = (g(r"ScratchSize \[bytes/lane\]: (\d+)"), g(r" VGPRs: (\d+)"), g(r"AGPRs: (\d+)"), g(r"SGPRs: (\d+)"), g(r"Occupancy \[waves/SIMD\]: (\d+)"),
                      g(r"SGPRs Spill: (\d+)"), g(r"VGPRs Spill: (\d+)"), g(r"LDS Size \[bytes/block\]: (\d+)"))
    return rows


if sys.argv[1] == "--diff":      # (scratch, VGPRs, AGPRs, SGPRs, occupancy, SGPR spills, VGPR spills, static LDS) per kernel
    old, new = read(sys.argv[2]), read(sys.argv[3])
    changed = [k for k in sorted(set(old) | set(new)) if old.get(k) != new.get(k)]
    for k in changed:
        print(old.get(k), "->", new.get(k), k)
    print(f"{len(old)} / {len(new)} kernels, {len(changed)} with different resources")
    sys.exit(1 if changed else 0)
rows = read(sys.argv[1])
print(len(rows), "kernels; scratch histogram:", dict(collections.Counter(v[0] for v in rows.values())))
for pat in sys.argv[2:]:
    for k, v in rows.items():
        if pat in k:
            print(f"scratch {v[0]:4d}  vgpr {v[1]:3d}  agpr {v[2]:3d}  sgpr {v[3]:3d}  occ {v[4]}  {k}")
