#!/usr/bin/env python
"""Development aid: per-launch table from a rocprofv3 kernel trace of bench.py (profiles/r10, r20): for every kernel whose name matches
REGEX, its launches by position in the step (launch i of a kernel with k launches per step is position i % k), mean / standard deviation /
min / max over the steps.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bench -- python3 bench.py --gpus 1 --steps 10 --warmup 3 ...
    python tools/trace_per_launch.py LABEL DIR 13 [REGEX]

Default REGEX: the kernels of the 128-channel block tails (fused and as two launches)."""
import csv
import glob
import re
import statistics
import sys

label, d, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
pat = re.compile(sys.argv[4] if len(sys.argv) > 4 else
                 r"tail128_h8_kernel|tail2_h8_kernel|tail_h8_kernel|conv_h8_kernel<2, 2, 1|gemm1x1_h8_kernel<2, 4, 3>|conv1x1_h8_kernel<4, 1>")
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
by = {}
for r in rows:
    n = r["Kernel_Name"]
    if pat.search(n):
        by.setdefault(n, []).append(r)
for n, rs in sorted(by.items()):
    per = len(rs) // steps
    short = re.sub(r"^void |\(anonymous namespace\)::|\(.*\)$", "", n)
    print(f"{label} {short}: {len(rs)} launches, {per} per step" + ("" if per * steps == len(rs) else "  (NOT a multiple of the steps)"))
    if per == 0:
        continue
    rs = rs[len(rs) - per * steps:]
    for p in range(per):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs[p::per]]
        g = rs[p].get("Grid_Size", rs[p].get("Grid_Size_X", "?"))
        print(f"   position {p} grid {g:>8}: mean {statistics.mean(us):8.1f} us  stdev {statistics.pstdev(us):6.1f}  min {min(us):8.1f}  max {max(us):8.1f}  n={len(us)}")
