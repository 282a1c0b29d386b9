#!/usr/bin/env python
"""Development aid (no GPU): opcode histogram of every loop of one kernel in a gfx950 assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Isemanticlidarunc_amd/csrc --cuda-device-only -S \\
          -Rpass-analysis=kernel-resource-usage semanticlidarunc_amd/csrc/head_mc_h8.hip -o head.s
    python tools/isa_loop_hist.py head.s head_mc_h8_kernelILi2ELi3EE [FIRST-LAST REGEX]

A loop is a backward branch: the lines from its target label to the branch.  Nested loops and loops with several back edges are printed
once per back edge, innermost first by position.  With FIRST-LAST REGEX the lines of that range (numbered from the kernel's label) that
match REGEX are printed too, e.g. `440-820 'global_load|s_waitcnt|v_mfma'` to see where a wait sits relative to the loads."""
import collections
import re
import sys

PREFIXES = ("v_exp_f32", "v_log_f32", "v_cndmask", "s_and_saveexec", "s_cbranch", "v_mfma", "global_load", "global_store", "s_load", "s_waitcnt",
            "v_rcp", "v_div", "v_cvt", "v_fma", "v_mul", "v_add", "v_pk")


def kernel_body(path, key):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % re.escape(key), l))
    # up to the function's end label: a kernel may hold an early-exit s_endpgm, or two whole loops with one each (gemm1x1_h8_kernel)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")) - 1
    return lines[start:end + 1]


def histogram(body, first, last):
    ops = [l.split()[0] for l in body[first:last + 1] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    count = collections.Counter(ops)
    vector = sum(n for o, n in count.items() if o.startswith("v_"))
    return len(ops), vector, {p: sum(n for o, n in count.items() if o.startswith(p)) for p in PREFIXES}


def main(argv):
    body = kernel_body(argv[1], argv[2])
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    print(f"{argv[2]}: {len(body)} lines")
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            n, vector, picked = histogram(body, labels[m.group(1)], i)
            print(f"loop {m.group(1)} lines {labels[m.group(1)]}-{i}: {n} instructions, {vector} v_*, "
                  + ", ".join(f"{k}={v}" for k, v in picked.items() if v))
    if len(argv) > 4:
        first, last = map(int, argv[3].split("-"))
        n, vector, picked = histogram(body, first, last)
        print(f"lines {first}-{last}: {n} instructions, {vector} v_*, " + ", ".join(f"{k}={v}" for k, v in picked.items() if v))
        for i in range(first, min(last, len(body) - 1) + 1):
            if re.search(argv[4], body[i]):
                print(i, body[i])


if __name__ == "__main__":
    main(sys.argv)
