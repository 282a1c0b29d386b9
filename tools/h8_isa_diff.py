#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 code of two builds (development aid for refactors that must not change what the compiler emits):

    python tools/h8_isa_diff.py OLD NEW [--match SUBSTR] [--launched names.json|stats.csv ...]

OLD / NEW: a libslu_hip.so (its code objects are extracted the way tools/check_counted_waits.py does) or one device code object
(`hipcc --cuda-device-only -c`).  For every kernel whose name contains SUBSTR (default "h8") the instruction text is compared with comments stripped; the
literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the PC-relative address of a global: it moves with the layout of the code
object, not with the kernel) is masked.  Verdicts: `same`; `commuted` = same length, same opcode at every position, the operands of the
differing lines permuted; `CHANGED` with both instruction counts.  --launched: kernel names as rocprofv3 prints them (a JSON object keyed
by name or a --stats CSV); a CHANGED kernel of that set, or (default match only) any CHANGED ring3_h8_kernel / tail2_h8_kernel, makes the
exit status 1.  For the fp32-storage conv / wgrad kernels: --match kernel --launched profiles/r05/coverage_recorded_names.json --launched
profiles/r03/train_kernel_stats.csv.  For any other refactor: --match kernel (every kernel of the library); a kernel the change renamed shows as
`only in OLD` / `only in NEW` and is compared pairwise with kernels() and verdict() of this module (profiles/r16)."""
import collections
import csv
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def short(demangled):      # "void (anonymous namespace)::k<1, 2>((anonymous namespace)::Args)" -> "k<1, 2>"
    s = demangled.replace("(anonymous namespace)::", "").replace("void ", "", 1).strip()
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def kernels(path, match="h8"):
    """{short name: [instruction lines]} of the kernels of a library or code object whose name contains `match`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "in.bin")
        shutil.copy(path, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "amdgcn" in f] or [local]
        for obj in objs:
            asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", obj], check=True, capture_output=True, text=True).stdout
            cur, pcrel = None, 0
            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(short(m.group(1)), []) if match in m.group(1) else None
                    continue
                ins = " ".join(line.split("//")[0].split())
                if cur is None or not ins or ins == "...":      # "...": objdump's mark for the zero padding between two symbols, not an instruction
                    continue
                if ins.startswith("s_getpc_b64"):
                    pcrel = 2
                elif pcrel and ins.startswith(("s_add_u32", "s_addc_u32")):
                    ins, pcrel = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "PCREL", ins), pcrel - 1
                cur.append(ins)
    return out


def verdict(a, b):
    if a == b:
        return "same"
    split = lambda i: (i.split(None, 1)[0], sorted(re.split(r"[ ,]+", i.split(None, 1)[1])) if " " in i else [])
    if len(a) == len(b) and all(x == y or split(x) == split(y) for x, y in zip(a, b)):
        return f"commuted ({sum(x != y for x, y in zip(a, b))} lines)"
    same_ops = collections.Counter(i.split()[0] for i in a) == collections.Counter(i.split()[0] for i in b)
    return f"CHANGED {len(a)} -> {len(b)} instructions" + (", same opcode multiset" if same_ops else "")


def main():
    args, launched, match = sys.argv[1:], set(), "h8"
    if "--match" in args:
        i = args.index("--match")
        match = args[i + 1]
        del args[i:i + 2]
    while "--launched" in args:
        i = args.index("--launched")
        f = args[i + 1]
        del args[i:i + 2]
        names = json.load(open(f)) if f.endswith(".json") else [r["Name"] for r in csv.DictReader(open(f))]
        launched |= {short(n) for n in names}
    old, new = kernels(args[0], match), kernels(args[1], match)
    always = ("ring3_h8_kernel", "tail2_h8_kernel") if match == "h8" else ()
    bad, tally = 0, collections.Counter()
    for name in sorted(set(old) | set(new)):
        v = verdict(old[name], new[name]) if name in old and name in new else ("only in OLD" if name in old else "only in NEW")
        must = name in launched or name.startswith(always)
        tally[v.split()[0]] += 1
        if v != "same":
            print(f"{'launched ' if must else '         '}{name}: {v}")
        if must and not v.startswith(("same", "commuted")):
            bad += 1
    print(f"{len(old)} / {len(new)} {match} kernels: {dict(tally)}; {bad} launched{', ring3 or tail2' if always else ''} kernels changed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
