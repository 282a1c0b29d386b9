#!/usr/bin/env python
"""Guard for the counted-wait kernels (tail2_h8_kernel and its C = 128 member tail128_h8_kernel, ring3_h8_kernel: DESIGN 3.1g).  Their speed -- not their results -- depends on two
things the compiler is free to change: that it leaves the `s_waitcnt vmcnt(N)` of the source alone, and that it does not add its own
`vmcnt(0)` inside the tile loop (it does for LDS reads without a TBAA tag and for tracked global loads once LDS-DMAs are interleaved).  This
script disassembles the gfx950 code objects of libslu_hip.so and reports, per instantiation, the vmcnt values in the tile loop; it exits
non-zero when a loop contains more `vmcnt(0)` than the first-tile branches account for, or when an instruction reads the destination of
one of the kernels' untracked (inline-asm) register loads before a vmcnt wait has RETIRED that load (that one WOULD be a wrong result): all
vector-memory operations are tracked in issue order and `vmcnt(N)` retires all but the N youngest, so a compiler-inserted move or spill of such
a register behind a counted wait with N > 0 is caught too.  The scan is linear over the disassembly (not branch-aware).

    python tools/check_counted_waits.py [path/to/libslu_hip.so] [--kernels REGEX]

--kernels REGEX scans the kernels whose (mangled) name matches REGEX as well.  gemm1x1_h8_kernel (gemm1x1_h8.hip; not its A/B form
gemm1x1_h8_kernel_v1) has rules of its own: its residual epilogue must not wait in full, so every `vmcnt(0)` has to be, by what follows it
within three instructions, one of the set-up (a `ds_write` of an epilogue constant: the tile loops fill LDS by DMA alone), the chunk wait of a
ring of depth 2 (D = 2: `vmcnt(0)`, `lgkmcnt(0)`, `s_barrier`) or the exit's (`s_endpgm`, or the branch to it from the first of the kernel's
two tile loops); it holds no FLAT operation (they count in lgkmcnt as well) and no scratch access; the untracked-load rule applies as above.
The A/B form is listed and not judged.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ap = argparse.ArgumentParser()
ap.add_argument("so", nargs="?", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semanticlidarunc_amd", "libslu_hip.so"))
ap.add_argument("--kernels", default=None, help="regular expression: scan these kernels too")
args = ap.parse_args()
so = os.path.abspath(args.so)
EXTRA = re.compile(args.kernels) if args.kernels else None
GEMM = re.compile(r"gemm1x1_h8_kernelILi(\d+)ELi(\d+)ELi(\d+)E")      # <MB, KC, D>; the _v1 form's mangled name continues with "_v1"
bad = 0
with tempfile.TemporaryDirectory() as tmp:
    local = os.path.join(tmp, "lib.so")
    shutil.copy(so, local)                                  # llvm-objdump --offloading writes the bundles next to its input
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
        name, waits, nbar = None, [], 0
        gemm, recent, unexplained, forbidden = None, [], [], 0      # the GEMM's rules
        vm_ops = []        # vector-memory operations issued so far in program order: the destination registers of an untracked register
                           # load, or an empty set for anything else that counts in vmcnt (stores, LDS-DMA, tracked loads, atomics)
        def pending_regs():
            r = set()
            for regs in vm_ops:
                r |= regs
            return r
        def flush():
            global bad, forbidden
            if name is None:
                return
            if "gemm1x1_h8_kernel_v1" in name:      # the A/B form keeps the full waits of its residual loads: reported, not judged
                print(f"{name[:90]:90s} barriers {nbar:2d}  counted {sorted(set(w for w in waits if w > 0))}  vmcnt(0) x{sum(1 for w in waits if w == 0)}   (A/B form)")
                return
            if gemm:
                for u in unexplained:
                    if u is not None:      # never followed by a barrier or the end of the program
                        forbidden += 1
                        print(f"{name[:90]}: {u}   <-- a full wait that is neither the set-up's, a D = 2 chunk wait nor the exit's")
                counted = sorted(set(w for w in waits if w > 0))
                flag = "" if not forbidden else f"   <-- {forbidden} full wait(s) / FLAT / scratch operation(s) in the GEMM"
                if flag:
                    bad += 1
                print(f"{name[:90]:90s} barriers {nbar:2d}  counted {counted}  vmcnt(0) x{sum(1 for w in waits if w == 0)}{flag}")
                return
            inner = [w for w in waits]
            zeros = sum(1 for w in inner if w == 0)
            counted = [w for w in inner if w > 0]
            # expected vmcnt(0): set-up (<= 6), one per first-tile position (<= positions), the kernel's exit, RESWAIT == 0 forms (<= 1)
            limit = 6 + max(1, nbar) + 2
            flag = "" if zeros <= limit and counted else "   <-- more vmcnt(0) than the first-tile branches explain" if counted else "   <-- no counted wait left"
            if flag:
                bad += 1
            print(f"{name[:90]:90s} barriers {nbar:2d}  counted {sorted(set(counted))}  vmcnt(0) x{zeros}{flag}")
        for line in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                flush()
                name = m.group(1) if any(k in m.group(1) for k in ("tail2_h8_kernel", "tail128_h8_kernel", "ring3_h8_kernel")) else None
                if name is None and EXTRA and EXTRA.search(m.group(1)):
                    name = m.group(1)
                gemm = GEMM.search(name) if name and EXTRA else None
                recent, unexplained, forbidden = [], [], 0
                waits, nbar = [], 0
                vm_ops.clear()
                continue
            if name is None:
                continue
            ins = line.split("//")[0]
            if gemm and ins.strip():
                op = ins.split()[0]
                if op.startswith(("flat_", "scratch_")):
                    forbidden += 1
                    print(f"{name[:90]}: {ins.strip()[:80]}   <-- FLAT / scratch operation in the GEMM")
                # a full wait stays "unexplained" until, within the next three instructions, a ds_write, an s_barrier (D = 2 only), s_endpgm
                # or a branch follows
                if op.startswith(("ds_write", "s_endpgm", "s_branch", "s_cbranch")) or (op == "s_barrier" and int(gemm.group(3)) == 2):
                    for u in recent:
                        unexplained[u[1]] = None
                recent = [(n - 1, k) for n, k in recent if n > 1]
                if re.search(r"s_waitcnt\s+vmcnt\(0\)", ins):
                    unexplained.append(ins.strip())
                    recent.append((3, len(unexplained) - 1))
            w = re.search(r"s_waitcnt\s+vmcnt\((\d+)\)", ins)
            if w:
                n = int(w.group(1))
                waits.append(n)
                # vmcnt(N) retires everything but the N YOUNGEST vector-memory operations: their destinations stay pending
                del vm_ops[:max(0, len(vm_ops) - n)]
            if "s_barrier" in ins:
                nbar += 1
            # the untracked register loads (inline asm, SGPR base + VGPR offset): nothing may read their destination before a wait retires them
            m2 = re.search(r"global_load_dwordx[24]\s+v\[(\d+):(\d+)\],\s*v\d+,\s*s\[", ins)
            if m2:
                vm_ops.append(set(range(int(m2.group(1)), int(m2.group(2)) + 1)))
                continue
            if re.search(r"\b(global_load|global_store|global_atomic|buffer_load|buffer_store|buffer_atomic|scratch_load|scratch_store)", ins):
                vm_ops.append(set())                       # counts in vmcnt, holds no untracked destination
                continue
            pend = pending_regs()
            if pend:
                ops = ins.strip().split(None, 1)
                srcs = ops[1].split(",", 1)[1] if len(ops) > 1 and "," in ops[1] else ""
                if ops and ops[0].startswith(("ds_write", "v_mfma", "s_")):
                    srcs = ops[1] if len(ops) > 1 else ""       # no destination operand first / accumulate in place
                used = set()
                for a, b, c in re.findall(r"v\[(\d+):(\d+)\]|\bv(\d+)\b", srcs):
                    used.update(range(int(a), int(b) + 1) if a else [int(c)])
                if used & pend:
                    print(f"{name[:90]}: {ins.strip()[:80]}   <-- reads a register of an untracked load that no vmcnt wait has retired yet")
                    bad += 1
                    for regs in vm_ops:
                        regs -= used
        flush()
sys.exit(1 if bad else 0)
