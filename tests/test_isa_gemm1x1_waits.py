"""CPU: gemm1x1_h8_kernel under tools/check_counted_waits.py (--kernels), on the BUILT library.  The residual epilogue issues its loads ahead
and waits with counted `vmcnt`, which the compiler is free to undo: a full wait that is neither the set-up's, the chunk wait of the depth-2
ring nor the exit's, a FLAT or scratch operation (the former counts in lgkmcnt too, the latter is a spill), or an instruction that reads the
destination of an untracked residual load before a wait has retired it (that one would be a wrong result) fails the check.  The A/B form
(gemm1x1_h8_kernel_v1, SLU_GEMM1X1_RES_AHEAD=0) keeps its full waits and is listed only."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs ROCm's llvm-objdump")
def test_gemm_epilogue_holds_only_counted_waits():
    lib = os.path.join(ROOT, "semanticlidarunc_amd", "libslu_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libslu_hip.so not built")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_counted_waits.py"), lib, "--kernels", "gemm1x1_h8_kernel"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows = {ln.split()[0]: ln for ln in r.stdout.splitlines() if "gemm1x1_h8_kernel" in ln and "barriers" in ln}
    judged = {n: ln for n, ln in rows.items() if "_v1" not in n}
    assert len(judged) == 2 and len(rows) == 4, sorted(rows)
    for n, ln in judged.items():
        counted = [int(v) for v in re.search(r"counted \[([^\]]*)\]", ln).group(1).split(",") if v.strip()]
        # the residual wait at the top of the epilogue is vmcnt(NPIECE): 8 pieces per wave and chunk in <4, 4, 2>, 6 in <2, 4, 3>
        assert (8 if "ILi4ELi4ELi2E" in n else 6) in counted, ln
    # the two families the tool scans by default are still in the report
    names = [ln.split()[0] for ln in r.stdout.splitlines() if "_h8_kernel" in ln and "barriers" in ln]
    assert sum("tail2_h8_kernel" in n for n in names) == 5 and sum("ring3_h8_kernel" in n for n in names) == 9, names
