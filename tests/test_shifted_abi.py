"""Build-time and host-only checks of multi-shift CG (cgx_solve_shifted): the argument check without a context, the header
constant and its Python mirror, and the register report of every kernel in csrc/cgx_shift.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_null_context_is_bad_arg(pkg):
    L = pkg.cgx.lib()
    sig = np.zeros(2)
    X = np.zeros((2, 8))
    dp = C.POINTER(C.c_double)
    assert L.cgx_solve_shifted(None, 2, sig.ctypes.data_as(dp), X.ctypes.data_as(dp), 8, None) == 1


def test_max_shifts_in_header_and_binding(pkg):
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    m = re.search(r"#define\s+CGX_MAX_SHIFTS\s+(\d+)", text)
    assert m and int(m.group(1)) == 16
    assert pkg.cgx.MAX_SHIFTS == 16
    assert "cgx_solve_shifted" in pkg.cgx.EXPORTS and hasattr(pkg.CGSolver, "solve_shifted")


def _resources(src):
    """Per kernel: the compiler's resource report (-Rpass-analysis=kernel-resource-usage), names demangled."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "conjugate-gradient_amd", "csrc", src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?):\s*(.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if "Name" in k:
            cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
        elif cur is not None:
            cur[k] = v
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_shift_kernels_never_spill():
    rows = [r for r in _resources("cgx_shift.hip") if "cgx::" in r["name"]]
    update = [r for r in rows if "k_shift_update" in r["name"]]
    assert len(update) == 5, [r["name"] for r in rows]   # widths 1, 2, 4, 8, 16
    assert len(rows) == 7, [r["name"] for r in rows]     # + begin, close (the norms: k_column_norms, cgx_multi.hip)
    for r in rows:
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
