"""Build-time and host-only checks of the multi right-hand-side entry points (cgx_solve_multi, cgx_probe_gemv_multi):
argument checks without a context, the header constant, and the register report of every kernel in csrc/cgx_multi.hip."""
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
    b = np.zeros(8)
    y = np.zeros(8)
    dp = b.ctypes.data_as(C.POINTER(C.c_double))
    yp = y.ctypes.data_as(C.POINTER(C.c_double))
    assert L.cgx_solve_multi(None, 1, dp, 8, yp, 8, None) == 1
    assert L.cgx_probe_gemv_multi(None, 1, dp, 8, yp, 8, dp) == 1


def test_max_rhs_in_header(pkg):
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    m = re.search(r"#define\s+CGX_MAX_RHS\s+(\d+)", text)
    assert m and int(m.group(1)) == 16
    assert pkg.cgx.MAX_RHS == 16


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
def test_multi_kernels_never_spill():
    rows = [r for r in _resources("cgx_multi.hip") if "cgx::" in r["name"]]
    gemv = [r for r in rows if "k_multi_gemv" in r["name"]]
    assert len(gemv) == 10, [r["name"] for r in rows]   # widths 1, 2, 4, 8, 16, plain and fused
    assert len(rows) == 15, [r["name"] for r in rows]   # + update, init, close, the column norms with and without sigma
    for r in rows:
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
