"""Build-time and host-only checks of the preconditioned multi right-hand-side entry point (cgx_solve_multi_pc, DESIGN.md
section 16): argument checks without a context, the prototype, the Python method, and the register report of every kernel in
csrc/cgx_multi_pc.hip."""
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
    assert L.cgx_solve_multi_pc(None, 1, dp, 8, yp, 8, None) == 1
    assert L.cgx_probe_multi_pc_apply(None, 1, dp, 8, yp, 8) == 1


def test_prototype_in_header():
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    proto = r"cgx_status\s+cgx_solve_multi_pc\(cgx_ctx \*ctx, int nrhs, const double \*B, long ldb, double \*X, long ldx, cgx_result \*res\);"
    assert re.search(proto, text)
    assert re.search(proto.replace("_pc", ""), text)   # the same arguments as cgx_solve_multi


def test_python_method(pkg):
    assert callable(pkg.cgx.CGSolver.solve_multi_pc)
    assert callable(pkg.cgx.CGSolver.solve_multi)


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
def test_multi_pc_kernels_never_spill():
    rows = [r for r in _resources("cgx_multi_pc.hip") if "cgx::" in r["name"]]
    names = [r["name"] for r in rows]
    for kernel, count in (("k_multi_gemv_pc", 5), ("k_multi_update_jac", 2), ("k_multi_lr_update", 2), ("k_multi_lr_apply", 5),
                          ("k_multi_close_pc", 1)):
        assert sum(kernel in nm for nm in names) == count, (kernel, names)
    assert len(rows) == 15, names
    for r in rows:
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= 160 * 1024, r
