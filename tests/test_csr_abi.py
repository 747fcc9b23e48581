"""CPU checks of the opt-in CSR storage (include/cgx.h CGX_MATRIX_CSR): the C ABI, the Python binding
and the register budget of every k_spmv_csr instantiation (gfx950 cross-compile, no GPU needed)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cgx.h")
SRC = os.path.join(ROOT, "conjugate-gradient_amd", "csrc", "cgx_csr.hip")
NEW = ("cgx_set_matrix_csr", "cgx_get_matrix_nnz")


def test_format_constant(pkg):
    text = open(HDR).read()
    assert re.search(r"CGX_MATRIX_CSR\s*=\s*2\b", text)
    assert pkg.cgx.MATRIX_CSR == 2 and pkg.MATRIX_CSR == 2


def test_prototypes_exports_and_symbols(pkg):
    text = open(HDR).read()
    assert re.search(r"cgx_status\s+cgx_set_matrix_csr\(cgx_ctx \*ctx, int n, const long long \*row_ptr, const int \*col_idx,"
                     r"\s*const double \*vals\);", text)
    assert re.search(r"cgx_status\s+cgx_get_matrix_nnz\(const cgx_ctx \*ctx, int local_shard, long long \*nnz\);", text)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.cgx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in pkg.cgx.EXPORTS
        assert re.search(r"\bT %s\b" % name, out), name


def test_python_methods_exist(pkg):
    for name in ("set_matrix_csr", "matrix_nnz"):
        assert callable(getattr(pkg.CGSolver, name))


def test_csr_kernels_do_not_spill(tmp_path):
    """Every k_spmv_csr<MODE, L> (3 modes x 7 lane counts) keeps its registers: no VGPR / SGPR spill, no scratch."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "include"), "-c", SRC, "-o", str(tmp_path / "csr.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        if "k_spmv_csr" not in name:
            continue
        m = re.search(r"k_spmv_csrILi(\d+)ELi(\d+)E", name)
        assert m, name
        key = (int(m.group(1)), int(m.group(2)))
        stats = {k: int(v) for k, v in re.findall(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", b)}
        assert stats.get("VGPRs Spill") == 0 and stats.get("SGPRs Spill") == 0, (key, stats)
        assert stats.get("ScratchSize [bytes/lane]") == 0, (key, stats)
        seen[key] = stats
    assert set(seen) == {(mode, L) for mode in (0, 1, 2) for L in (1, 2, 4, 8, 16, 32, 64)}, sorted(seen)


@pytest.mark.parametrize("flags", [["--csr", "--banded"], ["--banded", "--csr"]])
def test_cli_csr_with_banded_is_a_usage_error(pkg, flags):
    exe = os.path.join(ROOT, "conjugate-gradient_amd", "cgsolver")
    r = subprocess.run([exe, "64", "/dev/null"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage:" in r.stderr and "--csr" in r.stderr
