"""ctypes binding of libcgx.so (include/cgx.h) plus a Python mirror of the reference's CGSolver.

Only test/bench plumbing lives here: every number is computed by the HIP library.  There is no CPU
fallback: if libcgx.so is missing or no MI355X is visible, the calls raise.
Reference interface mirrored: class CGSolver, code/MPI/cg.hh:11-57 and code/CUDA/cg.hh:13-45.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libcgx.so")
UNIQUE_ID_BYTES = 128

IPC_HANDLE_BYTES = 64
COMM_SELF, COMM_LOOPBACK, COMM_RCCL, COMM_P2P = 0, 1, 2, 3
MATRIX_DENSE, MATRIX_BANDED = 0, 1   # BANDED: opt-in fast path, not the reference's storage (include/cgx.h)
MATRIX_CSR = 2                       # CSR: opt-in general sparse row block, not the reference's storage
MAX_DIAGONALS = 64

EXPORTS = [
    "cgx_config_init", "cgx_comm_unique_id", "cgx_create", "cgx_destroy", "cgx_last_error", "cgx_status_string",
    "cgx_get_comm_info", "cgx_get_gemv_plan", "cgx_get_resident_record", "cgx_p2p_export", "cgx_p2p_import", "cgx_p2p_selftest",
    "cgx_partition", "cgx_generate_lap2d_matrix", "cgx_set_matrix_dense", "cgx_read_matrix",
    "cgx_init_source_term", "cgx_set_source_term", "cgx_set_max_iter", "cgx_set_tolerance", "cgx_get_size",
    "cgx_get_matrix_format",
    "cgx_solve", "cgx_solve_begin", "cgx_solve_steps", "cgx_solve_end", "cgx_get_gemv_samples",
    "cgx_get_update_samples",
    "cgx_probe_gemv", "cgx_probe_time_gemv", "cgx_probe_vector_ops", "cgx_probe_get_matrix_rows",
    "cgx_probe_get_source_term", "cgx_probe_set_fault_after", "cgx_probe_set_resident_limit", "cgx_probe_persistent_plan",
    "cgx_probe_parse_matrix_market", "cgx_probe_p2p_mailbox_to_host", "cgx_probe_fill_matrix_hash",
    "cgx_probe_set_p2p_epoch", "cgx_probe_get_p2p_epoch", "cgx_probe_p2p_host_mailboxes", "cgx_probe_resident_test",
    "cgx_solve_multi", "cgx_probe_gemv_multi", "cgx_solve_shifted", "cgx_solve_minres",
    "cgx_set_preconditioner", "cgx_get_preconditioner",
    "cgx_set_preconditioner_block", "cgx_get_preconditioner_block", "cgx_probe_get_precond_blocks",
    "cgx_set_matrix_csr", "cgx_get_matrix_nnz",
    "cgx_set_preconditioner_rank", "cgx_get_preconditioner_rank", "cgx_set_preconditioner_shift", "cgx_get_preconditioner_shift",
    "cgx_probe_get_precond_lowrank", "cgx_probe_precond_apply",
    "cgx_solve_multi_pc", "cgx_probe_multi_pc_apply",
    "cgx_lanczos", "cgx_trace_slq", "cgx_tridiag_quadrature",
    "cgx_lanczos_pc", "cgx_precond_logdet", "cgx_slq_probes", "cgx_trace_slq_pc",
    "cgx_tridiag_function", "cgx_apply_function", "cgx_probe_funm_combine",
    "cgx_tridiag_eigenvectors", "cgx_eigenpairs", "cgx_probe_eigs_basis", "cgx_probe_eigs_orthogonalise",
]
MAX_RHS = 16   # CGX_MAX_RHS: right-hand sides of one cgx_solve_multi call
MAX_LANCZOS_STEPS = 1024   # CGX_MAX_LANCZOS_STEPS
MAX_PROBES = 256           # CGX_MAX_PROBES
SLQ_LOG, SLQ_INV = 0, 1    # cgx_trace_slq's fn
FN_SQRT, FN_INVSQRT, FN_INV, FN_LOG, FN_EXP = 0, 1, 2, 3, 4   # CGX_FN_*: cgx_apply_function's and cgx_tridiag_function's fn
EIG_LARGEST, EIG_SMALLEST = 0, 1   # CGX_EIG_*: cgx_eigenpairs's which
MAX_EIGENPAIRS = 16                # CGX_MAX_EIGENPAIRS
EIGS_SLOT_CHUNK = 32               # kEigsChunk (csrc/cgx_kernels.h): basis slots per workgroup of the projection kernel
_EIG_NAMES = {"largest": EIG_LARGEST, "smallest": EIG_SMALLEST}
MAX_SHIFTS = 16   # CGX_MAX_SHIFTS: shifts of one cgx_solve_shifted call
MAX_MINRES_SHIFTS = 16   # CGX_MAX_MINRES_SHIFTS: shifts of one cgx_solve_minres call
PRECOND_NONE, PRECOND_JACOBI = 0, 1   # CGX_PRECOND_*: cgx_set_preconditioner
PRECOND_PIVCHOL = 2                   # the pivoted-Cholesky low-rank factor: one GPU, dense storage
MAX_PRECOND_RANK = 256                # CGX_MAX_PRECOND_RANK: cgx_set_preconditioner_rank
_PRECOND_NAMES = {None: PRECOND_NONE, "jacobi": PRECOND_JACOBI, "pivchol": PRECOND_PIVCHOL}
PRECOND_BLOCKS = (1, 2, 4, 8, 16, 32, 64, 128, 256)   # cgx_set_preconditioner_block


class Config(C.Structure):
    _fields_ = [
        ("struct_version", C.c_int), ("comm_mode", C.c_int), ("device", C.c_int), ("rank", C.c_int),
        ("nranks", C.c_int), ("unique_id", C.c_ubyte * UNIQUE_ID_BYTES), ("gemv_variant", C.c_int),
        ("lda_pad", C.c_int), ("check_every", C.c_int), ("profile_gemv", C.c_int), ("profile_update", C.c_int),
        ("p2p_mailbox_kib", C.c_int), ("p2p_timeout_ms", C.c_int), ("p2p_separate_exchange", C.c_int),
        ("matrix_format", C.c_int), ("profile_first", C.c_int), ("profile_markers", C.c_int),
        ("p2p_no_acquire_fence", C.c_int), ("p2p_tagged", C.c_int),
    ]


class Result(C.Structure):
    _fields_ = [
        ("iterations", C.c_int), ("converged", C.c_int), ("residual_prev", C.c_double),
        ("residual_last", C.c_double), ("x_norm", C.c_double), ("rel_residual", C.c_double),
        ("seconds_solve", C.c_double), ("seconds_loop", C.c_double), ("gemv_ms_avg", C.c_double),
        ("gemv_ms_min", C.c_double), ("gemv_launches", C.c_longlong), ("gemv_bytes", C.c_double),
        ("gemv_ms_median", C.c_double), ("gemv_ms_max", C.c_double), ("gemv_discarded", C.c_longlong),
        ("steps_device_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class CgxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("libcgx status %d: %s" % (status, msg))
        self.status = status


def build(force=False):
    """hipcc --offload-arch=gfx950 build of libcgx.so + cgsolver (cross-compiles without a GPU)."""
    args = ["make", "-C", _PKG, "-s"] + (["-B"] if force else []) + ["all"]
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def lib():
    """Load libcgx.so.  Raises OSError if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("libcgx.so not built (run `make -C conjugate-gradient_amd` or __graft_entry__.build()); "
                          "the product path has no CPU fallback")
        # torch first, if it is there: libcgx then binds to the one HIP / RCCL runtime torch ships instead of bringing
        # /opt/rocm's as a second one into the process -- with two, whichever comes second may see no device (seen on the GPU
        # box when the library had been loaded before torch).  CGX_NO_TORCH=1 keeps torch out (the no-torch dev tools).
        if "torch" not in sys.modules and os.environ.get("CGX_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except Exception:   # noqa: BLE001 -- a box without torch: /opt/rocm's runtime alone is fine
                pass
        L = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int)
        vp = C.c_void_p
        L.cgx_config_init.argtypes = [C.POINTER(Config)]
        L.cgx_config_init.restype = None
        L.cgx_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
        L.cgx_create.argtypes = [C.POINTER(vp), C.POINTER(Config)]
        L.cgx_destroy.argtypes = [vp]
        L.cgx_last_error.argtypes = [vp]
        L.cgx_last_error.restype = C.c_char_p
        L.cgx_status_string.argtypes = [C.c_int]
        L.cgx_status_string.restype = C.c_char_p
        L.cgx_get_comm_info.argtypes = [vp, ip, ip, ip, C.c_char_p]
        L.cgx_get_gemv_plan.argtypes = [vp, C.c_int, ip]
        L.cgx_get_resident_record.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.cgx_p2p_export.argtypes = [vp, C.POINTER(C.c_ubyte)]
        L.cgx_p2p_import.argtypes = [vp, C.POINTER(C.c_ubyte)]
        L.cgx_p2p_selftest.argtypes = [vp, C.c_int, ip]
        L.cgx_partition.argtypes = [C.c_int, C.c_int, ip, ip]
        L.cgx_generate_lap2d_matrix.argtypes = [vp, C.c_int]
        L.cgx_set_matrix_dense.argtypes = [vp, dp, C.c_long, C.c_int]
        L.cgx_read_matrix.argtypes = [vp, C.c_char_p]
        L.cgx_init_source_term.argtypes = [vp, C.c_double]
        L.cgx_set_source_term.argtypes = [vp, dp]
        L.cgx_set_max_iter.argtypes = [vp, C.c_int]
        L.cgx_set_tolerance.argtypes = [vp, C.c_double]
        L.cgx_get_size.argtypes = [vp, ip, ip]
        L.cgx_get_matrix_format.argtypes = [vp, C.c_int, ip, ip, ip, dp]
        L.cgx_set_matrix_csr.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), ip, dp]
        L.cgx_get_matrix_nnz.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong)]
        L.cgx_solve.argtypes = [vp, dp, C.POINTER(Result)]
        L.cgx_solve_begin.argtypes = [vp, dp]
        L.cgx_solve_steps.argtypes = [vp, C.c_int, ip]
        L.cgx_solve_end.argtypes = [vp, dp, C.POINTER(Result)]
        L.cgx_get_gemv_samples.argtypes = [vp, dp, C.c_int, ip]
        L.cgx_get_update_samples.argtypes = [vp, dp, C.c_int, ip]
        L.cgx_probe_gemv.argtypes = [vp, dp, dp, dp]
        L.cgx_probe_time_gemv.argtypes = [vp, C.c_int, dp]
        L.cgx_probe_vector_ops.argtypes = [vp, C.c_int, C.c_double, C.c_double, dp, dp, dp, dp, dp]
        L.cgx_probe_get_matrix_rows.argtypes = [vp, C.c_int, dp, ip, ip]
        L.cgx_probe_get_source_term.argtypes = [vp, C.c_int, dp]
        L.cgx_probe_set_fault_after.argtypes = [vp, C.c_int]
        L.cgx_probe_set_resident_limit.argtypes = [vp, C.c_int]
        L.cgx_probe_persistent_plan.argtypes = [C.c_int, C.c_int, C.c_long, C.c_int, C.POINTER(C.c_long)]
        L.cgx_probe_p2p_mailbox_to_host.argtypes = [vp]
        L.cgx_probe_fill_matrix_hash.argtypes = [vp, C.c_ulonglong, C.c_int, C.c_double]
        L.cgx_probe_p2p_host_mailboxes.argtypes = [vp, C.c_char_p, C.c_int]
        L.cgx_probe_set_p2p_epoch.argtypes = [vp, C.c_int, C.c_ulonglong]
        L.cgx_probe_resident_test.argtypes = [vp, C.c_ulonglong, C.c_int]
        L.cgx_probe_get_p2p_epoch.argtypes = [vp, C.c_int, C.POINTER(C.c_ulonglong)]
        L.cgx_solve_multi.argtypes = [vp, C.c_int, dp, C.c_long, dp, C.c_long, C.POINTER(Result)]
        L.cgx_solve_multi_pc.argtypes = [vp, C.c_int, dp, C.c_long, dp, C.c_long, C.POINTER(Result)]
        L.cgx_probe_multi_pc_apply.argtypes = [vp, C.c_int, dp, C.c_long, dp, C.c_long]
        L.cgx_solve_shifted.argtypes = [vp, C.c_int, dp, dp, C.c_long, C.POINTER(Result)]
        L.cgx_solve_minres.argtypes = [vp, C.c_int, dp, dp, C.c_long, C.POINTER(Result)]
        L.cgx_lanczos.argtypes = [vp, C.c_int, C.c_int, dp, C.c_long, dp, dp, ip]
        L.cgx_trace_slq.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_ulonglong, dp, C.c_long, dp, dp, dp, dp]
        L.cgx_tridiag_quadrature.argtypes = [C.c_int, dp, dp, dp, dp]
        L.cgx_lanczos_pc.argtypes = [vp, C.c_int, C.c_int, dp, C.c_long, dp, dp, ip, dp]
        L.cgx_precond_logdet.argtypes = [vp, dp]
        L.cgx_slq_probes.argtypes = [vp, C.c_int, C.c_int, C.c_ulonglong, dp, C.c_long]
        L.cgx_trace_slq_pc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_ulonglong, dp, C.c_long, dp, dp, dp, dp, dp]
        L.cgx_tridiag_function.argtypes = [C.c_int, dp, dp, C.c_int, C.c_double, dp, dp]
        L.cgx_apply_function.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, dp, C.c_long, dp, C.c_long, ip, dp, dp]
        L.cgx_probe_funm_combine.argtypes = [vp, C.c_int, C.c_int, ip, dp, C.c_long, dp, dp, C.c_long]
        L.cgx_tridiag_eigenvectors.argtypes = [C.c_int, dp, dp, C.c_int, ip, dp, dp]
        L.cgx_eigenpairs.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, dp, C.c_ulonglong, dp, dp, C.c_long, dp, dp, ip, ip]
        L.cgx_probe_eigs_basis.argtypes = [vp, C.c_int, dp, dp, C.c_long, dp, dp, ip]
        L.cgx_probe_eigs_orthogonalise.argtypes = [vp, C.c_int, dp, C.c_long, dp, dp, dp]
        L.cgx_set_preconditioner.argtypes = [vp, C.c_int]
        L.cgx_get_preconditioner.argtypes = [vp, ip]
        L.cgx_set_preconditioner_block.argtypes = [vp, C.c_int]
        L.cgx_get_preconditioner_block.argtypes = [vp, ip]
        L.cgx_probe_get_precond_blocks.argtypes = [vp, C.c_int, dp]
        L.cgx_set_preconditioner_rank.argtypes = [vp, C.c_int]
        L.cgx_get_preconditioner_rank.argtypes = [vp, ip]
        L.cgx_set_preconditioner_shift.argtypes = [vp, C.c_double]
        L.cgx_get_preconditioner_shift.argtypes = [vp, dp, dp]
        L.cgx_probe_get_precond_lowrank.argtypes = [vp, ip, dp, dp]
        L.cgx_probe_precond_apply.argtypes = [vp, dp, dp]
        L.cgx_probe_gemv_multi.argtypes = [vp, C.c_int, dp, C.c_long, dp, C.c_long, dp]
        L.cgx_probe_parse_matrix_market.argtypes = [C.c_char_p, C.c_int, ip, ip, ip, ip, ip, ip, dp, C.c_long, C.c_char_p, C.c_int]
        for name in EXPORTS:
            fn = getattr(L, name)
            if fn.restype is C.c_int and name not in ("cgx_config_init",):
                fn.restype = C.c_int
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def partition(n, psize):
    """CGSolver::partition_matrix (code/MPI/cg.cc:236-268)."""
    s = (C.c_int * psize)()
    c = (C.c_int * psize)()
    st = lib().cgx_partition(n, psize, s, c)
    if st:
        raise CgxError(st, "cgx_partition")
    return list(s), list(c)


def comm_unique_id():
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    st = lib().cgx_comm_unique_id(buf)
    if st:
        raise CgxError(st, lib().cgx_last_error(None).decode(errors="replace"))
    return bytes(buf)


def tridiag_function(alpha, beta, fn, param=0.0):
    """Host only: f(T) e_1 for the Jacobi matrix with diagonal alpha (m entries) and off-diagonal beta (at least m - 1 entries, the
    rest is not read), f one of FN_SQRT, FN_INVSQRT, FN_INV, FN_LOG, FN_EXP (exp(-param theta)).  Returns (coef, theta_min,
    theta_max) (include/cgx.h cgx_tridiag_function)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    m = alpha.size
    if beta.size < m - 1:
        raise ValueError("beta must have at least m - 1 entries")
    coef = np.zeros(max(m, 1), dtype=np.float64)
    mm = np.full(2, np.nan)
    st = lib().cgx_tridiag_function(int(m), _dp(alpha), _dp(beta) if beta.size else None, int(fn), float(param), _dp(coef), _dp(mm))
    if st:
        raise CgxError(st, "cgx_tridiag_function: %s (eigenvalues of T in [%r, %r])"
                       % (lib().cgx_status_string(st).decode(errors="replace"), mm[0], mm[1]))
    return coef[:m], mm[0], mm[1]


def tridiag_eigenvectors(alpha, beta, index):
    """Host only: (theta, S) for the Jacobi matrix with diagonal alpha (m entries) and off-diagonal beta (at least m - 1 entries, the
    rest is not read): theta all m eigenvalues ascending, S[c] the unit eigenvector of the index[c]-th of them, its first component
    >= 0 (include/cgx.h cgx_tridiag_eigenvectors)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
    m = alpha.size
    if beta.size < m - 1:
        raise ValueError("beta must have at least m - 1 entries")
    theta = np.zeros(max(m, 1), dtype=np.float64)
    S = np.zeros((max(index.size, 1), max(m, 1)), dtype=np.float64)
    st = lib().cgx_tridiag_eigenvectors(int(m), _dp(alpha), _dp(beta) if beta.size else None, int(index.size),
                                        index.ctypes.data_as(C.POINTER(C.c_int)), _dp(theta), _dp(S))
    if st:
        raise CgxError(st, "cgx_tridiag_eigenvectors: %s" % lib().cgx_status_string(st).decode(errors="replace"))
    return theta[:m], S[:index.size, :m]


def parse_matrix_market(path, threads=0):
    """The library's Matrix-Market parser alone (host only): (m, n, symmetric, I, J, a) with 0-based indices in file order."""
    m, n, nz, sym = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    err = C.create_string_buffer(512)
    st = lib().cgx_probe_parse_matrix_market(os.fsencode(path), int(threads), C.byref(m), C.byref(n), C.byref(nz), C.byref(sym),
                                             None, None, None, 0, err, 512)
    if st:
        raise CgxError(st, err.value.decode(errors="replace"))
    I = np.zeros(nz.value, dtype=np.int32)
    J = np.zeros(nz.value, dtype=np.int32)
    a = np.zeros(nz.value, dtype=np.float64)
    st = lib().cgx_probe_parse_matrix_market(os.fsencode(path), int(threads), C.byref(m), C.byref(n), C.byref(nz), C.byref(sym),
                                             I.ctypes.data_as(C.POINTER(C.c_int)), J.ctypes.data_as(C.POINTER(C.c_int)), _dp(a),
                                             nz.value, err, 512)
    if st:
        raise CgxError(st, err.value.decode(errors="replace"))
    return m.value, n.value, bool(sym.value), I, J, a


class CGSolver:
    """Python mirror of the reference's CGSolver (same member names) over the C ABI.

    read_matrix / generate_lap2d_matrix / init_source_term / set_max_iter / tolerance / solve / m / n
    keep the reference's meaning; the constructor takes what `srun -n P` and MPI_Init gave the reference.
    """

    def __init__(self, comm_mode=COMM_SELF, nranks=1, rank=0, device=0, unique_id=None, gemv_variant=0,
                 lda_pad=-1, check_every=0, profile_gemv=False, p2p_timeout_ms=0, p2p_mailbox_kib=0,
                 p2p_separate_exchange=False, matrix_format=MATRIX_DENSE, profile_first=False,
                 profile_markers=False, p2p_no_acquire_fence=False, profile_update=False, p2p_tagged=False):
        L = lib()
        cfg = Config()
        L.cgx_config_init(C.byref(cfg))
        cfg.comm_mode = comm_mode
        cfg.nranks = nranks
        cfg.rank = rank
        cfg.device = device
        cfg.gemv_variant = gemv_variant
        cfg.lda_pad = lda_pad
        cfg.check_every = check_every
        cfg.profile_gemv = int(profile_gemv)   # n > 0: every n-th K1 launch is event-timed
        cfg.profile_update = 1 if profile_update else 0   # ... and the update kernel of the same iterations
        cfg.p2p_timeout_ms = p2p_timeout_ms
        cfg.p2p_mailbox_kib = p2p_mailbox_kib
        cfg.p2p_separate_exchange = 1 if p2p_separate_exchange else 0
        cfg.matrix_format = matrix_format
        cfg.profile_first = 1 if profile_first else 0
        cfg.profile_markers = 1 if profile_markers else 0
        cfg.p2p_no_acquire_fence = 1 if p2p_no_acquire_fence else 0
        cfg.p2p_tagged = 1 if p2p_tagged else 0
        if unique_id is not None:
            assert len(unique_id) == UNIQUE_ID_BYTES
            C.memmove(cfg.unique_id, bytes(unique_id), UNIQUE_ID_BYTES)
        self._h = C.c_void_p()
        st = L.cgx_create(C.byref(self._h), C.byref(cfg))
        if st:
            self._h = C.c_void_p()
            raise CgxError(st, L.cgx_last_error(None).decode(errors="replace"))
        self.nranks = nranks
        self.rank = rank

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, st):
        if st:
            raise CgxError(st, lib().cgx_last_error(self._h).decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().cgx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def comm_info(self):
        """What the transport really spans: {'comm_mode', 'ranks_wired', 'rank_seen', 'device_id'} (cgx_get_comm_info)."""
        mode, wired, seen = C.c_int(), C.c_int(), C.c_int()
        dev = C.create_string_buffer(32)
        self._check(lib().cgx_get_comm_info(self._h, C.byref(mode), C.byref(wired), C.byref(seen), dev))
        return {"comm_mode": mode.value, "ranks_wired": wired.value, "rank_seen": seen.value,
                "device_id": dev.value.decode(errors="replace")}

    def gemv_plan(self, local_shard=0):
        """The K1 launch shape of a local shard (cgx_get_gemv_plan): which kernel form runs on it."""
        v = (C.c_int * 8)()
        self._check(lib().cgx_get_gemv_plan(self._h, int(local_shard), v))
        return dict(zip(("variant", "R", "U", "waves", "light", "split", "grid", "ncols"), list(v)))

    def resident_record(self):
        """What the waits inside the persistent launches of the current / most recent solve cost (cgx_get_resident_record)."""
        v = (C.c_longlong * 10)()
        self._check(lib().cgx_get_resident_record(self._h, v))
        return dict(zip(("iterations", "watch_repeats", "gather_repeats", "launches", "wg0_first_wait_ticks", "wg0_longest_wait_ticks",
                         "max_first_wait_ticks", "max_longest_wait_ticks", "fallbacks", "persistent"), list(v)))

    # -- direct peer exchange wire-up (COMM_P2P) ------------------------------------------------------
    def p2p_export(self):
        buf = (C.c_ubyte * IPC_HANDLE_BYTES)()
        self._check(lib().cgx_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_import(self, handles):
        """handles: bytes of length nranks*64, rank order (every rank's p2p_export())."""
        assert len(handles) == self.nranks * IPC_HANDLE_BYTES
        buf = (C.c_ubyte * len(handles)).from_buffer_copy(handles)
        self._check(lib().cgx_p2p_import(self._h, buf))

    def p2p_selftest(self, rounds=32):
        ok = C.c_int()
        self._check(lib().cgx_p2p_selftest(self._h, int(rounds), C.byref(ok)))
        return bool(ok.value)

    def matrix_format(self, local_shard=0):
        """(format, offsets, device bytes) of a local shard's row block; offsets is [] for dense storage."""
        fmt, nd, nbytes = C.c_int(), C.c_int(), C.c_double()
        offs = (C.c_int * MAX_DIAGONALS)()
        self._check(lib().cgx_get_matrix_format(self._h, int(local_shard), C.byref(fmt), C.byref(nd), offs, C.byref(nbytes)))
        return fmt.value, list(offs[:nd.value]), nbytes.value

    def matrix_nnz(self, local_shard=0):
        """Entries stored for a local shard: rows*n (dense), ndiag*rows (banded), nnz (CSR)."""
        nnz = C.c_longlong()
        self._check(lib().cgx_get_matrix_nnz(self._h, int(local_shard), C.byref(nnz)))
        return nnz.value

    def set_matrix_csr(self, indptr, indices=None, data=None, n=None):
        """The global n x n matrix as CSR (0-based; columns strictly ascending within a row).  indptr may also be any object
        with .indptr / .indices / .data / .shape (a scipy.sparse CSR matrix, say); scipy itself is never imported."""
        if hasattr(indptr, "indptr") and hasattr(indptr, "indices") and hasattr(indptr, "data"):
            mat = indptr
            if n is None:
                n = int(mat.shape[0])
            indptr, indices, data = mat.indptr, mat.indices, mat.data
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if n is None:
            n = len(indptr) - 1
        self._check(lib().cgx_set_matrix_csr(self._h, int(n), indptr.ctypes.data_as(C.POINTER(C.c_longlong)),
                                             indices.ctypes.data_as(C.POINTER(C.c_int)), _dp(data)))

    # -- reference interface --------------------------------------------------------------------
    def generate_lap2d_matrix(self, size):
        self._check(lib().cgx_generate_lap2d_matrix(self._h, int(size)))

    def read_matrix(self, filename):
        self._check(lib().cgx_read_matrix(self._h, os.fsencode(filename)))

    def set_matrix_dense(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        assert A.ndim == 2 and A.shape[0] == A.shape[1]
        self._check(lib().cgx_set_matrix_dense(self._h, _dp(A), A.shape[1], A.shape[0]))

    def init_source_term(self, h):
        self._check(lib().cgx_init_source_term(self._h, float(h)))

    def set_source_term(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        self._check(lib().cgx_set_source_term(self._h, _dp(b)))

    def set_max_iter(self, max_iter):
        self._check(lib().cgx_set_max_iter(self._h, int(max_iter)))

    def tolerance(self, tol):
        self._check(lib().cgx_set_tolerance(self._h, float(tol)))

    def set_preconditioner(self, kind, block=1, rank=32, shift=0.0):
        """None (plain CG), "jacobi" or "pivchol": takes effect at the next solve (include/cgx.h cgx_set_preconditioner).  block > 1
        makes "jacobi" block Jacobi with the block x block diagonal blocks (cgx_set_preconditioner_block; 1 = point Jacobi).
        rank (1 ... MAX_PRECOND_RANK) and shift (0 = automatic, else positive and finite) belong to "pivchol", the rank-k pivoted
        Cholesky factor plus shift of a dense SPD matrix on one GPU (cgx_set_preconditioner_rank / _shift)."""
        if kind not in _PRECOND_NAMES:
            raise ValueError("preconditioner must be None, 'jacobi' or 'pivchol', not %r" % (kind,))
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in PRECOND_BLOCKS:
            raise ValueError("block must be one of %r, not %r" % (PRECOND_BLOCKS, block))
        if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or not 1 <= int(rank) <= MAX_PRECOND_RANK:
            raise ValueError("rank must be an integer 1 ... %d, not %r" % (MAX_PRECOND_RANK, rank))
        if isinstance(shift, bool) or not isinstance(shift, (int, float, np.integer, np.floating)) or not 0.0 <= float(shift) < float("inf"):
            raise ValueError("shift must be 0 (automatic) or positive and finite, not %r" % (shift,))
        self._check(lib().cgx_set_preconditioner(self._h, _PRECOND_NAMES[kind]))
        self._check(lib().cgx_set_preconditioner_block(self._h, int(block)))
        if kind == "pivchol":   # (another kind leaves the rank, the shift and the factor made with them as they are)
            self._check(lib().cgx_set_preconditioner_rank(self._h, int(rank)))
            self._check(lib().cgx_set_preconditioner_shift(self._h, float(shift)))

    def preconditioner_block(self):
        b = C.c_int()
        self._check(lib().cgx_get_preconditioner_block(self._h, C.byref(b)))
        return b.value

    def preconditioner_rank(self):
        k = C.c_int()
        self._check(lib().cgx_get_preconditioner_rank(self._h, C.byref(k)))
        return k.value

    def preconditioner_shift(self):
        """(the shift as set, the shift of the factor in use: 0.0 until a solve has made one)."""
        a, b = C.c_double(), C.c_double()
        self._check(lib().cgx_get_preconditioner_shift(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _probe_precond_lowrank(self):
        """Test hook: (pivots, L as an (n, rank) array, the shift in use) of the "pivchol" factor."""
        k = self.preconditioner_rank()
        piv = np.zeros(k, dtype=np.int32)
        L = np.zeros((self.n(), k), dtype=np.float64)
        d = C.c_double()
        self._check(lib().cgx_probe_get_precond_lowrank(self._h, piv.ctypes.data_as(C.POINTER(C.c_int)), _dp(L), C.byref(d)))
        return piv, L, d.value

    def _probe_precond_apply(self, r):
        """Test hook: z = P^-1 r through the loop's kernels."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (self.n(),):
            raise ValueError("r must have n entries")
        z = np.zeros_like(r)
        self._check(lib().cgx_probe_precond_apply(self._h, _dp(r), _dp(z)))
        return z

    def _probe_precond_blocks(self, local_shard=0):
        """Test hook: the block inverses of a local shard as an (n, block) array, row i = (D_b^-1)(i, s(i) : s(i) + block)."""
        W = np.zeros((self.n(), self.preconditioner_block()), dtype=np.float64)
        self._check(lib().cgx_probe_get_precond_blocks(self._h, int(local_shard), _dp(W)))
        return W

    @property
    def preconditioner(self):
        k = C.c_int()
        self._check(lib().cgx_get_preconditioner(self._h, C.byref(k)))
        return {v: n for n, v in _PRECOND_NAMES.items()}[k.value]

    def _size(self):
        m = C.c_int()
        n = C.c_int()
        self._check(lib().cgx_get_size(self._h, C.byref(m), C.byref(n)))
        return m.value, n.value

    def m(self):
        return self._size()[0]

    def n(self):
        return self._size()[1]

    def solve(self, x):
        """x: float64 array of length n, initial guess in / solution out.  Returns the result dict."""
        assert x.dtype == np.float64 and x.flags["C_CONTIGUOUS"] and x.size == self.n()
        res = Result()
        self._check(lib().cgx_solve(self._h, _dp(x), C.byref(res)))
        return res.as_dict()

    def _solve_block(self, entry, B, X):
        B = np.ascontiguousarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[1] == self.n(), B.shape
        X = np.zeros_like(B) if X is None else np.array(X, dtype=np.float64, copy=True, order="C")
        assert X.shape == B.shape, (X.shape, B.shape)
        k = B.shape[0]
        res = (Result * max(k, 1))()
        self._check(entry(self._h, int(k), _dp(B), int(B.shape[1]), _dp(X), int(X.shape[1]), res))
        return X, [res[j].as_dict() for j in range(k)]

    def solve_multi(self, B, X=None):
        """B: float64 array (k, n), one right-hand side per row; X: initial guesses of the same shape (None = zeros).
        Returns (X, [k result dicts]): k independent CG solves on the current matrix, one pass over A per iteration.
        Refuses a preconditioner: solve_multi_pc takes it."""
        return self._solve_block(lib().cgx_solve_multi, B, X)

    def solve_multi_pc(self, B, X=None):
        """solve_multi with the preconditioner that is set ("jacobi" with block 1, or "pivchol"): k independent preconditioned
        CG solves, one pass over A per iteration, the inverse diagonal / the factor shared with solve().  With no preconditioner
        set it is solve_multi, bit for bit."""
        return self._solve_block(lib().cgx_solve_multi_pc, B, X)

    def _probe_multi_pc_apply(self, R):
        """Test hook: R float64 (k, n); returns Z with Z[j] = M^-1 R[j] through the preconditioned multi-vector update kernels."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        assert R.ndim == 2 and R.shape[1] == self.n(), R.shape
        Z = np.zeros_like(R)
        self._check(lib().cgx_probe_multi_pc_apply(self._h, int(R.shape[0]), _dp(R), int(R.shape[1]), _dp(Z), int(Z.shape[1])))
        return Z

    def _solve_shifts(self, entry, shifts):
        sig = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
        k, n = sig.size, self.n()
        X = np.zeros((k, n), dtype=np.float64)
        res = (Result * max(k, 1))()
        self._check(entry(self._h, int(k), _dp(sig), _dp(X), int(n), res))
        return X, [res[j].as_dict() for j in range(k)]

    def solve_shifted(self, shifts):
        """shifts: sigma_j >= 0 (at most MAX_SHIFTS).  Returns (X, [result dicts]), X of shape (len(shifts), n): row j solves
        (A + sigma_j I) x = b for the current matrix and source term from a zero guess, all shifts in one Krylov sequence with
        one pass over A per iteration (multi-shift CG, cgx_solve_shifted)."""
        return self._solve_shifts(lib().cgx_solve_shifted, shifts)

    def solve_minres(self, shifts):
        """shifts: finite sigma_j of either sign (at most MAX_MINRES_SHIFTS).  Returns (X, [result dicts]), X of shape
        (len(shifts), n): row j solves (A + sigma_j I) x = b for the current matrix, taken as symmetric (it need not be definite),
        and source term from a zero guess, all shifts on one Lanczos recurrence with one pass over A per iteration (MINRES,
        cgx_solve_minres)."""
        return self._solve_shifts(lib().cgx_solve_minres, shifts)

    def lanczos(self, V0, steps):
        """V0: float64 array (k, n), one start vector per row (k <= MAX_RHS).  Returns (alpha, beta, steps_done): the coefficients
        of `steps` steps of the Lanczos recurrence on the current matrix from every start vector, one pass over A per step;
        alpha, beta of shape (k, steps), zero at t >= steps_done[j] (a column that reached an invariant subspace stops early)."""
        V0 = np.ascontiguousarray(V0, dtype=np.float64)
        assert V0.ndim == 2 and V0.shape[1] == self.n(), V0.shape
        k, steps = V0.shape[0], int(steps)
        alpha = np.zeros((max(k, 1), max(steps, 1)), dtype=np.float64)
        beta = np.zeros_like(alpha)
        done = np.zeros(max(k, 1), dtype=np.int32)
        self._check(lib().cgx_lanczos(self._h, int(k), steps, _dp(V0), int(V0.shape[1]), _dp(alpha), _dp(beta),
                                      done.ctypes.data_as(C.POINTER(C.c_int))))
        return alpha[:k, :steps], beta[:k, :steps], done[:k]

    def _trace_slq(self, fn, probes, steps, seed, Z):
        if Z is not None:
            Z = np.ascontiguousarray(Z, dtype=np.float64)
            assert Z.ndim == 2 and Z.shape[1] == self.n(), Z.shape
            probes = Z.shape[0]
        est, err = C.c_double(), C.c_double()
        per = np.zeros(max(int(probes), 1), dtype=np.float64)
        ritz = np.zeros(2, dtype=np.float64)
        self._check(lib().cgx_trace_slq(self._h, int(fn), int(probes), int(steps), int(seed), None if Z is None else _dp(Z),
                                        0 if Z is None else int(Z.shape[1]), C.byref(est), C.byref(err), _dp(per), _dp(ritz)))
        return {"estimate": est.value, "std_error": err.value, "per_probe": per[:int(probes)], "ritz_min": ritz[0], "ritz_max": ritz[1]}

    def logdet(self, probes=16, steps=100, seed=1, Z=None):
        """log det of the current (symmetric positive definite, dense) matrix by stochastic Lanczos quadrature: `probes` Rademacher
        vectors made by the library from `seed`, or the rows of Z; `steps` Lanczos steps each.  Returns a dict: estimate, std_error
        (sample standard deviation / sqrt(probes)), per_probe, ritz_min, ritz_max (the extreme Ritz values over all probes)."""
        return self._trace_slq(SLQ_LOG, probes, steps, seed, Z)

    def trace_inv(self, probes=16, steps=100, seed=1, Z=None):
        """tr(A^-1) of the current matrix, as logdet."""
        return self._trace_slq(SLQ_INV, probes, steps, seed, Z)

    def lanczos_pc(self, V0, steps):
        """lanczos with the preconditioner M that is set ("jacobi" with block 1, or "pivchol"): returns (alpha, beta, steps_done,
        eta2), the coefficients of the Jacobi matrix of M^-1/2 A M^-1/2 from the start vectors M^-1/2 V0[j] and eta2[j] =
        V0[j] . M^-1 V0[j] (include/cgx.h cgx_lanczos_pc).  With no preconditioner set it is lanczos, bit for bit, and eta2 =
        ||V0[j]||^2."""
        V0 = np.ascontiguousarray(V0, dtype=np.float64)
        assert V0.ndim == 2 and V0.shape[1] == self.n(), V0.shape
        k, steps = V0.shape[0], int(steps)
        alpha = np.zeros((max(k, 1), max(steps, 1)), dtype=np.float64)
        beta = np.zeros_like(alpha)
        done = np.zeros(max(k, 1), dtype=np.int32)
        eta2 = np.zeros(max(k, 1), dtype=np.float64)
        self._check(lib().cgx_lanczos_pc(self._h, int(k), steps, _dp(V0), int(V0.shape[1]), _dp(alpha), _dp(beta),
                                         done.ctypes.data_as(C.POINTER(C.c_int)), _dp(eta2)))
        return alpha[:k, :steps], beta[:k, :steps], done[:k], eta2[:k]

    def apply_function(self, B, fn, steps, param=0.0):
        """B: float64 array (k, n), one vector per row (k <= MAX_RHS); fn one of FN_SQRT, FN_INVSQRT, FN_INV, FN_LOG, FN_EXP
        (exp(-param A)).  Returns (X, info): X[j] ~ f(A) B[j] from `steps` Lanczos steps on the current matrix, one pass over A per
        step for all vectors (include/cgx.h cgx_apply_function); info = dict(steps_done, change, coef): the steps every column
        made, the convergence indicator and the coefficients of the Lanczos vectors, shape (k, steps)."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[1] == self.n(), B.shape
        k, steps = B.shape[0], int(steps)
        X = np.zeros((max(k, 1), B.shape[1]), dtype=np.float64)
        coef = np.zeros((max(k, 1), max(steps, 1)), dtype=np.float64)
        change = np.zeros(max(k, 1), dtype=np.float64)
        done = np.zeros(max(k, 1), dtype=np.int32)
        self._check(lib().cgx_apply_function(self._h, int(fn), float(param), int(k), steps, _dp(B), int(B.shape[1]), _dp(X),
                                             int(X.shape[1]), done.ctypes.data_as(C.POINTER(C.c_int)), _dp(change), _dp(coef)))
        return X[:k], {"steps_done": done[:k], "change": change[:k], "coef": coef[:k, :steps]}

    def _probe_funm_combine(self, Q, Cf, m):
        """Test hook: Q float64 (steps, k, n), Cf (k, steps), m k step counts; returns X (k, n) with X[j] = sum over t < m[j] of
        Cf[j, t] Q[t, j] from the combine kernel of apply_function."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        Cf = np.ascontiguousarray(Cf, dtype=np.float64)
        m = np.ascontiguousarray(m, dtype=np.int32)
        assert Q.ndim == 3 and Q.shape[2] == self.n() and Cf.shape == (Q.shape[1], Q.shape[0]) and m.shape == (Q.shape[1],)
        X = np.zeros((Q.shape[1], Q.shape[2]), dtype=np.float64)
        self._check(lib().cgx_probe_funm_combine(self._h, int(Q.shape[1]), int(Q.shape[0]), m.ctypes.data_as(C.POINTER(C.c_int)), _dp(Q),
                                                 int(Q.shape[2]), _dp(Cf), _dp(X), int(X.shape[1])))
        return X

    def eigenpairs(self, k, which="largest", steps=None, tol=0.0, v0=None, seed=1):
        """The k largest (which = "largest", descending) or smallest ("smallest", ascending) eigenvalues of the current symmetric,
        dense matrix and their eigenvectors by Lanczos with full reorthogonalisation (include/cgx.h cgx_eigenpairs): at most `steps`
        steps (default min(n, MAX_LANCZOS_STEPS, max(2 k + 20, 100))) from v0 (n doubles) or, with v0 = None, from the library's
        Rademacher vector of `seed`; tol = 0 runs all steps, tol > 0 stops once the Ritz estimates are below tol max |theta|.
        Returns (values, vectors, info): values (k,), vectors (k, n) one per row, info = dict(residual, estimate, steps_done,
        nfound); entries at j >= nfound are 0."""
        n, k = self.n(), int(k)
        if steps is None:
            steps = min(n, MAX_LANCZOS_STEPS, max(2 * k + 20, 100))
        steps = int(steps)
        if v0 is not None:
            v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1)
            assert v0.size == n, v0.shape
        kk = max(k, 1)
        values, residual, estimate = np.zeros(kk), np.zeros(kk), np.zeros(kk)
        vectors = np.zeros((kk, n), dtype=np.float64)
        done, found = C.c_int(), C.c_int()
        self._check(lib().cgx_eigenpairs(self._h, _EIG_NAMES.get(which, which), k, steps, float(tol), None if v0 is None else _dp(v0),
                                         int(seed), _dp(values), _dp(vectors), int(n), _dp(residual), _dp(estimate), C.byref(done),
                                         C.byref(found)))
        return values[:k], vectors[:k], {"residual": residual[:k], "estimate": estimate[:k], "steps_done": done.value,
                                         "nfound": found.value}

    def _probe_eigs_basis(self, v0, steps):
        """Test hook: the recurrence of eigenpairs alone.  Returns (Q, alpha, beta, steps_done): Q has steps + 1 rows, slots 0 ..
        m - 1 and, when the run was not frozen, the next vector q_m; the rows behind them are zero."""
        v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1)
        n, steps = self.n(), int(steps)
        assert v0.size == n, v0.shape
        Q = np.zeros((max(steps, 0) + 1, n), dtype=np.float64)
        alpha, beta = np.zeros(max(steps, 1)), np.zeros(max(steps, 1))
        done = C.c_int()
        self._check(lib().cgx_probe_eigs_basis(self._h, steps, _dp(v0), _dp(Q), int(n), _dp(alpha), _dp(beta), C.byref(done)))
        return Q, alpha[:steps], beta[:steps], done.value

    def _probe_eigs_orthogonalise(self, Q, w, nslots=None):
        """Test hook: one projection + subtraction pass of eigenpairs.  Q float64 (rows >= nslots, ldq >= n), w (>= n,): returns
        (h, w_new) with h[s] = Q[s, :n] . w[:n] for s < nslots and w_new = w[:n] - h @ Q[:nslots, :n]."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        n = self.n()
        nslots = Q.shape[0] if nslots is None else int(nslots)
        assert Q.ndim == 2 and Q.shape[1] >= n and Q.shape[0] >= nslots and w.size >= n
        h, out = np.zeros(max(nslots, 1)), np.zeros(n)
        self._check(lib().cgx_probe_eigs_orthogonalise(self._h, nslots, _dp(Q), int(Q.shape[1]), _dp(w), _dp(out), _dp(h)))
        return h[:nslots], out

    def precond_logdet(self):
        """log det M of the preconditioner that is set (0.0 with none); makes the preconditioner if no call has made it yet."""
        v = C.c_double()
        self._check(lib().cgx_precond_logdet(self._h, C.byref(v)))
        return v.value

    def slq_probes(self, fn, probes, seed=1):
        """The (probes, n) library probes logdet_pc (fn = SLQ_LOG: covariance M) / trace_inv_pc (fn = SLQ_INV: Rademacher) make
        themselves for this seed and the preconditioner that is set."""
        probes = int(probes)
        Z = np.zeros((max(probes, 1), self.n()), dtype=np.float64)
        self._check(lib().cgx_slq_probes(self._h, int(fn), probes, int(seed), _dp(Z), int(Z.shape[1])))
        return Z[:probes]

    def _trace_slq_pc(self, fn, probes, steps, seed, Z):
        if Z is not None:
            Z = np.ascontiguousarray(Z, dtype=np.float64)
            assert Z.ndim == 2 and Z.shape[1] == self.n(), Z.shape
            probes = Z.shape[0]
        est, err, ldm = C.c_double(), C.c_double(), C.c_double()
        per = np.zeros(max(int(probes), 1), dtype=np.float64)
        ritz = np.zeros(2, dtype=np.float64)
        self._check(lib().cgx_trace_slq_pc(self._h, int(fn), int(probes), int(steps), int(seed), None if Z is None else _dp(Z),
                                           0 if Z is None else int(Z.shape[1]), C.byref(est), C.byref(err), _dp(per), _dp(ritz),
                                           C.byref(ldm)))
        return {"estimate": est.value, "std_error": err.value, "per_probe": per[:int(probes)], "ritz_min": ritz[0], "ritz_max": ritz[1],
                "logdet_precond": ldm.value}

    def logdet_pc(self, probes=16, steps=30, seed=1, Z=None):
        """logdet through the preconditioner M that is set: log det M + the quadrature of log on M^-1/2 A M^-1/2, which needs far
        fewer steps and has a far smaller variance on a kernel matrix.  The probes must have covariance M: the library's (from
        `seed`), or the rows of Z, for whose covariance the caller answers.  Returns logdet's dict (ritz_*: of M^-1/2 A M^-1/2)
        plus logdet_precond = log det M; per_probe are the quadratures without log det M."""
        return self._trace_slq_pc(SLQ_LOG, probes, steps, seed, Z)

    def trace_inv_pc(self, probes=16, steps=30, seed=1, Z=None):
        """trace_inv through the preconditioner: the same probes (covariance I) and values z^T A^-1 z in fewer steps;
        logdet_precond is 0."""
        return self._trace_slq_pc(SLQ_INV, probes, steps, seed, Z)

    def probe_gemv_multi(self, P):
        """P: float64 array (k, n).  Returns (Y, pAp): Y[j] = A P[j] from the multi-vector K1, pAp[j] = P[j] . Y[j]."""
        P = np.ascontiguousarray(P, dtype=np.float64)
        assert P.ndim == 2 and P.shape[1] == self.n(), P.shape
        k = P.shape[0]
        Y = np.zeros_like(P)
        pap = np.zeros(max(k, 1), dtype=np.float64)
        self._check(lib().cgx_probe_gemv_multi(self._h, int(k), _dp(P), int(P.shape[1]), _dp(Y), int(Y.shape[1]), _dp(pap)))
        return Y, pap[:k]

    # -- stepping interface used by bench.py ----------------------------------------------------------
    def solve_begin(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self._check(lib().cgx_solve_begin(self._h, _dp(x0)))

    def solve_steps(self, nsteps):
        done = C.c_int()
        self._check(lib().cgx_solve_steps(self._h, int(nsteps), C.byref(done)))
        return bool(done.value)

    def solve_end(self, x=None):
        res = Result()
        xp = _dp(x) if x is not None else None
        self._check(lib().cgx_solve_end(self._h, xp, C.byref(res)))
        return res.as_dict()

    def gemv_samples(self):
        """K1 durations (ms) of the most recent solve_steps call, launch order (needs profile_gemv)."""
        cnt = C.c_int()
        self._check(lib().cgx_get_gemv_samples(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, dtype=np.float64)
        if cnt.value:
            self._check(lib().cgx_get_gemv_samples(self._h, _dp(out), cnt.value, C.byref(cnt)))
        return out

    def update_samples(self):
        """Durations (ms) of the event-timed update kernels (K3 / K3 with the exchange inside) of the most recent solve_steps
        call, launch order (needs profile_gemv and profile_update)."""
        cnt = C.c_int()
        self._check(lib().cgx_get_update_samples(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, dtype=np.float64)
        if cnt.value:
            self._check(lib().cgx_get_update_samples(self._h, _dp(out), cnt.value, C.byref(cnt)))
        return out

    # -- kernel probes -------------------------------------------------------------------------------
    def probe_gemv(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        y = np.zeros(self.n(), dtype=np.float64)
        pap = C.c_double()
        self._check(lib().cgx_probe_gemv(self._h, _dp(p), _dp(y), C.byref(pap)))
        return y, pap.value

    def probe_time_gemv(self, reps=20):
        ms = C.c_double()
        self._check(lib().cgx_probe_time_gemv(self._h, int(reps), C.byref(ms)))
        return ms.value

    def probe_vector_ops(self, alpha, beta, x, r, p, Ap):
        x, r, p = (np.array(v, dtype=np.float64, copy=True) for v in (x, r, p))
        Ap = np.ascontiguousarray(Ap, dtype=np.float64)
        rr = C.c_double()
        self._check(lib().cgx_probe_vector_ops(self._h, x.size, alpha, beta, _dp(x), _dp(r), _dp(p), _dp(Ap),
                                               C.byref(rr)))
        return x, r, p, rr.value

    def _set_fault_after(self, calls):
        """Error-path tests: the HIP call after `calls` more of this context fails (-1 = off)."""
        lib().cgx_probe_set_fault_after(self._h, int(calls))

    def _mailbox_to_host(self):
        """Test hook: the mailbox of a one-rank P2P context moves to pinned coherent host memory (exchange over PCIe)."""
        self._check(lib().cgx_probe_p2p_mailbox_to_host(self._h))

    def _host_mailboxes(self, prefix, stage):
        """Test hook: every rank's mailbox in POSIX shared host memory (stage 0: create own; barrier; stage 1: map the peers')."""
        self._check(lib().cgx_probe_p2p_host_mailboxes(self._h, prefix.encode(), int(stage)))

    def _set_p2p_epoch(self, chan, value):
        """Test hook: move the epoch counter of a mailbox channel forward (same call on every rank, between two solves)."""
        self._check(lib().cgx_probe_set_p2p_epoch(self._h, int(chan), int(value)))

    def _p2p_epoch(self, chan):
        v = C.c_ulonglong()
        self._check(lib().cgx_probe_get_p2p_epoch(self._h, int(chan), C.byref(v)))
        return v.value

    def _resident_test(self, epoch=0, mute_workgroup=-1):
        """Test hook of the LDS-resident solver: move its epoch counter forward / make one workgroup of the next launch skip a publish."""
        self._check(lib().cgx_probe_resident_test(self._h, int(epoch), int(mute_workgroup)))

    def _set_resident_limit(self, workgroups):
        """Test hook: bound of co-resident workgroups the fused P2P update may assume (0 = ask the runtime)."""
        lib().cgx_probe_set_resident_limit(self._h, int(workgroups))

    def probe_fill_matrix_hash(self, seed, symmetric=False, diag=0.0):
        """Test probe: the dense row blocks of the current problem overwritten on the device with the counter-based hash matrix
        (every element a different number in [-1, 1); the tests rebuild any row on the host from the same definition)."""
        self._check(lib().cgx_probe_fill_matrix_hash(self._h, int(seed), 1 if symmetric else 0, float(diag)))

    def probe_source_term(self, local_shard=0):
        """The device copy of b (n doubles) of a local shard."""
        b = np.zeros(self.n(), dtype=np.float64)
        self._check(lib().cgx_probe_get_source_term(self._h, int(local_shard), _dp(b)))
        return b

    def probe_matrix_rows(self, local_shard=0):
        row0 = C.c_int()
        rows = C.c_int()
        self._check(lib().cgx_probe_get_matrix_rows(self._h, local_shard, None, C.byref(row0), C.byref(rows)))
        A = np.zeros((rows.value, self.n()), dtype=np.float64)
        if rows.value:
            self._check(lib().cgx_probe_get_matrix_rows(self._h, local_shard, _dp(A), C.byref(row0), C.byref(rows)))
        return A, row0.value
