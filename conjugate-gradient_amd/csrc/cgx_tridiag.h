// cgx_tridiag.h -- what the host code of the Lanczos family shares about a Jacobi matrix T (diagonal alpha, off-diagonal beta):
// cgx_tridiag.cpp, host arithmetic only.  No HIP header and no cgx_ctx, so the file builds and runs under the host sanitizers by
// itself (tools/sanitize/tridiag_harness.cc).
#pragma once

#include "../../include/cgx.h"

namespace cgxi {

// alpha[0 .. m) and beta[0 .. m - 1) are finite (beta[m - 1] is not part of T and is not read)
bool finite_entries(int m, const double *alpha, const double *beta);

// The m-point Gauss rule of T: the eigenvalues ascending (ties by their place in the sweep's d) and the squared first components of
// their eigenvectors.  false: no convergence in 60 sweeps per value.
bool gauss_rule(int m, const double *alpha, const double *beta, double *theta, double *weight);

bool funm_args_ok(int fn, double param);   // a known CGX_FN_*, and for CGX_FN_EXP a finite param >= 0
enum class TridiagFn { ok, no_convergence, domain };
// coef = f(T) e_1, entries and arguments already checked.  minmax (may be null): the smallest and largest eigenvalue, filled before
// the domain is looked at.  *bad (may be null): the smallest eigenvalue when it lies outside the domain of f.
TridiagFn tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, double *minmax, double *bad);
// All eigenvalues ascending into theta (may be null) and the unit eigenvectors of index[0 .. nsel), counted in that order, as rows of
// S (m doubles each, first component >= 0); entries already checked.  false: no convergence.
bool tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index, double *theta, double *S);

}  // namespace cgxi
