// cgx_tridiag.cpp -- cgx_tridiag_quadrature, cgx_tridiag_function, cgx_tridiag_eigenvectors and what the Lanczos hosts share with
// them (cgx_tridiag.h): everything about a Jacobi matrix that needs no device (DESIGN.md sections 17, 19, 20).
//
// One eigen-decomposition serves all of it: implicit symmetric QL with Wilkinson's shift, the rotations applied to the first row of
// the eigenvector matrix alone -- O(m^2) time, O(m) memory, no LAPACK -- and, where a whole vector is wanted (f(T) e_1, an
// eigenvector), recorded and replayed in reverse.  cgx.h and the standard library only; every call works on its own storage, so
// calls on separate outputs may run side by side (cgx_apply_function gives every column a thread).
#include "cgx_tridiag.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

using namespace cgxi;

namespace {

// sqrt(a^2 + b^2) without overflow (the QL sweep's plane rotations)
double pythag(double a, double b) { return std::hypot(a, b); }

// Implicit symmetric QL with Wilkinson's shift on (d, e), carrying the FIRST ROW z of the eigenvector matrix along: the rotations
// of a sweep are applied to z alone, so the work is O(m^2) and nothing m x m is held.  e[i] couples i and i + 1; e[m-1] is work space.
// rec != nullptr: every plane rotation applied to z is appended, in the order applied (about 1.1 m^2 of them); the arithmetic of
// the sweep is the same with and without.
struct Rotation {
    int i;
    double c, s;
};

bool ql_first_row(int m, double *d, double *e, double *z, std::vector<Rotation> *rec)
{
    for (int l = 0; l < m; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; ++mm) {
                const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
                if (std::fabs(e[mm]) + dd == dd) break;
            }
            if (mm != l) {
                if (iter++ == 60) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = pythag(g, 1.0);
                g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = pythag(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[mm] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                    f = z[i + 1];
                    z[i + 1] = s * z[i] + c * f;
                    z[i] = c * z[i] - s * f;
                    if (rec) rec->push_back(Rotation{i, c, s});
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[mm] = 0.0;
            }
        } while (mm != l);
    }
    return true;
}

// T = S diag(d) S^T with S the product of the sweep's rotations in the order applied, and z = S^T e_1.
struct Jacobi {
    std::vector<double> work;       // d, e, z: m doubles each
    std::vector<Rotation> rot;      // record: the rotations
    std::vector<int> order;         // sort: the places of d in ascending order of value, ties by place
    const double *d = nullptr, *z = nullptr;
    // S x over x (m doubles): the recorded rotations from the last one back
    void apply_S(double *x) const
    {
        for (size_t r = rot.size(); r-- > 0;) {
            const Rotation &q = rot[r];
            const double a = x[q.i], b = x[q.i + 1];
            x[q.i] = q.c * a + q.s * b;
            x[q.i + 1] = q.c * b - q.s * a;
        }
    }
};

// THE set-up of every function here: (alpha, beta) into d and e, z = e_1, the sweep.  false: no convergence in 60 sweeps per value.
bool decompose(int m, const double *alpha, const double *beta, bool record, bool sort, Jacobi *J)
{
    J->work.assign((size_t)3 * m, 0.0);
    if (record) J->rot.reserve((size_t)m * m + (size_t)m * m / 4 + 64);
    double *d = J->work.data(), *e = d + m, *z = e + m;
    for (int i = 0; i < m; ++i) {
        d[i] = alpha[i];
        if (i + 1 < m) e[i] = beta[i];
    }
    z[0] = 1.0;
    J->d = d;
    J->z = z;
    if (!ql_first_row(m, d, e, z, record ? &J->rot : nullptr)) return false;
    if (sort) {
        J->order.resize((size_t)m);
        std::iota(J->order.begin(), J->order.end(), 0);
        std::sort(J->order.begin(), J->order.end(), [d](int a, int b) { return d[a] < d[b] || (d[a] == d[b] && a < b); });
    }
    return true;
}

bool funm_in_domain(int fn, double theta)
{
    return fn == CGX_FN_EXP || (fn == CGX_FN_SQRT ? theta >= 0.0 : theta > 0.0);
}

double funm_value(int fn, double param, double theta)
{
    switch (fn) {
    case CGX_FN_SQRT: return std::sqrt(theta);
    case CGX_FN_INVSQRT: return 1.0 / std::sqrt(theta);
    case CGX_FN_INV: return 1.0 / theta;
    case CGX_FN_LOG: return std::log(theta);
    default: return std::exp(-param * theta);
    }
}

}  // namespace

bool cgxi::finite_entries(int m, const double *alpha, const double *beta)
{
    for (int i = 0; i < m; ++i)
        if (!std::isfinite(alpha[i]) || (i + 1 < m && !std::isfinite(beta[i]))) return false;
    return true;
}

bool cgxi::gauss_rule(int m, const double *alpha, const double *beta, double *theta, double *weight)
{
    Jacobi J;
    if (!decompose(m, alpha, beta, false, true, &J)) return false;
    for (int i = 0; i < m; ++i) {
        theta[i] = J.d[J.order[i]];
        weight[i] = J.z[J.order[i]] * J.z[J.order[i]];
    }
    return true;
}

bool cgxi::funm_args_ok(int fn, double param)
{
    if (fn < CGX_FN_SQRT || fn > CGX_FN_EXP) return false;
    return fn != CGX_FN_EXP || (std::isfinite(param) && param >= 0.0);
}

// f(T) e_1 = S g with g_k = f(d_k) z_k.
cgxi::TridiagFn cgxi::tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, double *minmax,
                                       double *bad)
{
    Jacobi J;
    if (!decompose(m, alpha, beta, true, false, &J)) return TridiagFn::no_convergence;
    double lo = J.d[0], hi = J.d[0];
    for (int i = 1; i < m; ++i) {
        lo = std::min(lo, J.d[i]);
        hi = std::max(hi, J.d[i]);
    }
    if (minmax) { minmax[0] = lo; minmax[1] = hi; }
    if (!funm_in_domain(fn, lo)) {
        if (bad) *bad = lo;
        return TridiagFn::domain;
    }
    for (int i = 0; i < m; ++i) coef[i] = funm_value(fn, param, J.d[i]) * J.z[i];
    J.apply_S(coef);
    return TridiagFn::ok;
}

// The eigenvector of d_k is S e_k: O(m^2) each, nothing m x m held.
bool cgxi::tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index, double *theta, double *S)
{
    Jacobi J;
    if (!decompose(m, alpha, beta, true, true, &J)) return false;
    if (theta)
        for (int i = 0; i < m; ++i) theta[i] = J.d[J.order[i]];
    for (int c = 0; c < nsel; ++c) {
        double *v = S + (size_t)c * m;
        std::fill(v, v + m, 0.0);
        v[J.order[index[c]]] = 1.0;
        J.apply_S(v);
        if (v[0] < 0.0)
            for (int i = 0; i < m; ++i) v[i] = -v[i];
    }
    return true;
}

extern "C" {

cgx_status cgx_tridiag_eigenvectors(int m, const double *alpha, const double *beta, int nsel, const int *index, double *theta, double *S)
{
    if (m < 1 || !alpha || !S || (m > 1 && !beta) || nsel < 1 || !index || !finite_entries(m, alpha, beta)) return CGX_ERR_BAD_ARG;
    for (int c = 0; c < nsel; ++c)
        if (index[c] < 0 || index[c] >= m) return CGX_ERR_BAD_ARG;
    return tridiag_eigenvectors(m, alpha, beta, nsel, index, theta, S) ? CGX_OK : CGX_ERR_UNSUPPORTED;   // (no convergence in 60 sweeps)
}

cgx_status cgx_tridiag_function(int m, const double *alpha, const double *beta, int fn, double param, double *coef, double *theta_minmax)
{
    if (m < 1 || !alpha || !coef || (m > 1 && !beta) || !funm_args_ok(fn, param) || !finite_entries(m, alpha, beta)) return CGX_ERR_BAD_ARG;
    switch (tridiag_function(m, alpha, beta, fn, param, coef, theta_minmax, nullptr)) {
    case TridiagFn::ok: return CGX_OK;
    case TridiagFn::domain: return CGX_ERR_BAD_ARG;        // an eigenvalue where f is not defined (theta_minmax is filled)
    default: return CGX_ERR_UNSUPPORTED;                   // (no convergence in 60 sweeps per value)
    }
}

cgx_status cgx_tridiag_quadrature(int m, const double *alpha, const double *beta, double *theta, double *weight)
{
    if (m < 1 || !alpha || !theta || !weight || (m > 1 && !beta) || !finite_entries(m, alpha, beta)) return CGX_ERR_BAD_ARG;
    return gauss_rule(m, alpha, beta, theta, weight) ? CGX_OK : CGX_ERR_UNSUPPORTED;   // (no convergence in 60 sweeps per value)
}

}  // extern "C"
