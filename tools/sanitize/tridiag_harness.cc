// The Jacobi-matrix functions of csrc/cgx_tridiag.cpp under the host sanitizers: linked with that file alone, no HIP library.
// Prints one line per case; exit code 1 if a call returns something else than the case expects.
#include "cgx.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <thread>
#include <vector>

static int failures = 0;

static void expect(const char *what, int m, cgx_status got, cgx_status want)
{
    printf("%s m=%d: status %d%s\n", what, m, got, got == want ? "" : "  UNEXPECTED");
    if (got != want) ++failures;
}

// the three public functions on one matrix; every eigenvector is asked for when m <= 50, else the two outermost
static void run_all(const char *what, const std::vector<double> &alpha, const std::vector<double> &beta, cgx_status want,
                    cgx_status want_log = CGX_OK)
{
    const int m = (int)alpha.size();
    std::vector<double> theta(m), weight(m), coef(m), all(m);
    double minmax[2] = {0.0, 0.0};
    expect(what, m, cgx_tridiag_quadrature(m, alpha.data(), beta.data(), theta.data(), weight.data()), want);
    for (int fn = CGX_FN_SQRT; fn <= CGX_FN_EXP; ++fn)
        expect(what, m, cgx_tridiag_function(m, alpha.data(), beta.data(), fn, 0.5, coef.data(), minmax),
               want == CGX_OK && fn != CGX_FN_EXP ? want_log : want);
    std::vector<int> index;
    if (m <= 50) for (int i = 0; i < m; ++i) index.push_back(i);
    else index = {0, m - 1};
    std::vector<double> S(index.size() * (size_t)m);
    expect(what, m, cgx_tridiag_eigenvectors(m, alpha.data(), beta.data(), (int)index.size(), index.data(), all.data(), S.data()), want);
    expect(what, m, cgx_tridiag_eigenvectors(m, alpha.data(), beta.data(), 1, index.data(), nullptr, S.data()), want);
}

// a positive definite Jacobi matrix: 2.5 + small variation on the diagonal, off-diagonals below 1
static void jacobi(int m, std::vector<double> *alpha, std::vector<double> *beta)
{
    alpha->assign(m, 0.0);
    beta->assign(m, 0.0);   // (m entries: the last one is never part of T)
    for (int i = 0; i < m; ++i) {
        (*alpha)[i] = 2.5 + 0.25 * std::sin(0.37 * i);
        (*beta)[i] = 0.6 + 0.3 * std::cos(0.11 * i);
    }
}

int main()
{
    std::vector<double> a, b;
    for (int m : {1, 2, 3, 50, 1024}) {
        jacobi(m, &a, &b);
        run_all("positive definite", a, b, CGX_OK);
    }
    jacobi(50, &a, &b);
    b[20] = 0.0;
    run_all("interior zero beta", a, b, CGX_OK);
    a.assign(24, 3.0);
    b.assign(24, 0.0);
    run_all("repeated eigenvalues (3 I)", a, b, CGX_OK);
    for (int i = 0; i < 24; i += 2) b[i] = 1.0;   // twelve copies of [[3, 1], [1, 3]]: eigenvalues 2 and 4, twelve times each
    run_all("repeated eigenvalues (blocks)", a, b, CGX_OK);

    // refusals
    jacobi(8, &a, &b);
    a[3] = std::numeric_limits<double>::quiet_NaN();
    run_all("NaN alpha", a, b, CGX_ERR_BAD_ARG);
    jacobi(8, &a, &b);
    b[6] = std::numeric_limits<double>::infinity();
    run_all("infinite beta", a, b, CGX_ERR_BAD_ARG);
    jacobi(8, &a, &b);
    b[7] = std::numeric_limits<double>::quiet_NaN();   // beyond T: not read
    run_all("NaN behind the last beta", a, b, CGX_OK);
    jacobi(8, &a, &b);
    a[2] = -40.0;                                      // a negative eigenvalue: outside the domain of all but exp
    run_all("indefinite", a, b, CGX_OK, CGX_ERR_BAD_ARG);
    {
        jacobi(8, &a, &b);
        std::vector<double> out(8), S(8);
        double minmax[2];
        const int inside = 0, below = -1, above = 8;
        expect("m = 0", 0, cgx_tridiag_quadrature(0, a.data(), b.data(), out.data(), S.data()), CGX_ERR_BAD_ARG);
        expect("null alpha", 8, cgx_tridiag_quadrature(8, nullptr, b.data(), out.data(), S.data()), CGX_ERR_BAD_ARG);
        expect("null beta", 8, cgx_tridiag_function(8, a.data(), nullptr, CGX_FN_SQRT, 0.0, out.data(), minmax), CGX_ERR_BAD_ARG);
        expect("null beta, m = 1", 1, cgx_tridiag_function(1, a.data(), nullptr, CGX_FN_SQRT, 0.0, out.data(), nullptr), CGX_OK);
        expect("unknown fn", 8, cgx_tridiag_function(8, a.data(), b.data(), CGX_FN_EXP + 1, 0.0, out.data(), minmax), CGX_ERR_BAD_ARG);
        expect("fn below the range", 8, cgx_tridiag_function(8, a.data(), b.data(), -1, 0.0, out.data(), minmax), CGX_ERR_BAD_ARG);
        expect("negative exp param", 8, cgx_tridiag_function(8, a.data(), b.data(), CGX_FN_EXP, -1.0, out.data(), minmax), CGX_ERR_BAD_ARG);
        expect("NaN exp param", 8, cgx_tridiag_function(8, a.data(), b.data(), CGX_FN_EXP, std::nan(""), out.data(), minmax), CGX_ERR_BAD_ARG);
        expect("nsel = 0", 8, cgx_tridiag_eigenvectors(8, a.data(), b.data(), 0, &inside, out.data(), S.data()), CGX_ERR_BAD_ARG);
        expect("index below", 8, cgx_tridiag_eigenvectors(8, a.data(), b.data(), 1, &below, out.data(), S.data()), CGX_ERR_BAD_ARG);
        expect("index above", 8, cgx_tridiag_eigenvectors(8, a.data(), b.data(), 1, &above, out.data(), S.data()), CGX_ERR_BAD_ARG);
        a[0] = 0.0;                                    // T = diag(0, ...) + couplings has a Ritz value <= 0: log is out of its domain
        a[1] = 0.0;
        expect("log out of domain", 8, cgx_tridiag_function(8, a.data(), b.data(), CGX_FN_LOG, 0.0, out.data(), minmax), CGX_ERR_BAD_ARG);
        printf("  smallest eigenvalue reported %.3g\n", minmax[0]);
        if (!(minmax[0] <= 0.0)) ++failures;
    }

    // as cgx_apply_function: 15 threads at once, every one on outputs of its own, m = 256
    const int m = 256, nthreads = 15;
    jacobi(m, &a, &b);
    std::vector<std::vector<double>> coef(nthreads, std::vector<double>(m));
    std::vector<cgx_status> st(nthreads, CGX_ERR_BAD_ARG);
    std::vector<std::thread> pool;
    for (int j = 0; j < nthreads; ++j)
        pool.emplace_back([&, j] { st[j] = cgx_tridiag_function(m - j, a.data(), b.data(), CGX_FN_SQRT + j % 5, 0.5, coef[j].data(), nullptr); });
    for (std::thread &t : pool) t.join();
    for (int j = 0; j < nthreads; ++j) expect("threaded", m - j, st[j], CGX_OK);
    std::vector<double> again(m);
    expect("threaded, repeated serially", m, cgx_tridiag_function(m, a.data(), b.data(), CGX_FN_SQRT, 0.5, again.data(), nullptr), CGX_OK);
    if (again != coef[0]) { printf("threaded and serial results differ  UNEXPECTED\n"); ++failures; }
    printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
