// cgx_funm.hip -- the combine kernel of cgx_apply_function: X_j = sum_t c_j[t] v_(j,t), the kept Lanczos
// vectors of column j weighted with the coefficients ||b_j|| f(T_j) e_1 that the host made.
//
// The basis is laid out as the recurrence left it: slot t holds the nvec columns at pitch lda, so element i of v_(j,t) is at
// (t * nvec + j) * lda + i -- an offset that leaves 32 bits well inside the supported sizes (16 vectors and 1024 steps: 2^32 bytes
// at n = 32768, 2^31 doubles at n = 131072), hence size_t throughout.  A thread owns one element and walks t over [0, m_j) only:
// the slots behind a column's last step hold whatever an earlier call left there and are never read.  The sum is ONE fma chain in
// ascending t from +0.0, so a column's bits depend on its own basis and coefficients alone; the loads of kUnroll steps are issued
// ahead of their fmas.  The basis is read once (non-temporal 8-byte loads: correct at any row pitch), the coefficient is the same
// for the whole workgroup (scalar loads), the store is plain.  No floating-point atomics.
#include "cgx_kernels.h"
#include "cgx_device.h"

namespace cgx {

namespace {

constexpr int kUnroll = 8;

// Workgroup (b, j) = rows [256 b, 256 b + 256) of column j.
__global__ __launch_bounds__(256) void k_funm_combine(int n, int nvec, int steps, long lda, const double *__restrict__ Q,
                                                      const double *__restrict__ C, const int *__restrict__ m, double *__restrict__ X,
                                                      long ldx)
{
    const int j = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int mj = min(max(m[j], 0), steps);
    const size_t stride = (size_t)nvec * (size_t)lda;
    const double *q = Q + (size_t)j * (size_t)lda + (size_t)i;
    const double *c = C + (size_t)j * (size_t)steps;
    double acc = 0.0;
    int t = 0;
    for (; t + kUnroll <= mj; t += kUnroll) {
        double v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = __builtin_nontemporal_load(q + (size_t)(t + u) * stride);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) acc = fma(c[t + u], v[u], acc);
    }
    for (; t < mj; ++t) acc = fma(c[t], __builtin_nontemporal_load(q + (size_t)t * stride), acc);
    X[(size_t)j * (size_t)ldx + (size_t)i] = acc;
}

}  // namespace

hipError_t launch_funm_combine(const FunmArgs &a, hipStream_t s)
{
    if (a.nvec < 1 || a.nvec > kMaxRhs || a.n < 1 || a.steps < 1 || a.steps > kMaxLanczosSteps || a.lda < a.n || a.ldx < a.n)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_funm_combine, dim3((a.n + 255) / 256, a.nvec), dim3(256), 0, s, a.n, a.nvec, a.steps, a.lda, a.Q, a.C, a.m, a.X,
                       a.ldx);
    return hipGetLastError();
}

}  // namespace cgx
