// Dev tool: what does the memory system deliver for the ACCESS PATTERN of the symmetric K1 (csrc/cgx_symv.hip) alone?
// The upper-triangle B x B tiles of an n x n block at pitch lda (n = 32768: 8 GiB), walked as k_symv_tiles walks them: a grid
// of 4 workgroups per CU, each a run of consecutive tiles in strip order; per tile every wave reads B/4 rows in batches, lane =
// 16 B of each 1-KiB column piece, 16 loads in flight per lane, non-temporal.  Bytes counted = the tiles' bytes.
// hipcc --offload-arch=gfx950 -O3 tools/hbm_tri_bw.hip -o /tmp/hbm_tri_bw && /tmp/hbm_tri_bw [n]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double d2 __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
    } while (0)

__device__ long strip_start(long I, long nb) { return I * nb - I * (I - 1) / 2; }

template <int B>
__global__ __launch_bounds__(256, 4) void k_tri(const double *__restrict__ A, long lda, int n, int nb, long tiles, double *out)
{
    constexpr int H = B / 128, R = 16 / H, RW = B / 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long G = gridDim.x, t0 = tiles * (long)blockIdx.x / G, t1 = tiles * ((long)blockIdx.x + 1) / G;
    if (t0 >= t1) return;
    long I = 0;
    while (I + 1 < nb && strip_start(I + 1, nb) <= t0) ++I;
    long J = I + (t0 - strip_start(I, nb));
    double s0 = 0.0, s1 = 0.0;
    for (long t = t0; t < t1; ++t) {
        for (int b = 0; b < RW / R; ++b) {
            d2 a[R][H];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                long row = I * B + w * RW + b * R + q;
                if (row > n - 1) row = n - 1;
                const char *ar = reinterpret_cast<const char *>(A + row * lda);
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    int c = (int)(J * B) + h * 128 + 2 * lane;
                    if (c > n - 2) c = n - 2;
                    a[q][h] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(ar + (unsigned)c * 8u));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int h = 0; h < H; ++h) { s0 += a[q][h].x; s1 += a[q][h].y; }
        }
        if (++J == nb) { ++I; J = I; }
    }
    if (s0 + s1 == 12345.678) out[blockIdx.x * 256 + threadIdx.x] = s0;   // keeps the loads alive
}

template <int B>
void run(const double *A, long lda, int n, int cus, double *out)
{
    const int nb = (n + B - 1) / B;
    const long tiles = (long)nb * (nb + 1) / 2;
    const int grid = (int)std::min<long>(tiles, 4L * cus);
    double bytes = 0;   // the tiles' bytes inside the n x n block
    for (int I = 0; I < nb; ++I)
        for (int J = I; J < nb; ++J)
            bytes += 8.0 * std::min(B, n - I * B) * std::min(B, n - J * B);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 12; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_tri<B>, dim3(grid), dim3(256), 0, 0, A, lda, n, nb, tiles, out);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float t = 0;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2], best = ms[0];
    printf("{\"B\": %d, \"tiles\": %ld, \"grid\": %d, \"bytes\": %.0f, \"median_ms\": %.4f, \"best_ms\": %.4f, \"median_GBps\": %.1f, \"best_GBps\": %.1f}\n",
           B, tiles, grid, bytes, med, best, bytes / med / 1e6, bytes / best / 1e6);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 32768;
    const long lda = ((long)n + 15) / 16 * 16 + 16;   // the library's default pitch (CGX_LDA_PAD 16)
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    double *A = nullptr, *out = nullptr;
    CHECK(hipMalloc(&A, (size_t)n * lda * sizeof(double)));
    CHECK(hipMalloc(&out, 4L * prop.multiProcessorCount * 256 * sizeof(double)));
    CHECK(hipMemset(A, 0, (size_t)n * lda * sizeof(double)));
    run<128>(A, lda, n, prop.multiProcessorCount, out);
    run<256>(A, lda, n, prop.multiProcessorCount, out);
    run<512>(A, lda, n, prop.multiProcessorCount, out);
    CHECK(hipFree(A));
    CHECK(hipFree(out));
    return 0;
}
