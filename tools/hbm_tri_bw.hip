// Dev tool: what does the memory system deliver for the ACCESS PATTERN of the symmetric K1 (csrc/cgx_symv.hip) alone?
// The upper-triangle B x B tiles of an n x n block at pitch lda (n = 32768: 8 GiB), walked as k_symv_tiles walks them: every
// workgroup a run of consecutive tiles in strip order; per tile every wave reads B/4 rows in batches, lane = 16 B of each
// 1-KiB column piece, 16 loads in flight per lane, non-temporal.  Bytes counted = the tiles' bytes.
//   hbm_tri_bw [n]            B = 128 / 256 / 512 at a grid of 4 workgroups per CU (the figures of profiles/r06_symv/tri_bw.txt)
//   hbm_tri_bw [n] forms      the B = 256 walk in six forms on one block, 10 repetitions each, the forms interleaved:
//                               a        strided A, grid = 4 x CUs (static runs of 8 or 9 tiles at n = 32768)
//                               b4 b2 b1 strided A, grid = tiles / 4, tiles / 2, tiles (static runs of 4, 2 and 1 tiles)
//                               c        as a, reading a tile-packed copy (tile t = 256 x 256 contiguous doubles at t * 65536)
//                               d        as b1, reading the tile-packed copy
//   hbm_tri_bw [n] blocks [K] K strided blocks and K packed copies alive at once (K = 4: 48 GiB at n = 32768), forms a, b1 and d
//                             on each, the blocks interleaved: a time that belongs to where an allocation landed shows as
//                             one block slow and another fast in the same process
//                             (profiles/symv_walk/)
// hipcc --offload-arch=gfx950 -O3 tools/hbm_tri_bw.hip -o /tmp/hbm_tri_bw && /tmp/hbm_tri_bw [n] [forms]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef double d2 __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
    } while (0)

// as csrc/cgx_symv.hip: tile t of the strip order to (I, J)
__device__ __forceinline__ long strip_start(long I, long nb) { return I * nb - I * (I - 1) / 2; }
__device__ __forceinline__ void tri_tile(long t, long nb, long *I, long *J)
{
    const double b = 2.0 * (double)nb + 1.0;
    long i = (long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    i = i < 0 ? 0 : (i > nb - 1 ? nb - 1 : i);
    while (i + 1 < nb && strip_start(i + 1, nb) <= t) ++i;
    while (i > 0 && strip_start(i, nb) > t) --i;
    *I = i;
    *J = i + (t - strip_start(i, nb));
}

// PACKED: A is the tile-packed copy (tile t at A + t * B * B, row pitch B, zero filled outside n: no clamps)
template <int B, bool PACKED>
__global__ __launch_bounds__(256, 4) void k_tri(const double *__restrict__ A, long lda, int n, int nb, long tiles, double *out)
{
    constexpr int H = B / 128, R = 16 / H, RW = B / 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long G = gridDim.x, t0 = tiles * (long)blockIdx.x / G, t1 = tiles * ((long)blockIdx.x + 1) / G;
    if (t0 >= t1) return;
    long I, J;
    tri_tile(t0, nb, &I, &J);
    double s0 = 0.0, s1 = 0.0;
    for (long t = t0; t < t1; ++t) {
        for (int b = 0; b < RW / R; ++b) {
            d2 a[R][H];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const char *ar;
                if constexpr (PACKED) {
                    ar = reinterpret_cast<const char *>(A + t * (long)(B * B) + (long)(w * RW + b * R + q) * B);
                } else {
                    long row = I * B + w * RW + b * R + q;
                    if (row > n - 1) row = n - 1;
                    ar = reinterpret_cast<const char *>(A + row * lda);
                }
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    int c = h * 128 + 2 * lane;
                    if constexpr (!PACKED) {
                        c += (int)(J * B);
                        if (c > n - 2) c = n - 2;
                    }
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
    if (s0 + s1 == 12345.678) out[(blockIdx.x & 1023) * 256 + threadIdx.x] = s0;   // keeps the loads alive
}

template <int B>
double tile_bytes(int n)   // the tiles' bytes inside the n x n block
{
    const int nb = (n + B - 1) / B;
    double bytes = 0;
    for (int I = 0; I < nb; ++I)
        for (int J = I; J < nb; ++J)
            bytes += 8.0 * std::min(B, n - I * B) * std::min(B, n - J * B);
    return bytes;
}

template <int B, bool PACKED>
float timed(const double *A, long lda, int n, int grid, double *out, hipEvent_t e0, hipEvent_t e1)
{
    const int nb = (n + B - 1) / B;
    const long tiles = (long)nb * (nb + 1) / 2;
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_tri<B, PACKED>), dim3(grid), dim3(256), 0, 0, A, lda, n, nb, tiles, out);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float t = 0;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    return t;
}

template <int B>
void run(const double *A, long lda, int n, int cus, double *out, hipEvent_t e0, hipEvent_t e1)
{
    const int nb = (n + B - 1) / B;
    const long tiles = (long)nb * (nb + 1) / 2;
    const int grid = (int)std::min<long>(tiles, 4L * cus);
    const double bytes = tile_bytes<B>(n);
    std::vector<float> ms;
    for (int rep = 0; rep < 12; ++rep) {
        const float t = timed<B, false>(A, lda, n, grid, out, e0, e1);
        if (rep >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2], best = ms[0];
    printf("{\"B\": %d, \"tiles\": %ld, \"grid\": %d, \"bytes\": %.0f, \"median_ms\": %.4f, \"best_ms\": %.4f, \"median_GBps\": %.1f, \"best_GBps\": %.1f}\n",
           B, tiles, grid, bytes, med, best, bytes / med / 1e6, bytes / best / 1e6);
}

// The six forms of the B = 256 walk, interleaved: repetition r of every form before repetition r + 1 of any
void run_forms(const double *A, long lda, int n, int cus, double *out, hipEvent_t e0, hipEvent_t e1)
{
    constexpr int B = 256;
    const int nb = (n + B - 1) / B;
    const long tiles = (long)nb * (nb + 1) / 2;
    double *P = nullptr;   // zeros, as A: the loads do not depend on the values
    CHECK(hipMalloc(&P, (size_t)tiles * B * B * sizeof(double)));
    CHECK(hipMemset(P, 0, (size_t)tiles * B * B * sizeof(double)));
    const int g4 = (int)std::min<long>(tiles, 4L * cus);
    struct Form { const char *name; bool packed; int grid; std::vector<float> ms; };
    std::vector<Form> forms = {{"a", false, g4, {}},
                               {"b4", false, (int)std::max<long>(1, tiles / 4), {}},
                               {"b2", false, (int)std::max<long>(1, tiles / 2), {}},
                               {"b1", false, (int)tiles, {}},
                               {"c", true, g4, {}},
                               {"d", true, (int)tiles, {}}};
    for (int rep = 0; rep < 12; ++rep)
        for (Form &f : forms) {
            const float t = f.packed ? timed<B, true>(P, B, n, f.grid, out, e0, e1) : timed<B, false>(A, lda, n, f.grid, out, e0, e1);
            if (rep >= 2) f.ms.push_back(t);
        }
    const double strided = tile_bytes<B>(n), packed = (double)tiles * B * B * 8.0;
    for (Form &f : forms) {
        std::vector<float> s = f.ms;
        std::sort(s.begin(), s.end());
        const double med = 0.5 * (s[s.size() / 2 - 1] + s[s.size() / 2]), bytes = f.packed ? packed : strided;
        printf("{\"form\": \"%s\", \"packed\": %d, \"tiles\": %ld, \"grid\": %d, \"bytes\": %.0f, \"median_ms\": %.4f, \"best_ms\": %.4f, "
               "\"worst_ms\": %.4f, \"median_GBps\": %.1f, \"reps_ms\": [",
               f.name, f.packed ? 1 : 0, tiles, f.grid, bytes, med, (double)s.front(), (double)s.back(), bytes / med / 1e6);
        for (size_t i = 0; i < f.ms.size(); ++i) printf("%s%.4f", i ? ", " : "", (double)f.ms[i]);
        printf("]}\n");
    }
    CHECK(hipFree(P));
}

// K strided blocks and K packed copies alive at once in one process, forms a / b1 on each strided block and d on each packed
// one, 10 repetitions, the blocks interleaved: does the time belong to the block (where the allocation landed)?
void run_blocks(int K, long lda, int n, int cus, double *out, hipEvent_t e0, hipEvent_t e1)
{
    constexpr int B = 256;
    const int nb = (n + B - 1) / B;
    const long tiles = (long)nb * (nb + 1) / 2;
    const int g4 = (int)std::min<long>(tiles, 4L * cus);
    std::vector<double *> A(K, nullptr), P(K, nullptr);
    for (int k = 0; k < K; ++k) {
        CHECK(hipMalloc(&A[k], (size_t)n * lda * sizeof(double)));
        CHECK(hipMemset(A[k], 0, (size_t)n * lda * sizeof(double)));
        CHECK(hipMalloc(&P[k], (size_t)tiles * B * B * sizeof(double)));
        CHECK(hipMemset(P[k], 0, (size_t)tiles * B * B * sizeof(double)));
    }
    std::vector<std::vector<float>> ta(K), tb(K), td(K);
    for (int rep = 0; rep < 12; ++rep)
        for (int k = 0; k < K; ++k) {
            const float a = timed<B, false>(A[k], lda, n, g4, out, e0, e1);
            const float b = timed<B, false>(A[k], lda, n, (int)tiles, out, e0, e1);
            const float d = timed<B, true>(P[k], B, n, (int)tiles, out, e0, e1);
            if (rep >= 2) { ta[k].push_back(a); tb[k].push_back(b); td[k].push_back(d); }
        }
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]); };
    for (int k = 0; k < K; ++k)
        printf("{\"block\": %d, \"A\": \"%p\", \"packed\": \"%p\", \"a_median_ms\": %.4f, \"b1_median_ms\": %.4f, \"d_median_ms\": %.4f}\n", k,
               (void *)A[k], (void *)P[k], med(ta[k]), med(tb[k]), med(td[k]));
    for (int k = 0; k < K; ++k) { CHECK(hipFree(A[k])); CHECK(hipFree(P[k])); }
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 32768;
    const bool forms = argc > 2 && !strcmp(argv[2], "forms");
    if (n < 2) { fprintf(stderr, "n must be at least 2\n"); return 1; }
    if (argc > 2 && !strcmp(argv[2], "blocks")) {
        const int K = argc > 3 ? std::min(std::max(atoi(argv[3]), 1), 8) : 4;
        const long pitch = ((long)n + 15) / 16 * 16 + 16;
        hipDeviceProp_t pr;
        CHECK(hipGetDeviceProperties(&pr, 0));
        double *o = nullptr;
        hipEvent_t a, b;
        CHECK(hipMalloc(&o, 1024L * 256 * sizeof(double)));
        CHECK(hipEventCreate(&a));
        CHECK(hipEventCreate(&b));
        run_blocks(K, pitch, n, pr.multiProcessorCount, o, a, b);
        CHECK(hipEventDestroy(a));
        CHECK(hipEventDestroy(b));
        CHECK(hipFree(o));
        return 0;
    }
    const long lda = ((long)n + 15) / 16 * 16 + 16;   // the library's default pitch (CGX_LDA_PAD 16)
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    double *A = nullptr, *out = nullptr;
    CHECK(hipMalloc(&A, (size_t)n * lda * sizeof(double)));
    CHECK(hipMalloc(&out, 1024L * 256 * sizeof(double)));
    CHECK(hipMemset(A, 0, (size_t)n * lda * sizeof(double)));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    if (forms) {
        run_forms(A, lda, n, prop.multiProcessorCount, out, e0, e1);
    } else {
        run<128>(A, lda, n, prop.multiProcessorCount, out, e0, e1);
        run<256>(A, lda, n, prop.multiProcessorCount, out, e0, e1);
        run<512>(A, lda, n, prop.multiProcessorCount, out, e0, e1);
    }
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    CHECK(hipFree(A));
    CHECK(hipFree(out));
    return 0;
}
