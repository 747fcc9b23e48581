// Dev tool: which buffer of the symmetric K1 carries its two time levels?  The library's own plain
// product (launch_symv_plain: k_symv_tiles<256,false> + k_symv_fold<false>, csrc/cgx_symv.hip compiled in) on one 8 GiB A, with
// K slot buffers and K sets of vectors (v, Ap, partials) allocated in turn with spacers of odd sizes between them, so that they
// land at different offsets.  Timed: every slot buffer with vector set 0, every vector set with slot buffer 0, a second A.
// 20 launches per figure, median, the candidates interleaved.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iconjugate-gradient_amd/csrc -Iinclude tools/symv_buffers.hip -o /tmp/symv_buffers
#include "../conjugate-gradient_amd/csrc/cgx_symv.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } \
    } while (0)

struct Vecs { double *v, *Ap, *partials; };

static double timed(const cgx::GemvPlan &pl, const double *A, long lda, int n, const Vecs &x, double *parts, hipEvent_t e0, hipEvent_t e1)
{
    std::vector<float> ms;
    for (int rep = 0; rep < 22; ++rep) {
        CHECK(hipEventRecord(e0));
        CHECK(cgx::launch_symv_plain(pl, A, lda, n, x.v, parts, x.Ap, x.partials, 0));
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float t = 0;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    return 0.5 * (ms[ms.size() / 2 - 1] + ms[ms.size() / 2]);
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 32768;
    const int K = argc > 2 ? std::min(std::max(atoi(argv[2]), 1), 16) : 6;
    const int run = argc > 3 ? atoi(argv[3]) : cgx::kSymvRun;
    if (n <= 256) { fprintf(stderr, "n must be above 256\n"); return 1; }
    const long lda = ((long)n + 15) / 16 * 16 + 16;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const cgx::GemvPlan pl = cgx::plan_symv(n, lda, prop.multiProcessorCount, run);
    const int Sr = (n + 1) / 2 * 2;
    const size_t abytes = (size_t)n * lda * sizeof(double), pbytes = (size_t)pl.split * lda * sizeof(double);
    double *A[2];
    for (auto &a : A) {
        CHECK(hipMalloc(&a, abytes));
        CHECK(hipMemset(a, 0, abytes));
    }
    std::vector<double *> parts(K), spacer(2 * K);
    std::vector<Vecs> vecs(K);
    for (int k = 0; k < K; ++k) {
        CHECK(hipMalloc(&spacer[2 * k], (size_t)(k * 1300 + 7) * 1024));
        CHECK(hipMalloc(&parts[k], pbytes));
        CHECK(hipMemset(parts[k], 0, pbytes));
        CHECK(hipMalloc(&spacer[2 * k + 1], (size_t)(k * 37 + 3) * 4096));
        CHECK(hipMalloc(&vecs[k].v, lda * sizeof(double)));
        CHECK(hipMemset(vecs[k].v, 0, lda * sizeof(double)));
        CHECK(hipMalloc(&vecs[k].Ap, (size_t)(Sr + 16) * sizeof(double)));
        CHECK(hipMalloc(&vecs[k].partials, (size_t)(pl.light + 16) * sizeof(double)));
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    timed(pl, A[0], lda, n, vecs[0], parts[0], e0, e1);   // warm
    printf("{\"n\": %d, \"grid\": %d, \"A\": [\"%p\", \"%p\"]}\n", n, pl.grid, (void *)A[0], (void *)A[1]);
    for (int round = 0; round < 2; ++round) {
        for (int k = 0; k < K; ++k)
            printf("{\"round\": %d, \"vary\": \"parts\", \"k\": %d, \"parts\": \"%p\", \"ms\": %.4f}\n", round, k, (void *)parts[k],
                   timed(pl, A[0], lda, n, vecs[0], parts[k], e0, e1));
        for (int k = 0; k < K; ++k)
            printf("{\"round\": %d, \"vary\": \"vectors\", \"k\": %d, \"v\": \"%p\", \"Ap\": \"%p\", \"partials\": \"%p\", \"ms\": %.4f}\n", round, k,
                   (void *)vecs[k].v, (void *)vecs[k].Ap, (void *)vecs[k].partials, timed(pl, A[0], lda, n, vecs[k], parts[0], e0, e1));
        for (int a = 0; a < 2; ++a)
            printf("{\"round\": %d, \"vary\": \"A\", \"k\": %d, \"ms\": %.4f}\n", round, a, timed(pl, A[a], lda, n, vecs[0], parts[0], e0, e1));
    }
    return 0;
}
