// times the two stages of the 5-point solver (csrc/emat_lds.h) in the launch shapes of emat_hyp_kernel and emat_roots_kernel
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I../../include -I../../map-free-reloc_amd/csrc -o fivept_time fivept_time.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <random>
#include "emat_lds.h"
using namespace mfr;
#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)
// one lane per solve, as emat_hyp_kernel
__global__ void __launch_bounds__(64) front(const double *x0, const double *x1, double *Es, int *nsol)
{
    __shared__ double fp_lds[FP_LDS_DOUBLES * 64];
    __shared__ int fp_colp[9 * 64];
    const int it = blockIdx.x * 64 + threadIdx.x;
    double a[10], c[10];
    for (int q = 0; q < 10; ++q) { a[q] = x0[it * 10 + q]; c[q] = x1[it * 10 + q]; }
    nsol[it] = fivept_front_lds(a, c, Es + (size_t)it * FP_SLOT_DOUBLES, fp_lds + threadIdx.x, fp_colp + threadIdx.x);
}
// 8 lanes per solve, 32 solves per workgroup, as emat_roots_kernel
__global__ void __launch_bounds__(256) roots(double *Es, int *nsol, int total)
{
    __shared__ FprShared sh[FPR_HYP_PER_WG];
    const int g = threadIdx.x / FPR_GROUP, sub = threadIdx.x % FPR_GROUP;
    const int h = blockIdx.x * FPR_HYP_PER_WG + g;
    const bool active = h < total && nsol[h < total ? h : 0] == FP_NSOL_PENDING;
    fp_roots_group(Es + (size_t)(h < total ? h : 0) * FP_SLOT_DOUBLES, nsol + (h < total ? h : 0), &sh[g], sub, active);
}
int main()
{
    const int n = 250 * 64;
    std::mt19937 g(1); std::normal_distribution<double> nd(0, 0.3);
    std::vector<double> h0(n * 10), h1(n * 10);
    for (int i = 0; i < n; ++i) {                           // 5 points of a random two-view geometry: x1 ~ x0 + parallax
        for (int q = 0; q < 5; ++q) { double X = nd(g), Y = nd(g), Z = 3 + nd(g); h0[i * 10 + 2 * q] = X / Z; h0[i * 10 + 2 * q + 1] = Y / Z;
            h1[i * 10 + 2 * q] = (X + 0.3) / (Z + 0.05); h1[i * 10 + 2 * q + 1] = (Y + 0.02) / (Z + 0.05); }
    }
    double *d0, *d1, *Es; int *ns;
    CHECK(hipMalloc(&d0, n * 80)); CHECK(hipMalloc(&d1, n * 80));
    CHECK(hipMalloc(&Es, (size_t)n * FP_SLOT_DOUBLES * sizeof(double))); CHECK(hipMalloc(&ns, n * 4));
    CHECK(hipMemcpy(d0, h0.data(), n * 80, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d1, h1.data(), n * 80, hipMemcpyHostToDevice));
    const int rgrid = (n + FPR_HYP_PER_WG - 1) / FPR_HYP_PER_WG;
    hipEvent_t e0, e1, e2; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1)); CHECK(hipEventCreate(&e2));
    front<<<n / 64, 64>>>(d0, d1, Es, ns); roots<<<rgrid, 256>>>(Es, ns, n); CHECK(hipDeviceSynchronize());      // warm-up
    // the root stage consumes the records in place, so each timed root launch follows a front launch that wrote them
    CHECK(hipEventRecord(e0)); front<<<n / 64, 64>>>(d0, d1, Es, ns);
    CHECK(hipEventRecord(e1)); roots<<<rgrid, 256>>>(Es, ns, n);
    CHECK(hipEventRecord(e2)); CHECK(hipDeviceSynchronize());
    float ms_front, ms_roots; CHECK(hipEventElapsedTime(&ms_front, e0, e1)); CHECK(hipEventElapsedTime(&ms_roots, e1, e2));
    std::vector<int> hn(n); CHECK(hipMemcpy(hn.data(), ns, n * 4, hipMemcpyDeviceToHost));
    long tot = 0; for (int v : hn) tot += v;
    printf("%d solves: front end %.3f ms (%d workgroups of 64), root stage %.3f ms (%d workgroups of 256), mean solutions %.2f\n",
           n, ms_front, n / 64, ms_roots, rgrid, (double)tot / n);
    return 0;
}
