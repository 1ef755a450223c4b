// abx_ulp.hip -- the largest error, in ulps, of the device's atan2f, logf and sqrtf against the host's float64 functions over the
// arguments st_dtw_pairs passes them (tests/abx_oracle.py budgets twice these figures).  A program of its own:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/abx_ulp.hip -o abx_ulp && ./abx_ulp
// atan2f(p, q): p = 2 sin(phi), q = 2 cos(phi), phi in [0, pi / 2], half the samples at phi below 1e-3 (near-parallel frames), each
// perturbed by a few ulps; logf(z): z log-uniform in [1e-10, 2]; sqrtf(s): s log-uniform in [1e-12, 1e6].
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

__global__ void ulp_kernel(const float* a, const float* b, float* r_atan2, float* r_log, float* r_sqrt, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        r_atan2[i] = atan2f(a[i], b[i]);
        r_log[i] = logf(a[i]);
        r_sqrt[i] = sqrtf(a[i]);
    }
}

static double rnd(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

static double ulps(float got, double want) {
    int e;
    frexp(want, &e);                                            // |want| in [2^(e-1), 2^e): one ulp of a float there is 2^(e-24)
    const double ulp = ldexp(1.0, (e - 24 < -149) ? -149 : e - 24);
    return fabs((double)got - want) / ulp;
}

#define CHECK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    const int n = 1 << 22;
    std::vector<float> a(n), b(n), r0(n), r1(n), r2(n);
    float *da, *db, *d0, *d1, *d2;
    CHECK(hipMalloc(&da, n * 4)); CHECK(hipMalloc(&db, n * 4)); CHECK(hipMalloc(&d0, n * 4)); CHECK(hipMalloc(&d1, n * 4)); CHECK(hipMalloc(&d2, n * 4));
    uint64_t s = 12345;
    double worst[3] = {0, 0, 0};
    for (int pass = 0; pass < 3; ++pass) {
        for (int i = 0; i < n; ++i) {
            if (pass == 0) {
                const double phi = (i & 1) ? 1e-3 * rnd(s) * rnd(s) : 1.5707963267948966 * rnd(s);
                a[i] = (float)(2.0 * sin(phi) * (1.0 + 1e-6 * (rnd(s) - 0.5)));
                b[i] = (float)(2.0 * cos(phi) * (1.0 + 1e-6 * (rnd(s) - 0.5)));
            } else if (pass == 1) {
                a[i] = (float)exp(log(1e-10) + rnd(s) * (log(2.0) - log(1e-10)));
                b[i] = 1.0f;
            } else {
                a[i] = (float)exp(log(1e-12) + rnd(s) * (log(1e6) - log(1e-12)));
                b[i] = 1.0f;
            }
        }
        CHECK(hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(db, b.data(), n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ulp_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, da, db, d0, d1, d2, n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(r0.data(), d0, n * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(r1.data(), d1, n * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(r2.data(), d2, n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            double e;
            if (pass == 0) e = ulps(r0[i], atan2((double)a[i], (double)b[i]));
            else if (pass == 1) e = ulps(r1[i], log((double)a[i]));
            else e = ulps(r2[i], sqrt((double)a[i]));
            if (e > worst[pass]) worst[pass] = e;
        }
    }
    printf("{\"samples\": %d, \"atan2f_ulp\": %.4f, \"logf_ulp\": %.4f, \"sqrtf_ulp\": %.4f}\n", n, worst[0], worst[1], worst[2]);
    return 0;
}
