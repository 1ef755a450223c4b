// colreduce.h -- what grad.hip and batchnorm.hip both need: the activation derivative, the grid of the element-wise kernels and the merge
// of the row-split column reductions' chunk partials (st_colsum, st_bn_bwd_reduce)
#pragma once
#include "st_common.h"

namespace {

__device__ __forceinline__ float act_grad(float out, int act) {
    switch (act) {
        case ST_ACT_RELU: return out > 0.0f ? 1.0f : 0.0f;
        case ST_ACT_TANH: return 1.0f - out * out;
        case ST_ACT_SIGMOID: return out * (1.0f - out);
        default: return 1.0f;
    }
}

// out[q][n] (+)= sum_chunks part[chunk][q][n], q < Q.  16 (q, n) pairs x 16 chunk lanes per workgroup: lane j adds chunks j, j + 16, ...
// (at most 8, all loads issued at once), the lanes' sums are combined through LDS in a fixed order.
__global__ __launch_bounds__(256) void chunk_final_kernel(const float* part, int chunks, int Q, int N, float* out0, float* out1,
                                                          int accumulate) {
    constexpr int CL = 16, PER = 8;
    static_assert(CL * PER >= ST_COLREDUCE_MAX_CHUNKS, "every chunk needs a register");
    __shared__ float red[CL][16];
    const int c = threadIdx.x & 15, cl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + c;
    const bool ok = i < Q * N;
    const int ic = min(i, Q * N - 1);
    const int q = ic / N, n = ic - q * N;
    const float* p = part + (size_t)q * N + n;
    const size_t cs = (size_t)Q * N;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) { const int ch = cl + j * CL; v[j] = p[(size_t)(ch < chunks ? ch : 0) * cs] * (ch < chunks ? 1.0f : 0.0f); }   // (a factor, not a select: no branch + wait per load)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += v[j];
    red[cl][c] = s;
    __syncthreads();
    if (cl != 0 || !ok) return;
    float* out = q == 0 ? out0 : out1;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < CL; ++k) t += red[k][c];
    out[n] = accumulate ? out[n] + t : t;
}

inline int blocks_for(size_t n, int cap = 4096) {
    size_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    return (int)(b > (size_t)cap ? cap : b);
}

}  // namespace
