// Micro-benchmark (development tool): phase timing of the packed LSTM-cell kernel (pk_kernel<0>) at the decode shapes.
// hipcc --offload-arch=gfx950 -O3 -o mb_pk mb_pk.hip ../../semi_tts_amd/csrc/runtime.hip ../../semi_tts_amd/csrc/attention_bwd.hip
#include <hip/hip_runtime.h>
__device__ unsigned long long g_prof[256 * 8 * 8];
#define PK_PROF(n) do { if ((threadIdx.x & 63) == 0) g_prof[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + (n)] = __builtin_readcyclecounter(); } while (0)
#include "../../semi_tts_amd/csrc/skinny_packed.hip"
#include <cstdio>
#include <vector>
#include <cstdlib>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)

// touches the first `kbs` k-blocks of every tile's packed weights (and nothing else): does a warm L2 / TLB shorten the start of
// the next kernel?  WG t of this kernel and WG t of the LSTM kernel land on the same XCD (round-robin dispatch).
// (round 3: the 2-D tiled cell gives workgroup x the row tiles 2x and 2x+1, so prefetch workgroup x touches exactly those two)
__global__ __launch_bounds__(512) void prefetch_kernel(const f32x4* w, int w_kbs, int kbs, float* sink) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int rt = 0; rt < 2; ++rt)
        for (int k = wave; k < kbs; k += 8) { const f32x4 v = w[((size_t)(2 * blockIdx.x + rt) * w_kbs + k) * 64 + lane]; acc[0] += v[0]; acc[1] += v[1]; }
    if (acc[0] == 12345.678f) sink[0] = acc[1];
}

int main() {
    const int B = 32, H = 1024;
    for (int K : {256, 1792, 2560}) {
        int ks[1] = {K};
        size_t wf = st_packed_weight_floats(ks, 1, 4 * H, H), xf = st_t16_floats(B, K), hf = st_t16_floats(B, H);
        float *w, *x, *h0, *h1, *ha, *c0, *c1, *bi, *bh, *as, *am;
        CK(hipMalloc(&w, wf * 4)); CK(hipMalloc(&x, xf * 4)); CK(hipMalloc(&h0, hf * 4)); CK(hipMalloc(&h1, hf * 4)); CK(hipMalloc(&ha, hf * 4));
        CK(hipMalloc(&c0, B * H * 4)); CK(hipMalloc(&c1, B * H * 4)); CK(hipMalloc(&bi, 4 * H * 4)); CK(hipMalloc(&bh, 4 * H * 4));
        CK(hipMalloc(&as, B * H * 4)); CK(hipMalloc(&am, B * H * 4));
        CK(hipMemset(w, 0, wf * 4)); CK(hipMemset(x, 0, xf * 4)); CK(hipMemset(c0, 0, B * H * 4)); CK(hipMemset(bi, 0, 16 * H)); CK(hipMemset(bh, 0, 16 * H));
        CK(hipMemset(as, 0, B * H * 4)); CK(hipMemset(am, 0, B * H * 4)); CK(hipMemset(h0, 0, hf * 4)); CK(hipMemset(h1, 0, hf * 4)); CK(hipMemset(ha, 0, hf * 4));
        st_t16_view xv = {x, (K + 15) / 16, 0}, d0 = {h0, H / 16, 0}, d1 = {h1, H / 16, 0}, da = {ha, H / 16, 0};
        const st_lstm_cell_packed_job j = {w, xv, K, bi, bh, c0, H, nullptr, d0, d1, c1, H, nullptr, as, am, da, B, H, nullptr, 0};
        auto run = [&] { int rc = st_lstm_cell_packed_fwd(&j, nullptr);
            if (rc) { printf("rc=%d %s\n", rc, st_last_error()); exit(1); } };
        float* sink; CK(hipMalloc(&sink, 64));
        float* junk; CK(hipMalloc(&junk, 64 << 20));
        // variant timings: (a) LSTM alone after an unrelated 64 MB memset (cold), (b) prefetch kernel first
        for (int variant = 0; variant < 3; ++variant) {
            hipEvent_t a0, a1; CK(hipEventCreate(&a0)); CK(hipEventCreate(&a1));
            float tot = 0;
            for (int it = 0; it < 20; ++it) {
                CK(hipMemsetAsync(junk, it, 64 << 20, nullptr));                 // evict L2 / MALL-ish
                if (variant == 1) hipLaunchKernelGGL(prefetch_kernel, dim3(H / 8), dim3(512), 0, nullptr, (const f32x4*)w, (K + 15) / 16, ((K + 15) / 16 < 32 ? (K + 15) / 16 : 32), sink);
                if (variant == 2) hipLaunchKernelGGL(prefetch_kernel, dim3(H / 8), dim3(512), 0, nullptr, (const f32x4*)w, (K + 15) / 16, (K + 15) / 16, sink);
                CK(hipEventRecord(a0)); run(); CK(hipEventRecord(a1)); CK(hipEventSynchronize(a1));
                float ms; CK(hipEventElapsedTime(&ms, a0, a1)); tot += ms;
            }
            printf("K=%4d variant %d (%s): LSTM launch %.2f us (event to event)\n", K, variant,
                   variant == 0 ? "cold" : (variant == 1 ? "first 32 k-blocks of each tile prefetched" : "whole matrix prefetched"), tot * 1e3 / 20);
        }
        for (int i = 0; i < 5; ++i) run();
        CK(hipDeviceSynchronize());
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        CK(hipEventRecord(e0));
        for (int i = 0; i < 200; ++i) run();
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        std::vector<unsigned long long> hp(256 * 8 * 8);
        CK(hipMemcpyFromSymbol(hp.data(), HIP_SYMBOL(g_prof), hp.size() * 8));
        printf("K=%4d: %.2f us/launch (back-to-back, independent).  cycles since the workgroup's own wave-0 start (clocks of different XCDs are not comparable), over 256 workgroups:\n", K, ms * 1e3 / 200);
        const char* names[6] = {"wave start", "first loads issued", "first group multiplied", "K loop done", "LDS reduce synced", "epilogue done"};
        const int order[7] = {6, 7, 1, 2, 3, 4, 5};
        const char* nm[8] = {"wave start", "first group data in", "first group multiplied", "K loop done", "LDS reduce synced", "epilogue done",
                             "kernargs in, pointers set", "epilogue operands requested"};
        for (int oi = 0; oi < 7; ++oi) {
            const int n = order[oi];
            names[n < 6 ? n : 0] = names[n < 6 ? n : 0];
            std::vector<long long> v;
            for (int b = 0; b < 256; ++b) v.push_back((long long)(hp[(b * 8 + 0) * 8 + n] - hp[(b * 8 + 0) * 8 + 0]));
            std::sort(v.begin(), v.end());
            printf("  %-28s min %7lld  median %7lld  max %7lld\n", nm[n], v[0], v[128], v[255]);
        }
    }
    // ---- the small linears of the decode step (MODE 1, one batch tile per workgroup): pq (K=1024 -> 256), prenet-2 (256 -> 256),
    // proj (+) gate (+) prenet-1 (1536 -> 497)
    for (int which = 0; which < 3; ++which) {
        const int K = which == 0 ? 1024 : which == 1 ? 256 : 1536, N = which == 2 ? 497 : 256;
        int ks[1] = {K};
        size_t wf = st_packed_weight_floats(ks, 1, N, 0), xf = st_t16_floats(B, K);
        float *w, *x, *y, *bias;
        CK(hipMalloc(&w, wf * 4)); CK(hipMalloc(&x, xf * 4)); CK(hipMalloc(&y, B * N * 4)); CK(hipMalloc(&bias, N * 4));
        CK(hipMemset(w, 0, wf * 4)); CK(hipMemset(x, 0, xf * 4)); CK(hipMemset(bias, 0, N * 4));
        st_t16_view xv = {x, (K + 15) / 16, 0};
        st_packed_linear_job lj = st_plain_linear_job(w, xv, K, y, N, B, N);
        lj.bias = bias; lj.act = which == 1 ? ST_ACT_RELU : ST_ACT_NONE;
        auto run = [&] { int rc = st_skinny_linear_packed_fwd(&lj, nullptr);
            if (rc) { printf("rc=%d %s\n", rc, st_last_error()); exit(1); } };
        float* junk; CK(hipMalloc(&junk, 64 << 20));
        for (int i = 0; i < 3; ++i) run();
        CK(hipDeviceSynchronize());
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        float tot = 0;
        for (int it = 0; it < 50; ++it) {
            CK(hipMemsetAsync(junk, it, 64 << 20, nullptr));
            CK(hipEventRecord(e0)); run(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1)); tot += ms;
        }
        const int tiles = (N + 15) / 16;
        std::vector<unsigned long long> hp(256 * 8 * 8);
        CK(hipMemcpyFromSymbol(hp.data(), HIP_SYMBOL(g_prof), hp.size() * 8));
        printf("linear K=%d N=%d: %.2f us/launch (event to event, cold L2); cycles since wave-0 start over %d tiles:\n", K, N, tot * 1e3 / 50, tiles);
        const int order[7] = {6, 7, 1, 2, 3, 4, 5};
        const char* nm[8] = {"wave start", "first group data in", "first group multiplied", "K loop done", "LDS reduce synced", "epilogue done",
                             "kernargs in, pointers set", "loads + epilogue operands requested"};
        for (int oi = 0; oi < 7; ++oi) {
            const int n = order[oi];
            std::vector<long long> v;
            for (int b = 0; b < tiles; ++b) v.push_back((long long)(hp[(b * 8 + 0) * 8 + n] - hp[(b * 8 + 0) * 8 + 0]));
            std::sort(v.begin(), v.end());
            printf("  %-36s min %7lld  median %7lld  max %7lld\n", nm[n], v[0], v[tiles / 2], v[tiles - 1]);
        }
    }
    return 0;
}
