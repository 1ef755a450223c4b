// batchnorm.hip -- training-mode BatchNorm1d for gfx950 (MI355X): batch statistics and their SyncBN record / merge, the normalisation
// kernels, the two halves of the backward, and the K layers of a conv bank as one launch per stage (st_bn_bank_fwd / st_bn_bank_bwd).
//
// The statistics exist once: segment-indexed kernels over a BnBank.  st_bn_stats / st_bn_stats_record / st_bn_sync_merge run them on a
// bank of one segment.  (st_prenet_norm_* -- the decode step's BatchNorm over the rows of one step -- is norm.hip's.)
#include "colreduce.h"

namespace {

__global__ __launch_bounds__(256) void bn_apply_kernel(float* X, int ldx, int coff, int M, int N,
                                                       const float* mean, const float* var, const float* w,
                                                       const float* b, float eps, int act) {
    const size_t total = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
        float* p = X + (size_t)m * ldx + coff + n;
        float v = (*p - mean[n]) / sqrtf(var[n] + eps);
        v = v * (w ? w[n] : 1.0f) + (b ? b[n] : 0.0f);
        *p = st_act(v, act);
    }
}

// out-of-place BatchNorm normalisation: Y = act((X - mean) / sqrt(var + eps) * w + b); X is kept for the backward
__global__ __launch_bounds__(256) void bn_norm_fwd_kernel(const float* X, int ldx, int xoff, float* Y, int ldy, int yoff,
                                                          int M, int N, const float* mean, const float* var, const float* w,
                                                          const float* b, float eps, int act) {
    const size_t total = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / N;
        const int n = (int)(i - m * N);
        float v = (X[m * ldx + xoff + n] - mean[n]) / sqrtf(var[n] + eps);
        v = v * (w ? w[n] : 1.0f) + (b ? b[n] : 0.0f);
        Y[m * ldy + yoff + n] = st_act(v, act);
    }
}

// ConvLayer's tail in training (src/module.py:641-646): T = act(BatchNorm(X)) kept for the backward, Y = (T + res) * mask the layer's output
// (res, mask optional); 16-byte pieces (N % 4 == 0, all rows 16-byte aligned)
__global__ __launch_bounds__(256) void bn_norm_res_mask_fwd_kernel(const float* __restrict__ X, float* __restrict__ Tact, float* __restrict__ Y,
                                                                   int N4, size_t total4, const float* __restrict__ mean,
                                                                   const float* __restrict__ var, const float* __restrict__ w,
                                                                   const float* __restrict__ b, float eps, int act,
                                                                   const float* __restrict__ res, const float* __restrict__ mask) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const int n = 4 * (int)(i % N4);
        const f32x4 x = st_ld4(X + 4 * i), mu = st_ld4(mean + n), vr = st_ld4(var + n);
        f32x4 g = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f}, r = {0.f, 0.f, 0.f, 0.f}, k = {1.f, 1.f, 1.f, 1.f};
        if (w) g = st_ld4(w + n);
        if (b) be = st_ld4(b + n);
        if (res) r = st_ld4(res + 4 * i);
        if (mask) k = st_ld4(mask + 4 * i);
        f32x4 t, y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = (x[j] - mu[j]) / sqrtf(vr[j] + eps);           // (bn_norm_fwd_kernel's expression, element for element)
            v = v * g[j] + be[j];
            t[j] = st_act(v, act);
            y[j] = (t[j] + r[j]) * k[j];
        }
        if (Tact) *reinterpret_cast<f32x4*>(Tact + 4 * i) = t;
        *reinterpret_cast<f32x4*>(Y + 4 * i) = y;
    }
}

// BatchNorm (batch statistics) backward.  y = act((x - mean) / sqrt(var + eps) * w + b).
//   pass 1 (bn_bwd_reduce): s1[n] = sum dyb, s2[n] = sum dyb * xhat     with dyb = dy * act'(y)
//   pass 2 (bn_bwd_apply):  dx = w / sigma * (dyb - s1/M - xhat * s2/M)
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* dy, int ldd, int doff, const float* y, int ldy, int yoff,
                                                            int act, const float* x, int ldx, int xoff, const float* mean,
                                                            const float* var, float eps, int M, int N, int rows_per_chunk,
                                                            float* part, const float* mask = nullptr, int ldm = 0) {   // part[chunk][2][N]
    __shared__ float r1[4][64], r2[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int nc = min(n, N - 1);
    const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
    const float mu = mean[nc], inv = 1.0f / sqrtf(var[nc] + eps);
    const float* __restrict__ dp = dy + doff + nc;
    const float* __restrict__ xp = x + xoff + nc;
    const float* __restrict__ yp = act != ST_ACT_NONE ? y + yoff + nc : nullptr;
    const float* __restrict__ kp = mask ? mask + nc : nullptr;        // dropout mask behind the activation: dyb = dy * mask * act'(y)
    // two rows per pass with independent sums: (up to) six loads in flight per thread instead of a chain of dependent round trips
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    int m = m0 + rl;
    for (; m + 4 < m1; m += 8) {
        float g0 = dp[(size_t)m * ldd], g1 = dp[(size_t)(m + 4) * ldd];
        const float x0 = xp[(size_t)m * ldx], x1 = xp[(size_t)(m + 4) * ldx];
        if (kp) { g0 *= kp[(size_t)m * ldm]; g1 *= kp[(size_t)(m + 4) * ldm]; }
        if (yp) { g0 *= act_grad(yp[(size_t)m * ldy], act); g1 *= act_grad(yp[(size_t)(m + 4) * ldy], act); }
        a0 += g0; a1 += g1;
        b0 = fmaf(g0, (x0 - mu) * inv, b0); b1 = fmaf(g1, (x1 - mu) * inv, b1);
    }
    for (; m < m1; m += 4) {
        float g = dp[(size_t)m * ldd];
        if (kp) g *= kp[(size_t)m * ldm];
        if (yp) g *= act_grad(yp[(size_t)m * ldy], act);
        a0 += g;
        b0 = fmaf(g, (xp[(size_t)m * ldx] - mu) * inv, b0);
    }
    r1[rl][c] = a0 + a1; r2[rl][c] = b0 + b1;
    __syncthreads();
    if (rl == 0 && n < N) {
        part[((size_t)blockIdx.y * 2 + 0) * N + n] = r1[0][c] + r1[1][c] + r1[2][c] + r1[3][c];
        part[((size_t)blockIdx.y * 2 + 1) * N + n] = r2[0][c] + r2[1][c] + r2[2][c] + r2[3][c];
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* dy, int ldd, int doff, const float* y, int ldy, int yoff,
                                                           int act, const float* x, int ldx, int xoff, const float* mean,
                                                           const float* var, const float* w, float eps, int M, int N,
                                                           const float* s1, const float* s2, float* dx, int lddx, int dxoff,
                                                           int Mstat, const float* inv_total, const float* mask = nullptr, int ldm = 0,
                                                           float* dres = nullptr, int lddr = 0) {
    const size_t total = (size_t)M * N;
    // rows the statistics (and s1, s2) were taken over: > M under SyncBN, where 1 / (global row count) comes as a device scalar
    const float invM = inv_total ? inv_total[0] : 1.0f / (float)Mstat;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / N;
        const int n = (int)(i - m * N);
        float g = dy[m * ldd + doff + n];
        if (mask) g *= mask[m * ldm + n];
        if (dres) dres[m * lddr + n] = g;          // the gradient of a residual input added behind the activation, in front of the mask
        if (act != ST_ACT_NONE) g *= act_grad(y[m * ldy + yoff + n], act);
        const float inv = 1.0f / sqrtf(var[n] + eps);
        const float xh = (x[m * ldx + xoff + n] - mean[n]) * inv;
        dx[m * lddx + dxoff + n] = (w ? w[n] : 1.0f) * inv * (g - s1[n] * invM - xh * s2[n] * invM);
    }
}

// ---- K BatchNorm1d layers of equal width as segments of one launch ----------------------------------------------------------------------------
// A conv bank's K layers (st_bn_bank_fwd / st_bn_bank_bwd), or ONE layer: the statistics, record and merge kernels below are the only ones
// there are, and st_bn_stats / st_bn_stats_record / st_bn_sync_merge run them on a bank of one segment (x = X + coff, Bn = 1, T = M) -- the
// same rows per chunk and the same merge order whatever the segment count.  Output, sums and dx of a one-segment bank against the
// per-layer st_bn_norm_fwd / st_bn_bwd_reduce / st_bn_bwd_apply are still two kernels each: the first two agree bit for bit (same chunking,
// same order), dx to rounding -- the two apply kernels compile to different multiply-add sequences.  part: [seg][chunk][2][N].
struct BnBank { st_bn_bank_seg s[ST_BN_BANK_MAX]; int nseg, Bn, N; };

// column statistics, two launches: (1) grid = (column blocks of 64, row chunks, segments): every block reduces its chunk of
// rows to (mean_c, M2_c) with a chunk-local two-pass (the second pass re-reads <= 64 KB from cache);
// (2) the chunks are merged in a fixed order (Chan et al.: exact pairwise update of mean / M2).
// The grid is sized for the segment with the most chunks: blocks past a segment's own chunk count return.
__global__ __launch_bounds__(256) void bnb_stats_chunk_kernel(const BnBank a, float* part, int max_chunks) {
    __shared__ float red[4][64];
    __shared__ float smean[64];
    const st_bn_bank_seg& sg = a.s[blockIdx.z];
    const int N = a.N, M = a.Bn * sg.T;
    const int chunks = st_colreduce_chunks(M), rpc = (M + chunks - 1) / chunks;
    if ((int)blockIdx.y >= chunks) return;
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const bool ok = n < N;
    const int m0 = blockIdx.y * rpc, m1 = min(M, m0 + rpc);
    const int ldx = sg.ldx;
    const float* __restrict__ xp = sg.x + min(n, N - 1);
    // rows m0 + rl, + 4, ...: four independent running sums (rows 16 apart) keep four loads in flight per thread -- with one sum the
    // loop is a chain of dependent round trips (12.9 us per 4 MB layer in round 2's form)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int m = m0 + rl;
    for (; m + 12 < m1; m += 16) {
        s0 += xp[(size_t)m * ldx]; s1 += xp[(size_t)(m + 4) * ldx]; s2 += xp[(size_t)(m + 8) * ldx]; s3 += xp[(size_t)(m + 12) * ldx];
    }
    for (; m < m1; m += 4) s0 += xp[(size_t)m * ldx];
    red[rl][c] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rl == 0) smean[c] = (red[0][c] + red[1][c] + red[2][c] + red[3][c]) / (float)max(m1 - m0, 1);      // (an empty last chunk: m1 <= m0)
    __syncthreads();
    const float mean = smean[c];
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
    m = m0 + rl;
    for (; m + 12 < m1; m += 16) {      // (second pass: the chunk's rows come from cache)
        const float d0 = xp[(size_t)m * ldx] - mean, d1 = xp[(size_t)(m + 4) * ldx] - mean;
        const float d2 = xp[(size_t)(m + 8) * ldx] - mean, d3 = xp[(size_t)(m + 12) * ldx] - mean;
        q0 = fmaf(d0, d0, q0); q1 = fmaf(d1, d1, q1); q2 = fmaf(d2, d2, q2); q3 = fmaf(d3, d3, q3);
    }
    for (; m < m1; m += 4) { const float d = xp[(size_t)m * ldx] - mean; q0 = fmaf(d, d, q0); }
    __syncthreads();
    red[rl][c] = (q0 + q1) + (q2 + q3);
    __syncthreads();
    if (rl == 0 && ok) {
        float* pp = part + ((size_t)blockIdx.z * max_chunks + blockIdx.y) * 2 * N;
        pp[n] = mean;
        pp[N + n] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    }
}

// merge of the chunk records: 16 columns x 16 chunk lanes per workgroup; lane j holds chunks j, j + 16, ... (at most 8) in REGISTERS -- all
// its loads are issued at once, one memory round trip for both sweeps -- and the 16 lanes' sums are combined through LDS in a fixed order.
//   mean = sum_c n_c mean_c / M;   M2 = sum_c [M2_c + n_c (mean_c - mean)^2]      (exact decomposition, Chan et al.)
// (one thread per column walking all the chunks took 16 us per layer: 2 x 64 dependent-latency iterations)
// rec != NULL (SyncBN, local half): (mean, M2, row count) of segment k go to rec[k (2N + 1) ..]; nothing else is written but batches_tracked
__global__ __launch_bounds__(256) void bnb_stats_final_kernel(const BnBank a, const float* part, int max_chunks, float* rec) {
    constexpr int CL = 16, PER = 8;
    static_assert(CL * PER >= ST_COLREDUCE_MAX_CHUNKS, "every chunk needs a register");
    __shared__ float red[CL][16];
    __shared__ float smean[16];
    const st_bn_bank_seg& sg = a.s[blockIdx.y];
    const int N = a.N, M = a.Bn * sg.T;
    const int chunks = st_colreduce_chunks(M), rpc = (M + chunks - 1) / chunks;
    const int c = threadIdx.x & 15, cl = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + c;
    if (blockIdx.x == 0 && threadIdx.x == 0 && sg.batches_tracked) sg.batches_tracked[0] += 1;      // nn.BatchNorm1d.num_batches_tracked, without a launch of its own
    const bool ok = n < N;
    const float* pm = part + (size_t)blockIdx.y * max_chunks * 2 * N + min(n, N - 1);
    const size_t cs = (size_t)2 * N;
    float mu[PER], m2[PER], cnt[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int ch = cl + j * CL;
        const bool in = ch < chunks;
        const int chc = in ? ch : 0;
        // (absent chunks re-read chunk 0 and are zeroed by a FACTOR: `if (!in) m2 = 0` makes the compiler branch around the load and wait)
        mu[j] = pm[(size_t)chc * cs]; m2[j] = pm[(size_t)chc * cs + N] * (in ? 1.0f : 0.0f);
        cnt[j] = in ? (float)max(min(M, (ch + 1) * rpc) - ch * rpc, 0) : 0.0f;
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) acc = fmaf(cnt[j], mu[j], acc);
    red[cl][c] = acc;
    __syncthreads();
    if (cl == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < CL; ++k) t += red[k][c];
        smean[c] = t / (float)M;
    }
    __syncthreads();
    const float mean = smean[c];
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { const float d = mu[j] - mean; q += m2[j] + cnt[j] * d * d; }
    __syncthreads();
    red[cl][c] = q;
    __syncthreads();
    if (cl != 0 || !ok) return;
    float m2t = 0.f;
#pragma unroll
    for (int k = 0; k < CL; ++k) m2t += red[k][c];
    const float var_b = m2t / (float)M;
    if (rec) {
        float* r = rec + (size_t)blockIdx.y * (2 * N + 1);
        r[n] = mean; r[N + n] = m2t;
        if (n == 0) r[2 * N] = (float)M;
        return;
    }
    sg.mean[n] = mean;
    sg.var[n] = var_b;
    if (sg.run_mean) {
        const float var_u = M > 1 ? m2t / (float)(M - 1) : var_b;
        sg.run_mean[n] = (1.0f - sg.momentum) * sg.run_mean[n] + sg.momentum * mean;
        sg.run_var[n] = (1.0f - sg.momentum) * sg.run_var[n] + sg.momentum * var_u;
    }
}

// SyncBN, merged half for all segments: allrec (world, nseg, 2N + 1) gathered records -> mean / var of the global batch of every segment,
// merged exactly and in rank order (Chan et al.), identically on every rank; running statistics updated as nn.BatchNorm1d does (unbiased
// variance over the GLOBAL row count); 1 / (global row count) per segment, the factor the backward's two sums are divided by
__global__ __launch_bounds__(256) void bnb_sync_merge_kernel(const BnBank a, const float* allrec, int world, float* inv_total_out) {
    const int k = blockIdx.y;
    const st_bn_bank_seg& sg = a.s[k];
    const int N = a.N;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t rs = (size_t)2 * N + 1, ws_ = rs * a.nseg;
    const float* rec = allrec + (size_t)k * rs;
    float total = 0.0f;
    for (int r = 0; r < world; ++r) total += rec[r * ws_ + 2 * N];
    if (n == 0) inv_total_out[k] = 1.0f / total;
    if (n >= N) return;
    float acc = 0.0f;
    for (int r = 0; r < world; ++r) acc = fmaf(rec[r * ws_ + 2 * N], rec[r * ws_ + n], acc);
    const float mean = acc / total;
    float m2 = 0.0f;
    for (int r = 0; r < world; ++r) { const float d = rec[r * ws_ + n] - mean; m2 += rec[r * ws_ + N + n] + rec[r * ws_ + 2 * N] * d * d; }
    sg.mean[n] = mean;
    sg.var[n] = m2 / total;
    if (sg.run_mean) {
        sg.run_mean[n] = (1.0f - sg.momentum) * sg.run_mean[n] + sg.momentum * mean;
        sg.run_var[n] = (1.0f - sg.momentum) * sg.run_var[n] + sg.momentum * (m2 / fmaxf(total - 1.0f, 1.0f));
    }
}

// Y[(b Tout + t)][k N + n] = BN_k(x_k[b T_k + t][n]), t < Tout.  blockIdx.y = segment (its fields stay in scalar registers); four
// channels per thread when N % 4 == 0 and the rows are 16-byte addressable
__global__ __launch_bounds__(256) void bnb_norm_kernel(const BnBank a, float* __restrict__ Y, int ldy, int Tout, int vec) {
    const int k = blockIdx.y;
    const st_bn_bank_seg& sg = a.s[k];
    const int N = a.N, T = sg.T, ldx = sg.ldx;
    const float* __restrict__ x = sg.x;
    if (vec) {
        const int N4 = N >> 2;
        const size_t total = (size_t)a.Bn * Tout * N4;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
            const size_t r = i / N4;
            const int n = (int)(i - r * N4) * 4;
            const int b = (int)(r / Tout), t = (int)(r - (size_t)b * Tout);
            const f32x4 xv = st_ld4(x + ((size_t)b * T + t) * ldx + n);
            const f32x4 mu = st_ld4(sg.mean + n), va = st_ld4(sg.var + n);
            const f32x4 w4 = sg.w ? st_ld4(sg.w + n) : f32x4{1.f, 1.f, 1.f, 1.f}, b4 = sg.b ? st_ld4(sg.b + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = (xv[c] - mu[c]) / sqrtf(va[c] + sg.eps) * w4[c] + b4[c];
            *reinterpret_cast<f32x4*>(Y + r * ldy + (size_t)k * N + n) = o;
        }
        return;
    }
    const size_t total = (size_t)a.Bn * Tout * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / N;
        const int n = (int)(i - r * N);
        const int b = (int)(r / Tout), t = (int)(r - (size_t)b * Tout);
        float v = (x[((size_t)b * T + t) * ldx + n] - sg.mean[n]) / sqrtf(sg.var[n] + sg.eps);
        v = v * (sg.w ? sg.w[n] : 1.0f) + (sg.b ? sg.b[n] : 0.0f);
        Y[r * ldy + (size_t)k * N + n] = v;
    }
}

__global__ __launch_bounds__(256) void bnb_bwd_reduce_kernel(const BnBank a, const float* __restrict__ dY, int lddy, int Tout, float* part, int max_chunks) {
    __shared__ float r1[4][64], r2[4][64];
    const int k = blockIdx.z;
    const st_bn_bank_seg& sg = a.s[k];
    const int N = a.N, T = sg.T, M = a.Bn * T;
    const int chunks = st_colreduce_chunks(M), rpc = (M + chunks - 1) / chunks;
    if ((int)blockIdx.y >= chunks) return;
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int nc = min(n, N - 1);
    const int m0 = blockIdx.y * rpc, m1 = min(M, m0 + rpc);
    const float mu = sg.mean[nc], inv = 1.0f / sqrtf(sg.var[nc] + sg.eps);
    const float* __restrict__ dp = dY + (size_t)k * N + nc;
    const float* __restrict__ xp = sg.x + nc;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    // rows whose frame lies past the bank (t >= Tout: the trimmed position of an even-k conv) have dy = 0 and add nothing
    auto dyrow = [&](int m) -> float {
        const int b = m / T, t = m - b * T;
        const float v = dp[((size_t)b * Tout + min(t, Tout - 1)) * lddy];
        return v * (t < Tout ? 1.0f : 0.0f);
    };
    int m = m0 + rl;
    for (; m + 4 < m1; m += 8) {
        const float g0 = dyrow(m), g1 = dyrow(m + 4);
        const float x0 = xp[(size_t)m * sg.ldx], x1 = xp[(size_t)(m + 4) * sg.ldx];
        a0 += g0; a1 += g1;
        b0 = fmaf(g0, (x0 - mu) * inv, b0); b1 = fmaf(g1, (x1 - mu) * inv, b1);
    }
    for (; m < m1; m += 4) {
        const float g = dyrow(m);
        a0 += g;
        b0 = fmaf(g, (xp[(size_t)m * sg.ldx] - mu) * inv, b0);
    }
    r1[rl][c] = a0 + a1; r2[rl][c] = b0 + b1;
    __syncthreads();
    if (rl == 0 && n < N) {
        float* pp = part + ((size_t)k * max_chunks + blockIdx.y) * 2 * N;
        pp[n] = r1[0][c] + r1[1][c] + r1[2][c] + r1[3][c];
        pp[N + n] = r2[0][c] + r2[1][c] + r2[2][c] + r2[3][c];
    }
}

// sums_k[q][n] = sum over the segment's chunks of part[k][chunk][q][n]   (chunk_final_kernel's merge order)
__global__ __launch_bounds__(256) void bnb_bwd_final_kernel(const BnBank a, const float* part, int max_chunks) {
    constexpr int CL = 16, PER = 8;
    static_assert(CL * PER >= ST_COLREDUCE_MAX_CHUNKS, "every chunk needs a register");
    __shared__ float red[CL][16];
    const st_bn_bank_seg& sg = a.s[blockIdx.y];
    const int N = a.N, M = a.Bn * sg.T;
    const int chunks = st_colreduce_chunks(M);
    const int c = threadIdx.x & 15, cl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + c;
    const bool ok = i < 2 * N;
    const int ic = min(i, 2 * N - 1);
    const float* p = part + (size_t)blockIdx.y * max_chunks * 2 * N + ic;
    const size_t cs = (size_t)2 * N;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) { const int ch = cl + j * CL; v[j] = p[(size_t)(ch < chunks ? ch : 0) * cs] * (ch < chunks ? 1.0f : 0.0f); }
    float sacc = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) sacc += v[j];
    red[cl][c] = sacc;
    __syncthreads();
    if (cl != 0 || !ok) return;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < CL; ++k) t += red[k][c];
    sg.sums[ic] = t;
}

__global__ __launch_bounds__(256) void bnb_bwd_apply_kernel(const BnBank a, const float* __restrict__ dY, int lddy, int Tout, int relu_in, int vec,
                                                            const float* __restrict__ inv_total) {
    const int k = blockIdx.y;
    const st_bn_bank_seg& sg = a.s[k];
    const int N = a.N, T = sg.T, M = a.Bn * T;
    // SyncBN: the sums were taken over every rank's rows; 1 / (global row count) of the segment comes as a device scalar
    const float invM = inv_total ? inv_total[k] : 1.0f / (float)M;
    if (vec) {      // four channels per thread (N % 4 == 0, 16-byte addressable rows): one row / frame split per four elements
        const int N4 = N >> 2;
        const size_t total = (size_t)M * N4;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
            const int m = (int)(i / N4), n = (int)(i - (size_t)m * N4) * 4;
            const int b = m / T, t = m - b * T;
            const f32x4 g4 = st_ld4(dY + ((size_t)b * Tout + min(t, Tout - 1)) * lddy + (size_t)k * N + n);
            const f32x4 xv = st_ld4(sg.x + (size_t)m * sg.ldx + n);
            const f32x4 mu = st_ld4(sg.mean + n), va = st_ld4(sg.var + n), s1 = st_ld4(sg.sums + n), s2 = st_ld4(sg.sums + N + n);
            const f32x4 w4 = sg.w ? st_ld4(sg.w + n) : f32x4{1.f, 1.f, 1.f, 1.f};
            const float on = t < Tout ? 1.0f : 0.0f;
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float g = g4[c] * on;
                const float inv = 1.0f / sqrtf(va[c] + sg.eps);
                const float xh = (xv[c] - mu[c]) * inv;
                float d = w4[c] * inv * (g - s1[c] * invM - xh * s2[c] * invM);
                if (relu_in) d *= act_grad(xv[c], ST_ACT_RELU);
                o[c] = d;
            }
            *reinterpret_cast<f32x4*>(sg.dx + (size_t)m * sg.lddx + n) = o;
        }
        return;
    }
    const size_t total = (size_t)M * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
        const int b = m / T, t = m - b * T;
        const float g = dY[((size_t)b * Tout + min(t, Tout - 1)) * lddy + (size_t)k * N + n] * (t < Tout ? 1.0f : 0.0f);
        const float inv = 1.0f / sqrtf(sg.var[n] + sg.eps);
        const float xv = sg.x[(size_t)m * sg.ldx + n];
        const float xh = (xv - sg.mean[n]) * inv;
        float d = (sg.w ? sg.w[n] : 1.0f) * inv * (g - sg.sums[n] * invM - xh * sg.sums[N + n] * invM);
        if (relu_in) d *= act_grad(xv, ST_ACT_RELU);
        sg.dx[(size_t)m * sg.lddx + n] = d;
    }
}

// a bank ready to launch: the segments by value, and the grid of the row-split stages (sized for the longest segment)
struct BnBankPlan { BnBank a; int max_chunks; size_t max_rows; };

static void bnb_add_segment(BnBankPlan& p, const st_bn_bank_seg& sg) {
    const int M = p.a.Bn * sg.T;
    p.a.s[p.a.nseg++] = sg;
    p.max_chunks = max(p.max_chunks, st_colreduce_chunks(M));
    p.max_rows = max(p.max_rows, (size_t)M);
}

// one layer as a bank of one segment: the M rows of X's columns [coff, coff + N)
static BnBankPlan bn_one_segment(const float* X, int ldx, int coff, int M, int N, float* mean, float* var, float* run_mean, float* run_var,
                                 float momentum, long long* batches_tracked) {
    BnBankPlan p;
    p.a.nseg = 0; p.a.Bn = 1; p.a.N = N; p.max_chunks = 1; p.max_rows = 0;
    st_bn_bank_seg sg;
    memset(&sg, 0, sizeof(sg));
    sg.x = X + coff; sg.ldx = ldx; sg.T = M;
    sg.mean = mean; sg.var = var; sg.run_mean = run_mean; sg.run_var = run_var; sg.momentum = momentum; sg.batches_tracked = batches_tracked;
    bnb_add_segment(p, sg);
    return p;
}

// the two launches of the batch statistics: chunk-local (mean, M2), then their merge -- into every segment's mean / var with the running
// update, or rec != NULL: (mean, M2) and the row count behind them
static int bnb_stats_launch(const BnBankPlan& p, float* rec, float* ws, hipStream_t st) {
    const int N = p.a.N, nseg = p.a.nseg;
    hipLaunchKernelGGL(bnb_stats_chunk_kernel, dim3((N + 63) / 64, p.max_chunks, nseg), dim3(256), 0, st, p.a, ws, p.max_chunks);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(bnb_stats_final_kernel, dim3((N + 15) / 16, nseg), dim3(256), 0, st, p.a, ws, p.max_chunks, rec);
    ST_LAUNCH_CHECK();
    return 0;
}

static int bnb_merge_launch(const BnBankPlan& p, const float* allrec, int world, float* inv_total, hipStream_t st) {
    hipLaunchKernelGGL(bnb_sync_merge_kernel, dim3((p.a.N + 255) / 256, p.a.nseg), dim3(256), 0, st, p.a, allrec, world, inv_total);
    ST_LAUNCH_CHECK();
    return 0;
}

// what a stage asks of every segment beyond x / T / ldx
enum { SEG_STATS = 1, SEG_FRAMES = 2, SEG_SUMS = 4, SEG_DX = 8 };

// the checks every stage shares, once, and the segments it may then launch on
static int bnb_plan(BnBankPlan& p, const st_bn_bank_job& j, int need, const char* who) {
    ST_CHECK_ARG(j.segs && j.nseg >= 1 && j.nseg <= ST_BN_BANK_MAX && j.Bn > 0 && j.N > 0, "%s: bad arguments (1 to %d segments)", who, ST_BN_BANK_MAX);
    p.a.nseg = 0; p.a.Bn = j.Bn; p.a.N = j.N; p.max_chunks = 1; p.max_rows = 0;
    for (int k = 0; k < j.nseg; ++k) {
        const st_bn_bank_seg& sg = j.segs[k];
        ST_CHECK_ARG(sg.x && sg.T > 0 && sg.ldx >= j.N, "%s: segment %d incomplete (x, T, ldx)", who, k);
        ST_CHECK_ARG(!(need & SEG_STATS) || (sg.mean && sg.var), "%s: segment %d without mean / var", who, k);
        ST_CHECK_ARG(!(need & SEG_FRAMES) || sg.T >= j.Tout, "%s: segment %d has %d frames, the bank %d", who, k, sg.T, j.Tout);
        ST_CHECK_ARG(!(need & SEG_SUMS) || sg.sums, "%s: segment %d without sums", who, k);
        ST_CHECK_ARG(!(need & SEG_DX) || (sg.dx && sg.lddx >= j.N), "%s: segment %d without dx (lddx >= N)", who, k);
        bnb_add_segment(p, sg);
    }
    return 0;
}

}  // namespace

extern "C" int st_bn_stats(const float* X, int ldx, int coff, int M, int N, float* mean_out, float* var_out,
                           float* run_mean, float* run_var, float momentum, long long* batches_tracked, float* ws, void* stream) {
    (void)hipGetLastError();  // drop stale errors left by other HIP users of this thread
    ST_CHECK_ARG(X && mean_out && var_out && M > 0 && N > 0, "st_bn_stats: bad arguments");
    ST_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "st_bn_stats: run_mean/run_var must both be given");
    ST_CHECK_ARG(ws, "st_bn_stats: null workspace (st_colreduce_workspace_floats)");
    return bnb_stats_launch(bn_one_segment(X, ldx, coff, M, N, mean_out, var_out, run_mean, run_var, momentum, batches_tracked), nullptr, ws,
                            (hipStream_t)stream);
}

// SyncBN, local half: rec = (mean[N], M2[N], row count) of THIS rank's rows -- what the ranks exchange in one all-gather
extern "C" int st_bn_stats_record(const float* X, int ldx, int coff, int M, int N, float* rec, long long* batches_tracked, float* ws,
                                  void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(X && rec && ws && M > 0 && N > 0, "st_bn_stats_record: bad arguments");
    return bnb_stats_launch(bn_one_segment(X, ldx, coff, M, N, nullptr, nullptr, nullptr, nullptr, 0.0f, batches_tracked), rec, ws,
                            (hipStream_t)stream);
}

// SyncBN, merged half: the gathered records of all ranks (world, 2N + 1) = (world, 1 segment, 2N + 1) -> the statistics of the global batch;
// inv_total_out = 1 / (global row count)
extern "C" int st_bn_sync_merge(const float* rec, int world, int N, float* mean_out, float* var_out, float* run_mean, float* run_var,
                                float momentum, float* inv_total_out, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(rec && mean_out && var_out && inv_total_out && world > 0 && N > 0, "st_bn_sync_merge: bad arguments");
    ST_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "st_bn_sync_merge: run_mean/run_var must both be given");
    // (the merge reads no rows: its segment carries the outputs only)
    return bnb_merge_launch(bn_one_segment(nullptr, 0, 0, 1, N, mean_out, var_out, run_mean, run_var, momentum, nullptr), rec, world, inv_total_out,
                            (hipStream_t)stream);
}

extern "C" int st_bn_apply(float* X, int ldx, int coff, int M, int N, const float* mean, const float* var,
                           const float* w, const float* b, float eps, int act, void* stream) {
    (void)hipGetLastError();  // drop stale errors left by other HIP users of this thread
    ST_CHECK_ARG(X && mean && var && M > 0 && N > 0, "st_bn_apply: bad arguments");
    const size_t total = (size_t)M * N;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       X, ldx, coff, M, N, mean, var, w, b, eps, act);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_bn_norm_fwd(const float* X, int ldx, int xoff, float* Y, int ldy, int yoff, int M, int N,
                              const float* mean, const float* var, const float* w, const float* b, float eps, int act,
                              void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(X && Y && mean && var && M > 0 && N > 0, "st_bn_norm_fwd: bad arguments");
    hipLaunchKernelGGL(bn_norm_fwd_kernel, dim3(blocks_for((size_t)M * N)), dim3(256), 0, (hipStream_t)stream,
                       X, ldx, xoff, Y, ldy, yoff, M, N, mean, var, w, b, eps, act);
    ST_LAUNCH_CHECK();
    return 0;
}

// Tact (M, N) = act(BatchNorm(X)) (may be NULL when nobody needs it), Y (M, N) = (Tact + res) * mask; X, res, mask, Tact, Y contiguous rows
// of N floats, N % 4 == 0, 16-byte aligned.  ref: ConvLayer.forward, src/module.py:641-646
extern "C" int st_bn_norm_res_mask_fwd(const float* X, float* Tact, float* Y, int M, int N, const float* mean, const float* var,
                                       const float* w, const float* b, float eps, int act, const float* res, const float* mask,
                                       void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(X && Y && mean && var && M > 0 && N > 0 && N % 4 == 0, "st_bn_norm_res_mask_fwd: bad arguments (N %% 4 == 0)");
    ST_CHECK_ARG(st_aligned16(X) && st_aligned16(Y) && st_aligned16(Tact) && st_aligned16(res) && st_aligned16(mask) && st_aligned16(mean) && st_aligned16(var) && st_aligned16(w) && st_aligned16(b),
                 "st_bn_norm_res_mask_fwd: 16-byte aligned operands");
    const size_t total4 = (size_t)M * (N / 4);
    hipLaunchKernelGGL(bn_norm_res_mask_fwd_kernel, dim3(blocks_for(total4)), dim3(256), 0, (hipStream_t)stream,
                       X, Tact, Y, N / 4, total4, mean, var, w, b, eps, act, res, mask);
    ST_LAUNCH_CHECK();
    return 0;
}

// BatchNorm backward in two halves so that a data-parallel caller can all-reduce the two sums in between (SyncBN):
//   reduce: s[0:N] = sum_rows dyb, s[N:2N] = sum_rows dyb * xhat      (local rows)
//   apply:  dx = w/sigma * (dyb - s1/Mstat - xhat * s2/Mstat)          (Mstat = rows behind mean / var / s)
// Both read one st_bn_bwd_job.  Its mask / dres serve a layer whose forward was Y = (act(BN(x)) + res) * mask (st_bn_norm_res_mask_fwd;
// ConvLayer, src/module.py:641-646): the incoming gradient is multiplied by the mask on the way in (no launch of its own), `y` is the kept
// act(BN(x)), and the apply half also hands out dres = dy * mask, the gradient of the residual input (NULL: no residual).
static bool bn_bwd_job_ok(const st_bn_bwd_job& j) {
    return j.dy && j.x && j.mean && j.var && j.s && j.M > 0 && j.N > 0 && (j.act == ST_ACT_NONE || j.y);
}

extern "C" int st_bn_bwd_reduce(const st_bn_bwd_job* job, float* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(job, "st_bn_bwd_reduce: null job");
    const st_bn_bwd_job& j = *job;
    ST_CHECK_ARG(bn_bwd_job_ok(j) && ws, "st_bn_bwd_reduce: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    float* part = ws + 2 * (size_t)j.N;
    const int chunks = st_colreduce_chunks(j.M);
    const int rpc = (j.M + chunks - 1) / chunks;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((j.N + 63) / 64, chunks), dim3(256), 0, st, j.dy, j.ldd, 0, j.y, j.ldy, 0, j.act,
                       j.x, j.ldx, 0, j.mean, j.var, j.eps, j.M, j.N, rpc, part, j.mask, j.ldm);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(chunk_final_kernel, dim3((2 * j.N + 15) / 16), dim3(256), 0, st, part, chunks, 2, j.N, j.s, j.s + j.N, 0);
    ST_LAUNCH_CHECK();
    return 0;
}

// inv_total (device scalar, st_bn_sync_merge): s holds the sums over ALL ranks' rows and *inv_total = 1 / their count; the kernel then
// does not read Mstat
extern "C" int st_bn_bwd_apply(const st_bn_bwd_job* job, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(job, "st_bn_bwd_apply: null job");
    const st_bn_bwd_job& j = *job;
    ST_CHECK_ARG(bn_bwd_job_ok(j) && j.dx && (j.inv_total || j.Mstat >= j.M), "st_bn_bwd_apply: bad arguments");
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks_for((size_t)j.M * j.N)), dim3(256), 0, (hipStream_t)stream, j.dy, j.ldd, 0, j.y, j.ldy, 0,
                       j.act, j.x, j.ldx, 0, j.mean, j.var, j.w, j.eps, j.M, j.N, j.s, j.s + j.N, j.dx, j.lddx, 0, j.Mstat, j.inv_total,
                       j.mask, j.ldm, j.dres, j.lddr);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t st_bn_bank_workspace_floats(int nseg, int max_rows, int N) {
    return (size_t)nseg * st_colreduce_chunks(max_rows) * 2 * N;
}

// Forward stages of the bank (include/semitts.h): STATS | NORM with rec == NULL is the single-device forward; under SyncBN the caller runs
// STATS with rec -> [all-gather] -> MERGE -> NORM on the same job.
extern "C" int st_bn_bank_fwd(const st_bn_bank_job* job, int stages, void* stream) {
    (void)hipGetLastError();
    static const char* const who = "st_bn_bank_fwd";
    ST_CHECK_ARG(job, "%s: null job", who);
    const st_bn_bank_job& j = *job;
    const bool stats = stages & ST_BN_STATS, merge = stages & ST_BN_MERGE, norm = stages & ST_BN_NORM;
    ST_CHECK_ARG(stages == (j.rec ? ST_BN_STATS : ST_BN_STATS | ST_BN_NORM) || stages == ST_BN_MERGE || stages == ST_BN_NORM,
                 "%s: stages %d (STATS | NORM without rec, STATS with rec, MERGE or NORM)", who, stages);
    BnBankPlan p;
    const int need = (stats && j.rec ? 0 : SEG_STATS) | (norm ? SEG_FRAMES : 0);
    if (const int rc = bnb_plan(p, j, need, who)) return rc;
    ST_CHECK_ARG(!stats || j.ws, "%s: null workspace", who);
    ST_CHECK_ARG(!merge || (j.allrec && j.world > 0 && j.inv_total), "%s: MERGE without allrec, world > 0 or inv_total", who);
    ST_CHECK_ARG(!norm || (j.Y && j.Tout > 0 && j.ld >= j.nseg * j.N), "%s: bad output (Y, Tout, ld >= nseg N)", who);
    hipStream_t st = (hipStream_t)stream;
    if (stats) if (const int rc = bnb_stats_launch(p, j.rec, j.ws, st)) return rc;
    if (merge) return bnb_merge_launch(p, j.allrec, j.world, j.inv_total, st);
    if (norm) {
        int vec = j.N % 4 == 0 && j.ld % 4 == 0 && st_aligned16(j.Y);
        for (int k = 0; k < j.nseg && vec; ++k) {
            const st_bn_bank_seg& sg = j.segs[k];
            vec = sg.ldx % 4 == 0 && st_aligned16(sg.x) && st_aligned16(sg.mean) && st_aligned16(sg.var) && (!sg.w || st_aligned16(sg.w)) &&
                  (!sg.b || st_aligned16(sg.b));
        }
        hipLaunchKernelGGL(bnb_norm_kernel, dim3(blocks_for((size_t)j.Bn * j.Tout * j.N / (vec ? 4 : 1), 1024), j.nseg), dim3(256), 0, st, p.a, j.Y,
                           j.ld, j.Tout, vec);
        ST_LAUNCH_CHECK();
    }
    return 0;
}

// Backward stages: REDUCE | APPLY is the single-device backward; under SyncBN the caller runs REDUCE -> [all-reduce of the sums] -> APPLY
// with the segments' sums pointing at the global sums and inv_total from the forward's MERGE.
extern "C" int st_bn_bank_bwd(const st_bn_bank_job* job, int stages, void* stream) {
    (void)hipGetLastError();
    static const char* const who = "st_bn_bank_bwd";
    ST_CHECK_ARG(job, "%s: null job", who);
    const st_bn_bank_job& j = *job;
    const bool reduce = stages & ST_BN_REDUCE, apply = stages & ST_BN_APPLY;
    ST_CHECK_ARG(stages > 0 && !(stages & ~(ST_BN_REDUCE | ST_BN_APPLY)), "%s: stages %d (REDUCE, APPLY or both)", who, stages);
    BnBankPlan p;
    if (const int rc = bnb_plan(p, j, SEG_STATS | SEG_FRAMES | SEG_SUMS | (apply ? SEG_DX : 0), who)) return rc;
    ST_CHECK_ARG(j.dY && j.Tout > 0 && j.ld >= j.nseg * j.N && (!reduce || j.ws), "%s: bad gradient / workspace", who);
    hipStream_t st = (hipStream_t)stream;
    if (reduce) {        // sums of this rank's rows
        hipLaunchKernelGGL(bnb_bwd_reduce_kernel, dim3((j.N + 63) / 64, p.max_chunks, j.nseg), dim3(256), 0, st, p.a, j.dY, j.ld, j.Tout, j.ws,
                           p.max_chunks);
        ST_LAUNCH_CHECK();
        hipLaunchKernelGGL(bnb_bwd_final_kernel, dim3((2 * j.N + 15) / 16, j.nseg), dim3(256), 0, st, p.a, j.ws, p.max_chunks);
        ST_LAUNCH_CHECK();
    }
    if (apply) {
        int vec = j.N % 4 == 0 && j.ld % 4 == 0 && st_aligned16(j.dY);
        for (int k = 0; k < j.nseg && vec; ++k) {
            const st_bn_bank_seg& sg = j.segs[k];
            vec = sg.ldx % 4 == 0 && sg.lddx % 4 == 0 && st_aligned16(sg.x) && st_aligned16(sg.dx) && st_aligned16(sg.mean) && st_aligned16(sg.var) &&
                  st_aligned16(sg.sums) && (!sg.w || st_aligned16(sg.w));
        }
        hipLaunchKernelGGL(bnb_bwd_apply_kernel, dim3(blocks_for(p.max_rows * j.N / (vec ? 4 : 1), 1024), j.nseg), dim3(256), 0, st, p.a, j.dY, j.ld,
                           j.Tout, j.relu_in, vec, j.inv_total);
        ST_LAUNCH_CHECK();
    }
    return 0;
}
