// stoi.hip -- short-time objective intelligibility of a ragged batch of (clean, processed) waveform pairs at 10 kHz (st_stoi_batch):
// STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016).  Contract and definition: include/semitts.h.
//
// Launch 1 (stoi_energy_kernel, grid (runs of F_pad, B)).  A workgroup of 256 threads stages the span of SI_RUN = 16 consecutive frames
// of the clean signal (15 * 128 + 256 samples) in LDS once; a wave owns a frame: lane l forms ONE chain acc = fmaf(v, v, acc) over
// v = w[j] x[j], j = l, l + 64, l + 128, l + 192, the 64 partials combine by the xor butterfly and lane 0 stores sqrtf(acc).
// Launch 2 (stoi_select_kernel, one workgroup per pair).  Pass A: the maximum norm and a finiteness flag.  Pass B walks the frames
// in chunks of SI_CHUNK = 256: thread tid tests frame c + tid against the threshold, an inclusive block scan carried across the
// chunks numbers the kept frames in order and each thread writes its own index.  It also writes the four counts and the scores of
// the pairs that have no segment (the sentinel, or NaN after a non-finite clean energy).
// Launch 3 (stoi_bands_kernel, one wave per (output frame, side, pair)).  Output frame m of the re-synthesised signal is gathered
// from the kept frames m - 1, m, m + 1 by index (the signal itself never exists in memory), windowed twice, transformed by a
// 256-point complex Stockham FFT in LDS (radix 4, one butterfly a lane a stage) with the real split against the 512 table, and its
// 212 bins are summed into the 15 third-octave bands (4 lanes a band, fixed order).
// Launch 4 (stoi_corr_kernel, one wave per (pair, segment)).  The 15 x 30 tiles of both sides go to LDS as float64; lane j < 15 forms
// row j's clipped correlation (STOI) and normalises the rows in place, lane n < 30 then normalises column n and forms its
// correlation (ESTOI); the xor butterfly sums them.  Launch 5 (stoi_final_kernel, one wave per pair) sums the segments in a fixed
// order.  No atomics anywhere: a pair's outputs depend on its samples alone, not on B, F_pad or its position in the batch.
#include <float.h>
#include <math.h>
#include <mutex>
#include "st_common.h"

namespace {

constexpr int SI_FRAME = 256, SI_HOP = 128, SI_NFFT = 512, SI_M = SI_NFFT / 2;
constexpr int SI_BANDS = 15, SI_SEG = 30;
constexpr int SI_NT = 256, SI_NW = SI_NT / ST_WAVE;
constexpr int SI_RUN = 16;                                  // frames a workgroup of launch 1 takes from one staged span
constexpr int SI_SPAN = (SI_RUN - 1) * SI_HOP + SI_FRAME;   // 2176 samples
constexpr int SI_CHUNK = SI_NT;                             // frames per step of launch 2 (ops.STOI_CHUNK: the tests straddle it)
constexpr int SI_MAX_B = 64;
constexpr int SI_MAX_LEN = 1 << 22;                         // samples of the longest signal (ops.STOI_MAX_LEN): 7 minutes at 10 kHz
constexpr float SI_EPS = 0x1p-52f;
constexpr float SI_RATIO = 0.01f;                           // 10^(-DYN / 20), DYN = 40 dB
constexpr float SI_SENTINEL = 1e-5f;
constexpr double SI_EPS_D = 0x1p-52;
constexpr double SI_CLIP = 6.623413251903491;               // 1 + 10^(-BETA / 20), BETA = -15 dB

// band j sums the bins [SI_EDGE[j], SI_EDGE[j + 1]): the bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid k * 10000 / 512
__constant__ int SI_EDGE[SI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

struct StoiMeta {
    long off[SI_MAX_B];
    int len[SI_MAX_B];
};

__host__ __device__ inline int stoi_frames(int L) { return L > SI_FRAME ? (L - SI_FRAME + SI_HOP - 1) / SI_HOP : 0; }   // #{i : 128 i < L - 256}

// ------------------------------------------------------------------ tables: e^{-2 pi i k / 512} and the window, computed in double on the host
__device__ float2 g_si_tw[SI_NFFT];
__device__ float g_si_win[SI_FRAME];

std::mutex g_si_mu;
bool g_si_done[64];

// First use on a device uploads the two tables (a synchronous copy): that first call may not be inside a stream capture.
int ensure_tables(void* stream) {
    int dev = 0;
    ST_HIP(hipGetDevice(&dev));
    ST_CHECK_ARG(dev >= 0 && dev < 64, "st_stoi_batch: device index %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_si_mu);
    if (g_si_done[dev]) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    ST_HIP(hipStreamIsCapturing((hipStream_t)stream, &cs));
    ST_CHECK_ARG(cs == hipStreamCaptureStatusNone,
                 "st_stoi_batch: the first call on a device uploads its tables and may not be captured; call once before capturing");
    static float2 tw[SI_NFFT];
    static float win[SI_FRAME];
    for (int k = 0; k < SI_NFFT; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)SI_NFFT;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    for (int n = 0; n < SI_FRAME; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(n + 1) / (double)(SI_FRAME + 1)));
    ST_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_si_tw), tw, sizeof(tw)));
    ST_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_si_win), win, sizeof(win)));
    g_si_done[dev] = true;
    return 0;
}

// ------------------------------------------------------------------ launch 1: frame norms of the clean signal.  grid (runs of F_pad, B)
__global__ __launch_bounds__(SI_NT) void stoi_energy_kernel(const float* __restrict__ x, StoiMeta meta, float* __restrict__ energy, int F_pad) {
    __shared__ float xs[SI_SPAN];
    __shared__ float ws[SI_FRAME];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int L = meta.len[b];
    const int F = stoi_frames(L);
    const int t0 = blockIdx.x * SI_RUN;
    const int nt = min(SI_RUN, F_pad - t0);                        // frames of this run inside the output (>= 1 by the grid)
    const int nf = max(0, min(SI_RUN, F - t0));                    // frames of this run inside the signal
    float* eb = energy + (size_t)b * F_pad + t0;
    if (nf == 0) {                                                 // (uniform) a run past the signal: the padding rows
        for (int r = tid; r < nt; r += SI_NT) eb[r] = 0.0f;
        return;
    }
    const float* xb = x + meta.off[b];
    const long g0 = (long)t0 * SI_HOP;
    const int used = (nf - 1) * SI_HOP + SI_FRAME;                 // g0 + used <= 128 (F - 1) + 256 < L
    for (int j = tid; j < used; j += SI_NT) xs[j] = (g0 + j < L) ? xb[g0 + j] : 0.0f;
    ws[tid] = g_si_win[tid];
    __syncthreads();
    for (int r = wave; r < nf; r += SI_NW) {                       // (uniform in the wave)
        const float* xf = xs + r * SI_HOP;
        float acc = 0.0f;
#pragma unroll
        for (int j = lane; j < SI_FRAME; j += ST_WAVE) { const float v = __fmul_rn(ws[j], xf[j]); acc = fmaf(v, v, acc); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) eb[r] = sqrtf(acc);
    }
    for (int r = nf + tid; r < nt; r += SI_NT) eb[r] = 0.0f;
}

// ------------------------------------------------------------------ launch 2: the kept frames in order, the counts.  One workgroup per pair
__global__ __launch_bounds__(SI_NT) void stoi_select_kernel(const float* __restrict__ energy, StoiMeta meta, int F_pad, int32_t* __restrict__ kept,
                                                            int32_t* __restrict__ counts, float* __restrict__ score) {
    __shared__ float s_m[SI_NW];
    __shared__ int s_bad[SI_NW];
    __shared__ int s_w[SI_NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int F = stoi_frames(meta.len[b]);
    const float* e = energy + (size_t)b * F_pad;
    int32_t* kb = kept + (size_t)b * F_pad;
    // ---- pass A: the largest norm, and whether every norm is finite
    float m = 0.0f;
    int bad = 0;
    for (int t = tid; t < F; t += SI_NT) {
        const float v = e[t];
        bad |= !(fabsf(v) <= FLT_MAX);
        m = fmaxf(m, v);                                           // (a NaN leaves m as it is; bad is set)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) { s_m[wave] = m; s_bad[wave] = bad; }
    __syncthreads();
    m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    // kept iff 20 log10(e + EPS) > 20 log10(max + EPS) - 40, i.e. e + EPS > 10^-2 (max + EPS): one fp32 product, a strict comparison
    const float thr = SI_RATIO * (m + SI_EPS);
    // ---- pass B
    int carry = 0;                                                 // frames kept before this chunk
    if (!bad) {                                                    // (uniform)
        for (int c = 0; c < F; c += SI_CHUNK) {                    // (uniform trip count)
            const int t = c + tid;
            const bool keep = t < F && (e[t] + SI_EPS) > thr;
            int v = keep;
#pragma unroll
            for (int o = 1; o < ST_WAVE; o <<= 1) { const int up = __shfl_up(v, o, 64); if (lane >= o) v += up; }
            if (lane == ST_WAVE - 1) s_w[wave] = v;
            __syncthreads();
            int base = carry, total = 0;
#pragma unroll
            for (int w = 0; w < SI_NW; ++w) { if (w < wave) base += s_w[w]; total += s_w[w]; }
            if (keep) kb[base + v - 1] = t;                        // base + v - 1 < number kept <= F <= F_pad
            carry += total;
            __syncthreads();                                       // (the next chunk overwrites s_w)
        }
    }
    const int K = carry;
    for (int k = K + tid; k < F_pad; k += SI_NT) kb[k] = -1;
    if (tid == 0) {
        const int M = max(K - 1, 0), S = M >= SI_SEG ? M - SI_SEG + 1 : 0;
        counts[4 * b] = F; counts[4 * b + 1] = K; counts[4 * b + 2] = M; counts[4 * b + 3] = S;
        if (S == 0) {                                              // (launch 5 writes the pairs that have segments)
            const float v = bad ? __builtin_nanf("") : SI_SENTINEL;
            score[2 * b] = v; score[2 * b + 1] = v;
        }
    }
}

// ------------------------------------------------------------------ launch 3: third-octave bands.  One wave per (output frame, side, pair)
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmul_negi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)

// In-place forward 256-point complex FFT of buf (LDS) by one wave, natural order in and out: Stockham autosort, radix 4, lane l takes
// butterfly l of each of the four stages.  tw: the 512 table.  Ends with a barrier.
__device__ __forceinline__ void fft256_wave(float2* buf, const float2* __restrict__ tw, int lane) {
    constexpr int NB = SI_M / 4;                                   // 64 butterflies a stage
    int Ns = 1;
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = buf[lane + r * NB];
        __syncthreads();
        const int jm = lane & (Ns - 1);
        const int tstep = SI_NFFT / (Ns * 4);                      // index jm r tstep <= 3 (Ns - 1) 128 / Ns < 384
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < 4; ++r) v[r] = cmul(v[r], tw[jm * r * tstep]);
        }
        const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]);
        const float2 a2 = cadd(v[1], v[3]), a3 = cmul_negi(csub(v[1], v[3]));
        const int o = (lane - jm) * 4 + jm;                        // o + 3 Ns <= 255
        buf[o] = cadd(a0, a2);
        buf[o + Ns] = cadd(a1, a3);
        buf[o + 2 * Ns] = csub(a0, a2);
        buf[o + 3 * Ns] = csub(a1, a3);
        __syncthreads();
        Ns *= 4;
    }
}

// grid (F_pad, 2, B), 64 threads.  side 0 reads x, side 1 reads y (the same offsets and lengths).
__global__ __launch_bounds__(ST_WAVE) void stoi_bands_kernel(const float* __restrict__ x, const float* __restrict__ y, StoiMeta meta, int F_pad,
                                                             const int32_t* __restrict__ kept, const int32_t* __restrict__ counts,
                                                             float* __restrict__ bands) {
    __shared__ float2 buf[SI_M];
    __shared__ float pw[SI_M + 1];
    const int m = blockIdx.x, side = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    float* out = bands + ((size_t)(b * 2 + side) * SI_BANDS) * F_pad + m;
    const int M = counts[4 * b + 2];
    if (m >= M) {                                                  // (uniform) the padding columns
        if (lane < SI_BANDS) out[(size_t)lane * F_pad] = 0.0f;
        return;
    }
    const int F = stoi_frames(meta.len[b]);
    const float* s = (side ? y : x) + meta.off[b];
    const int32_t* kb = kept + (size_t)b * F_pad;
    // m < M = K - 1: kept[m] and kept[m + 1] exist; a kept index is a frame of the signal, so 128 k + 255 < L
    const int kp = m > 0 ? kb[m - 1] : -1, kc = kb[m], kn = kb[m + 1];
    const bool okp = kp >= 0 && kp < F, okc = kc >= 0 && kc < F, okn = kn >= 0 && kn < F;
    const float* sp = s + (size_t)max(kp, 0) * SI_HOP;
    const float* sc = s + (size_t)max(kc, 0) * SI_HOP;
    const float* sn = s + (size_t)max(kn, 0) * SI_HOP;
    // sample n of the output frame = (overlap-add of the windowed kept frames at 128 m + n) * w[n]; z[q] = v[2 q] + i v[2 q + 1]
#pragma unroll
    for (int q = lane; q < SI_FRAME / 2; q += ST_WAVE) {
        float v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int n = 2 * q + u;
            float r;
            if (n < SI_HOP) {
                const float a = okp ? __fmul_rn(g_si_win[n + SI_HOP], sp[n + SI_HOP]) : 0.0f;
                const float c = okc ? __fmul_rn(g_si_win[n], sc[n]) : 0.0f;
                r = __fadd_rn(a, c);
            } else {
                const float c = okc ? __fmul_rn(g_si_win[n], sc[n]) : 0.0f;
                const float d = okn ? __fmul_rn(g_si_win[n - SI_HOP], sn[n - SI_HOP]) : 0.0f;
                r = __fadd_rn(c, d);
            }
            v[u] = __fmul_rn(g_si_win[n], r);
        }
        buf[q] = make_float2(v[0], v[1]);
        buf[q + SI_FRAME / 2] = make_float2(0.0f, 0.0f);           // the zero padding to 512
    }
    __syncthreads();
    fft256_wave(buf, g_si_tw, lane);
    // real split: X[k], X[256 - k] of the 512-point real transform from Z[k], Z[256 - k] (k = 0 gives X[0] and X[256])
    for (int k = lane; k <= SI_M / 2; k += ST_WAVE) {
        const float2 zk = buf[k], zc = buf[(SI_M - k) & (SI_M - 1)], w = g_si_tw[k];
        const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
        const float2 o = make_float2(0.5f * (zk.y + zc.y), -0.5f * (zk.x - zc.x));
        const float2 wo = cmul(w, o);
        const float2 xk = cadd(e, wo), xc = csub(e, wo);           // (|conj| = |.|)
        pw[k] = xk.x * xk.x + xk.y * xk.y;
        pw[SI_M - k] = xc.x * xc.x + xc.y * xc.y;
    }
    __syncthreads();
    // band j: lanes 4 j + q, q < 4, each one chain over the bins lo + q, lo + q + 4, ... in ascending order, then (q0 + q1) + (q2 + q3)
    const int j = min(lane >> 2, SI_BANDS - 1), q = lane & 3;
    float acc = 0.0f;
    for (int k = SI_EDGE[j] + q; k < SI_EDGE[j + 1]; k += 4) acc += pw[k];
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (q == 0 && lane < 4 * SI_BANDS) out[(size_t)j * F_pad] = sqrtf(acc);
}

// ------------------------------------------------------------------ launch 4: both correlations of a segment.  One wave per (pair, segment)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (ceil(S_pad / 4), B), 256 threads; part (B, S_pad, 2) float64
__global__ __launch_bounds__(SI_NT) void stoi_corr_kernel(const float* __restrict__ bands, const int32_t* __restrict__ counts, int F_pad, int S_pad,
                                                          double* __restrict__ part) {
    __shared__ double tile[SI_NW][2][SI_BANDS][SI_SEG];            // 28800 bytes
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int s = blockIdx.x * SI_NW + wave;
    const int S = counts[4 * b + 3];
    const bool live = s < S;                                       // (uniform in the wave; every wave reaches the barriers)
    double (*X)[SI_SEG] = tile[wave][0];
    double (*Y)[SI_SEG] = tile[wave][1];
    if (live) {
        const float* xb = bands + (size_t)(b * 2) * SI_BANDS * F_pad + s;      // columns s .. s + 29 <= M - 1 < F_pad
        const float* yb = xb + (size_t)SI_BANDS * F_pad;
        for (int i = lane; i < SI_BANDS * SI_SEG; i += ST_WAVE) {
            const int j = i / SI_SEG, n = i - j * SI_SEG;
            X[j][n] = (double)xb[(size_t)j * F_pad + n];
            Y[j][n] = (double)yb[(size_t)j * F_pad + n];
        }
    }
    __syncthreads();
    double d = 0.0, de = 0.0;
    if (live && lane < SI_BANDS) {
        double* xr = X[lane];
        double* yr = Y[lane];
        double sxx = 0.0, syy = 0.0;
        for (int n = 0; n < SI_SEG; ++n) { sxx += xr[n] * xr[n]; syy += yr[n] * yr[n]; }
        const double c = sqrt(sxx) / (sqrt(syy) + SI_EPS_D);
        // ---- STOI: y' = min(c y, CLIP x) (a NaN in c y stays: the comparison is false), both rows centred and scaled
        double mx = 0.0, my = 0.0;
        for (int n = 0; n < SI_SEG; ++n) {
            const double cy = c * yr[n], bx = SI_CLIP * xr[n];
            mx += xr[n];
            my += (cy > bx) ? bx : cy;
        }
        mx /= SI_SEG; my /= SI_SEG;
        double nx = 0.0, ny = 0.0, dot = 0.0;
        for (int n = 0; n < SI_SEG; ++n) {
            const double cy = c * yr[n], bx = SI_CLIP * xr[n];
            const double u = xr[n] - mx, v = ((cy > bx) ? bx : cy) - my;
            nx += u * u; ny += v * v; dot += u * v;
        }
        d = dot / ((sqrt(nx) + SI_EPS_D) * (sqrt(ny) + SI_EPS_D));
        // ---- ESTOI, rows: centred and scaled in place (x's mean is mx)
        double mr = 0.0;
        for (int n = 0; n < SI_SEG; ++n) mr += yr[n];
        mr /= SI_SEG;
        double ry = 0.0;
        for (int n = 0; n < SI_SEG; ++n) { const double v = yr[n] - mr; ry += v * v; }
        const double ix = sqrt(nx) + SI_EPS_D, iy = sqrt(ry) + SI_EPS_D;
        for (int n = 0; n < SI_SEG; ++n) { xr[n] = (xr[n] - mx) / ix; yr[n] = (yr[n] - mr) / iy; }
    }
    __syncthreads();
    if (live && lane < SI_SEG) {                                   // ---- ESTOI, columns
        double mx = 0.0, my = 0.0;
        for (int j = 0; j < SI_BANDS; ++j) { mx += X[j][lane]; my += Y[j][lane]; }
        mx /= SI_BANDS; my /= SI_BANDS;
        double nx = 0.0, ny = 0.0, dot = 0.0;
        for (int j = 0; j < SI_BANDS; ++j) {
            const double u = X[j][lane] - mx, v = Y[j][lane] - my;
            nx += u * u; ny += v * v; dot += u * v;
        }
        de = dot / ((sqrt(nx) + SI_EPS_D) * (sqrt(ny) + SI_EPS_D));
    }
    if (live) {
        d = wave_sum_d(d);
        de = wave_sum_d(de);
        if (lane == 0) {
            double* p = part + ((size_t)b * S_pad + s) * 2;
            p[0] = d; p[1] = de;
        }
    }
}

// ------------------------------------------------------------------ launch 5: the segments of a pair in a fixed order.  One wave per pair
__global__ __launch_bounds__(ST_WAVE) void stoi_final_kernel(const double* __restrict__ part, const int32_t* __restrict__ counts, int S_pad,
                                                             float* __restrict__ score) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int S = counts[4 * b + 3];
    if (S == 0) return;                                            // (uniform) launch 2 wrote this pair's scores
    const double* p = part + (size_t)b * S_pad * 2;
    double d = 0.0, de = 0.0;
    for (int s = lane; s < S; s += ST_WAVE) { d += p[2 * s]; de += p[2 * s + 1]; }
    d = wave_sum_d(d);
    de = wave_sum_d(de);
    if (lane == 0) {
        score[2 * b] = (float)(d / ((double)SI_BANDS * S));
        score[2 * b + 1] = (float)(de / ((double)SI_SEG * S));
    }
}

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }

}  // namespace

extern "C" int st_stoi_frames(int len) { return len >= 1 && len <= SI_MAX_LEN ? stoi_frames(len) : -1; }

extern "C" size_t st_stoi_workspace_floats(int B, int F_pad) {
    if (B < 1 || F_pad < 1) return 0;
    // segment partials (B, F_pad, 2) float64 first, then energies (B, F_pad), kept (B, F_pad) and bands (B, 2, 15, F_pad)
    return round64((size_t)B * F_pad * 4) + 2 * round64((size_t)B * F_pad) + round64((size_t)B * F_pad * 2 * SI_BANDS);
}

extern "C" int st_stoi_batch(const st_wave_batch* x, const float* y, float* score, int32_t* counts, int F_pad, float* energy, int32_t* kept,
                             float* bands, float* ws, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(x, "st_stoi_batch: null pointer");
    ST_CHECK_ARG(x->B >= 0 && x->B <= SI_MAX_B, "st_stoi_batch: batch %d outside [0, %d]", x->B, SI_MAX_B);
    if (x->B == 0) return 0;
    ST_CHECK_ARG(x->x && x->off && x->len && y && score && counts && ws, "st_stoi_batch: null pointer");
    ST_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "st_stoi_batch: the workspace must be 8-byte aligned");
    StoiMeta meta;
    memset(&meta, 0, sizeof(meta));
    int fmax = 0;
    for (int b = 0; b < x->B; ++b) {
        ST_CHECK_ARG(x->len[b] >= 1 && x->off[b] >= 0 && x->off[b] + x->len[b] <= x->n_samples,
                     "st_stoi_batch: signal %d [%ld, +%d) outside the %ld samples", b, x->off[b], x->len[b], x->n_samples);
        ST_CHECK_ARG(x->len[b] <= SI_MAX_LEN, "st_stoi_batch: signal %d has %d samples, above the limit of %d", b, x->len[b], SI_MAX_LEN);
        meta.off[b] = x->off[b];
        meta.len[b] = x->len[b];
        fmax = max(fmax, stoi_frames(x->len[b]));
    }
    ST_CHECK_ARG(F_pad >= 1 && F_pad >= fmax, "st_stoi_batch: F_pad %d below the %d frames of the longest signal (at least 1)", F_pad, fmax);
    int rc;
    if ((rc = ensure_tables(stream)) != 0) return rc;
    const int B = x->B;
    const size_t bf = (size_t)B * F_pad;
    double* part = reinterpret_cast<double*>(ws);
    float* p = ws + round64(bf * 4);
    float* e_ws = p; p += round64(bf);
    int32_t* k_ws = reinterpret_cast<int32_t*>(p); p += round64(bf);
    float* b_ws = p;
    if (!energy) energy = e_ws;
    if (!kept) kept = k_ws;
    if (!bands) bands = b_ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((F_pad + SI_RUN - 1) / SI_RUN), B), dim3(SI_NT), 0, st, x->x, meta, energy, F_pad);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_select_kernel, dim3(B), dim3(SI_NT), 0, st, energy, meta, F_pad, kept, counts, score);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_bands_kernel, dim3(F_pad, 2, B), dim3(ST_WAVE), 0, st, x->x, y, meta, F_pad, kept, counts, bands);
    ST_LAUNCH_CHECK();
    const int S_pad = F_pad - SI_SEG;                              // S <= M - 29 <= F_pad - 30
    if (S_pad >= 1) {
        hipLaunchKernelGGL(stoi_corr_kernel, dim3((unsigned)((S_pad + SI_NW - 1) / SI_NW), B), dim3(SI_NT), 0, st, bands, counts, F_pad, S_pad, part);
        ST_LAUNCH_CHECK();
        hipLaunchKernelGGL(stoi_final_kernel, dim3(B), dim3(ST_WAVE), 0, st, part, counts, S_pad, score);
        ST_LAUNCH_CHECK();
    }
    return 0;
}
