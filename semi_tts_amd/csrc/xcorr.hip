// xcorr.hip -- integer-delay search (st_xcorr_delay), SI-SDR / SNR on the overlap a delay leaves (st_sisdr_batch) and the span copy that
// gives two cut batches one layout (st_wave_gather), for ragged batches of (reference, processed) waveform pairs.
// Contract and definitions: include/semitts.h.
//
// st_xcorr_delay, launch 1 (xcorr_partial_kernel, grid (lag tile, sample chunk, pair), 256 threads).  A workgroup owns XC_T = 2048
// consecutive lags and one chunk of the pair's x.  The chunk is walked in pieces of XC_C = 1024 samples: a piece of x and the span
// XC_C + XC_T of y it meets are staged in LDS once, ALREADY AS float64 and zero outside the signals, so the inner loop holds no
// conversion and no bound.  Thread t owns the XC_R = 8 consecutive lags t 8 .. t 8 + 7 and takes XC_S = 8 samples a step: the 64 FMAs
// of a step need 15 reads of y and 8 broadcast reads of x.  y lies in LDS de-interleaved by 8 (element k at row k % 8, column k / 8),
// so the 64 lanes of every read touch 64 consecutive doubles (no bank conflict) and all 15 addresses are one base register plus a
// compile-time offset.  Each lag is ONE chain acc = fma(x, y, acc) over ascending n through the whole chunk; a zero of the padding
// leaves a chain as it is, so the padding is invisible for finite input.  A piece that holds a non-finite sample takes a guarded
// loop over the same terms in the same order instead (0 * inf would otherwise reach lags whose range excludes that sample).
// Launch 2 (xcorr_finish_kernel, one workgroup per pair) adds a lag's chunks in ascending order, writes corr, picks the largest by
// the total order (value, then smaller |d|, then d >= 0), forms sum x^2 and sum y^2 and writes delay and coef.
// How a pair is cut depends on its own Lx and D alone (xcorr_chunk_len); no atomics: every output of a pair is bitwise what the pair
// gives alone.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "st_common.h"

namespace {

constexpr int XC_NT = 256, XC_NW = XC_NT / ST_WAVE;
constexpr int XC_FT = 1024, XC_FW = XC_FT / ST_WAVE;          // threads and waves of the finish launch
constexpr int XC_R = 8, XC_S = 8;                           // register tile: lags x samples
constexpr int XC_T = XC_NT * XC_R;                          // 2048 lags a workgroup (ops.XCORR_LAG_TILE)
constexpr int XC_C = 1024;                                  // samples a staged piece, the smallest chunk (ops.XCORR_CHUNK)
constexpr int XC_MAX_CHUNKS = 32;                           // chunks of the longest pair (ops.XCORR_MAX_CHUNKS): the chunk grows with Lx
constexpr int XC_YCOLS = (XC_C + XC_T) / XC_R;              // 384 columns of the de-interleaved y span
constexpr int XC_YROW = XC_YCOLS + 4;                       // row stride: 388 = 4 mod 32, the 32 lanes of a staging write fall on 32 banks
constexpr int XC_MAX_B = 64;
constexpr int XC_MAX_LEN = 1 << 22;
constexpr int XC_MAX_LAG = 16384;
constexpr int SD_CHUNK = 8192;                              // samples a workgroup of st_sisdr_batch's first launch (ops.SISDR_CHUNK)

static_assert(XC_R == 8 && XC_S == 8 && XC_C % XC_S == 0 && (XC_C + XC_T) % XC_R == 0, "the tile arithmetic below assumes 8 x 8");

struct XcMeta {
    long offx[XC_MAX_B], offy[XC_MAX_B];
    int lx[XC_MAX_B], ly[XC_MAX_B];
};

struct GatherMeta {
    long so[XC_MAX_B], dof[XC_MAX_B];
    int len[XC_MAX_B];
};

// chunk of a pair's x: XC_C times the smallest factor that leaves at most XC_MAX_CHUNKS chunks
__host__ __device__ inline int xcorr_chunk_len(int Lx) { return XC_C * ((Lx + XC_C * XC_MAX_CHUNKS - 1) / (XC_C * XC_MAX_CHUNKS)); }
__host__ __device__ inline int xcorr_chunks(int Lx) { const int cl = xcorr_chunk_len(Lx); return (Lx + cl - 1) / cl; }
// the chunk count is not monotone in Lx (32768 samples are 32 chunks, 32769 are 17): the most any signal of at most max_len samples has
inline int xcorr_chunk_rows(int max_len) { return min(XC_MAX_CHUNKS, (max_len + XC_C - 1) / XC_C); }

__device__ __forceinline__ bool xc_finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ st_xcorr_delay, launch 1.  grid (lag tiles, chunks of the longest x, B)
// part (B, nch_stride, nlags) float64
__global__ __launch_bounds__(XC_NT) void xcorr_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, XcMeta meta, int D,
                                                              int nch_stride, double* __restrict__ part) {
    __shared__ double xs[XC_C];
    __shared__ double ys[XC_R * XC_YROW];
    const int b = blockIdx.z, chunk = blockIdx.y, tid = threadIdx.x, wave = tid / ST_WAVE;
    const int Lx = meta.lx[b], Ly = meta.ly[b];
    const int cl = xcorr_chunk_len(Lx);
    if (chunk >= (Lx + cl - 1) / cl) return;                       // (uniform) launch 2 reads this pair's own chunks only
    const int nlags = 2 * D + 1;
    const int jt = blockIdx.x * XC_T;                              // first lag index of the tile (lag d = j - D)
    const int j0 = jt + tid * XC_R;                                // this thread's first lag index
    const bool wave_live = jt + wave * (ST_WAVE * XC_R) < nlags;   // (uniform in the wave) some lag of the wave exists
    const float* xb = x + meta.offx[b];
    const float* yb = y + meta.offy[b];
    const int c_lo = chunk * cl, c_hi = min(Lx, c_lo + cl);
    double acc[XC_R];
#pragma unroll
    for (int r = 0; r < XC_R; ++r) acc[r] = 0.0;
    for (int n0 = c_lo; n0 < c_hi; n0 += XC_C) {                   // (uniform) the pieces of the chunk in ascending order
        const int cn = min(XC_C, c_hi - n0);                       // samples of x in this piece
        const long y0 = (long)n0 + jt - D;                         // y index of ys element 0
        int bad = 0;
        for (int i = tid; i < XC_C; i += XC_NT) {
            const float v = i < cn ? xb[n0 + i] : 0.0f;
            bad |= !xc_finite(v);
            xs[i] = (double)v;
        }
        for (int k = tid; k < XC_C + XC_T; k += XC_NT) {
            const long yi = y0 + k;
            const float v = (yi >= 0 && yi < Ly) ? yb[yi] : 0.0f;
            bad |= !xc_finite(v);
            ys[(k & (XC_R - 1)) * XC_YROW + (k >> 3)] = (double)v;
        }
        bad = __syncthreads_or(bad);
        if (wave_live) {
            if (!bad) {                                            // (uniform)
                const int steps = (cn + XC_S - 1) / XC_S;          // (the samples past cn are staged zeros)
                const double* yt = ys + tid;
                for (int q = 0; q < steps; ++q) {
                    double yv[XC_R + XC_S - 1], xv[XC_S];
                    // element k = 8 q + 8 tid + c lies at row c % 8, column q + tid + c / 8 <= 127 + 255 + 1 < XC_YCOLS
#pragma unroll
                    for (int c = 0; c < XC_R + XC_S - 1; ++c) yv[c] = yt[(c & (XC_R - 1)) * XC_YROW + q + (c >> 3)];
#pragma unroll
                    for (int s = 0; s < XC_S; ++s) xv[s] = xs[q * XC_S + s];
#pragma unroll
                    for (int s = 0; s < XC_S; ++s) {
#pragma unroll
                        for (int r = 0; r < XC_R; ++r) acc[r] = fma(xv[s], yv[s + r], acc[r]);
                    }
                }
            } else {                                               // the same terms in the same order, the padding left out
#pragma unroll
                for (int r = 0; r < XC_R; ++r) {                   // (unrolled: acc stays in registers)
                    const long yoff = y0 + tid * XC_R + r;         // y index of sample i of the piece at this lag: yoff + i
                    double a = acc[r];
                    for (int i = 0; i < cn; ++i) {
                        const long yi = yoff + i;
                        const int k = i + tid * XC_R + r;          // < XC_C + XC_T
                        if (yi >= 0 && yi < Ly) a = fma(xs[i], ys[(k & (XC_R - 1)) * XC_YROW + (k >> 3)], a);
                    }
                    acc[r] = a;
                }
            }
        }
        __syncthreads();                                           // (the next piece overwrites xs and ys)
    }
    double* p = part + ((size_t)b * nch_stride + chunk) * nlags;
#pragma unroll
    for (int r = 0; r < XC_R; ++r)
        if (j0 + r < nlags) p[j0 + r] = acc[r];
}

// is candidate (v, d) ahead of (bv, bd)?  larger value, then smaller |d|, then the non-negative lag: a total order on distinct lags
__device__ __forceinline__ bool xc_ahead(double v, int d, double bv, int bd) {
    if (v != bv) return v > bv;
    const int a = abs(d), ba = abs(bd);
    if (a != ba) return a < ba;
    return d > bd;
}

// ------------------------------------------------------------------ st_xcorr_delay, launch 2.  One workgroup of 1024 threads per pair
// (few workgroups, each a chain of dependent reads: the width and the unrolled loads are what hide their latency)
__global__ __launch_bounds__(XC_FT) void xcorr_finish_kernel(const float* __restrict__ x, const float* __restrict__ y, XcMeta meta, int D,
                                                             int nch_stride, const double* __restrict__ part, double* __restrict__ corr,
                                                             int32_t* __restrict__ delay, float* __restrict__ coef) {
    __shared__ double s_v[XC_FW], s_xx[XC_FW], s_yy[XC_FW];
    __shared__ int s_d[XC_FW], s_nan[XC_FW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int Lx = meta.lx[b], Ly = meta.ly[b];
    const int nlags = 2 * D + 1, nch = xcorr_chunks(Lx);
    const double* p = part + (size_t)b * nch_stride * nlags;
    double bv = -INFINITY;
    int bd = INT_MAX, nan = 0;                                     // (no lag yet: any lag is ahead of it)
    for (int j = tid; j < nlags; j += XC_FT) {
        double r = 0.0;
#pragma unroll 8
        for (int c = 0; c < nch; ++c) r += p[(size_t)c * nlags + j];       // ascending chunks (the loads of 8 go out together)
        if (corr) corr[(size_t)b * nlags + j] = r;
        nan |= (r != r);
        const int d = j - D;
        if (bd == INT_MAX || xc_ahead(r, d, bv, bd)) { bv = r; bd = d; }
    }
    const float* xb = x + meta.offx[b];
    const float* yb = y + meta.offy[b];
    double sxx = 0.0, syy = 0.0;
#pragma unroll 8
    for (int i = tid; i < Lx; i += XC_FT) { const double v = (double)xb[i]; sxx = fma(v, v, sxx); }
#pragma unroll 8
    for (int i = tid; i < Ly; i += XC_FT) { const double v = (double)yb[i]; syy = fma(v, v, syy); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int od = __shfl_xor(bd, o, 64);
        nan |= __shfl_xor(nan, o, 64);
        if (od != INT_MAX && (bd == INT_MAX || xc_ahead(ov, od, bv, bd))) { bv = ov; bd = od; }
    }
    sxx = wave_sum_d(sxx);
    syy = wave_sum_d(syy);
    if (lane == 0) { s_v[wave] = bv; s_d[wave] = bd; s_nan[wave] = nan; s_xx[wave] = sxx; s_yy[wave] = syy; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < XC_FW; ++w) {                          // the waves in ascending order
            nan |= s_nan[w];
            if (s_d[w] != INT_MAX && (bd == INT_MAX || xc_ahead(s_v[w], s_d[w], bv, bd))) { bv = s_v[w]; bd = s_d[w]; }
            sxx += s_xx[w];
            syy += s_yy[w];
        }
        if (nan) {
            delay[b] = 0;
            coef[b] = __builtin_nanf("");
        } else {
            delay[b] = bd;
            coef[b] = (float)(bv / sqrt(__dmul_rn(sxx, syy)));
        }
    }
}

// ------------------------------------------------------------------ st_sisdr_batch
// the overlap a delay leaves: x from x0, y from y0, n samples (n <= 0: none)
__device__ __forceinline__ void sd_span(int Lx, int Ly, int d, long& x0, long& y0, long& n) {
    x0 = d >= 0 ? 0 : -(long)d;
    y0 = d >= 0 ? (long)d : 0;
    n = min((long)Lx - x0, (long)Ly - y0);
}

// launch 1: grid (chunks of the longest side, B).  part (B, nch_stride, 5) float64 = (sum x, sum y, sum x^2, sum y^2, sum x y) of a chunk
__global__ __launch_bounds__(XC_NT) void sisdr_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, XcMeta meta,
                                                              const int32_t* __restrict__ delay, int nch_stride, double* __restrict__ part) {
    static_assert(XC_NW == 4, "the four wave sums below are combined as (0 + 1) + (2 + 3)");
    __shared__ double s_p[XC_NW][5];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    long x0, y0, n;
    sd_span(meta.lx[b], meta.ly[b], delay ? delay[b] : 0, x0, y0, n);
    const long lo = (long)chunk * SD_CHUNK;
    if (lo >= n) return;                                           // (uniform; covers n <= 0) launch 2 reads the chunks below n only
    const long hi = min(n, lo + SD_CHUNK);
    const float* xb = x + meta.offx[b] + x0;                       // x0 + i < Lx and y0 + i < Ly for i < n
    const float* yb = y + meta.offy[b] + y0;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (long i = lo + tid; i < hi; i += XC_NT) {
        const double u = (double)xb[i], v = (double)yb[i];
        sx += u; sy += v;
        sxx = fma(u, u, sxx); syy = fma(v, v, syy); sxy = fma(u, v, sxy);
    }
    sx = wave_sum_d(sx); sy = wave_sum_d(sy); sxx = wave_sum_d(sxx); syy = wave_sum_d(syy); sxy = wave_sum_d(sxy);
    if (lane == 0) { s_p[wave][0] = sx; s_p[wave][1] = sy; s_p[wave][2] = sxx; s_p[wave][3] = syy; s_p[wave][4] = sxy; }
    __syncthreads();
    if (tid < 5) part[((size_t)b * nch_stride + chunk) * 5 + tid] = (s_p[0][tid] + s_p[1][tid]) + (s_p[2][tid] + s_p[3][tid]);
}

// the three figures from the five sums, every operation rounded on its own: with a product contracted into an fma, Cxx Cyy - Cxy Cxy of a
// scaled copy would not be the exact 0 that makes its SI-SDR +inf (hipcc contracts by default, also across the __dmul_rn family)
struct SdScores { double si, sn, g; };
__device__ __forceinline__ SdScores sd_scores(double nd, double sx, double sy, double sxx, double syy, double sxy, int zero_mean) {
#pragma clang fp contract(off)
    double cxx = sxx, cyy = syy, cxy = sxy;
    if (zero_mean) {
        const double mxx = sx * sx, myy = sy * sy, mxy = sx * sy;
        cxx = cxx - mxx / nd;
        cyy = cyy - myy / nd;
        cxy = cxy - mxy / nd;
    }
    const double t = cxy * cxy;
    const double p = cxx * cyy;
    const double two = 2.0 * cxy;
    SdScores r;
    r.si = 10.0 * log10(t / (p - t));
    r.sn = 10.0 * log10(cxx / ((cxx - two) + cyy));
    r.g = 20.0 * log10(fabs(cxy / cxx));
    return r;
}

// launch 2: one wave per pair
__global__ __launch_bounds__(ST_WAVE) void sisdr_finish_kernel(XcMeta meta, const int32_t* __restrict__ delay, int zero_mean, int nch_stride,
                                                               const double* __restrict__ part, double* __restrict__ sums,
                                                               float* __restrict__ score) {
    const int b = blockIdx.x, lane = threadIdx.x;
    long x0, y0, n;
    sd_span(meta.lx[b], meta.ly[b], delay ? delay[b] : 0, x0, y0, n);
    double* so = sums + 6 * b;
    float* sc = score + 3 * b;
    if (n <= 0) {                                                  // (uniform) the delay is longer than a side
        if (lane < 6) so[lane] = 0.0;
        if (lane < 3) sc[lane] = __builtin_nanf("");
        return;
    }
    const int nch = (int)((n + SD_CHUNK - 1) / SD_CHUNK);
    const double* p = part + (size_t)b * nch_stride * 5;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = lane; c < nch; c += ST_WAVE) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += p[(size_t)c * 5 + k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = wave_sum_d(s[k]);
    if (lane == 0) {
        const double nd = (double)n;
        so[0] = nd;
#pragma unroll
        for (int k = 0; k < 5; ++k) so[1 + k] = s[k];
        const SdScores r = sd_scores(nd, s[0], s[1], s[2], s[3], s[4], zero_mean);
        const double si = r.si, sn = r.sn, g = r.g;
        sc[0] = (float)si; sc[1] = (float)sn; sc[2] = (float)g;
    }
}

// ------------------------------------------------------------------ st_wave_gather.  grid (blocks, B)
__global__ __launch_bounds__(XC_NT) void wave_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, GatherMeta meta) {
    const int b = blockIdx.y;
    const int L = meta.len[b];
    const float* s = src + meta.so[b];
    float* d = dst + meta.dof[b];
    for (int i = blockIdx.x * XC_NT + threadIdx.x; i < L; i += gridDim.x * XC_NT) d[i] = s[i];
}

inline size_t round64(size_t n) { return (n + 63) & ~(size_t)63; }

// the checks both entry points share; fills meta and the longest lengths
int pair_meta(const char* what, const st_wave_batch* x, const st_wave_batch* y, XcMeta& meta, int& max_lx, int& max_l) {
    ST_CHECK_ARG(x && y, "%s: null pointer", what);
    ST_CHECK_ARG(x->B >= 0 && x->B <= XC_MAX_B, "%s: batch %d outside [0, %d]", what, x->B, XC_MAX_B);
    ST_CHECK_ARG(y->B == x->B, "%s: %d references and %d processed signals", what, x->B, y->B);
    memset(&meta, 0, sizeof(meta));
    max_lx = max_l = 0;
    if (x->B == 0) return 0;
    ST_CHECK_ARG(x->x && x->off && x->len && y->x && y->off && y->len, "%s: null pointer", what);
    for (int b = 0; b < x->B; ++b) {
        const st_wave_batch* side[2] = {x, y};
        for (int s = 0; s < 2; ++s) {
            const st_wave_batch* w = side[s];
            ST_CHECK_ARG(w->len[b] >= 1 && w->len[b] <= XC_MAX_LEN, "%s: %s signal %d has %d samples, outside [1, %d]", what, s ? "processed" : "reference",
                         b, w->len[b], XC_MAX_LEN);
            ST_CHECK_ARG(w->off[b] >= 0 && w->off[b] + w->len[b] <= w->n_samples, "%s: %s signal %d [%ld, +%d) outside the %ld samples", what,
                         s ? "processed" : "reference", b, w->off[b], w->len[b], w->n_samples);
        }
        meta.offx[b] = x->off[b]; meta.lx[b] = x->len[b];
        meta.offy[b] = y->off[b]; meta.ly[b] = y->len[b];
        max_lx = max(max_lx, x->len[b]);
        max_l = max(max_l, max(x->len[b], y->len[b]));
    }
    return 0;
}

}  // namespace

extern "C" size_t st_xcorr_workspace_bytes(int B, int max_len, int D) {
    if (B < 1 || B > XC_MAX_B || max_len < 1 || max_len > XC_MAX_LEN || D < 0 || D > XC_MAX_LAG) return 0;
    return round64((size_t)B * xcorr_chunk_rows(max_len) * (2 * (size_t)D + 1) * sizeof(double));
}

extern "C" int st_xcorr_delay(const st_wave_batch* x, const st_wave_batch* y, int max_lag, int32_t* delay, float* coef, double* corr, void* ws,
                              void* stream) {
    (void)hipGetLastError();
    XcMeta meta;
    int max_lx, max_l, rc;
    if ((rc = pair_meta("st_xcorr_delay", x, y, meta, max_lx, max_l)) != 0) return rc;
    ST_CHECK_ARG(max_lag >= 0 && max_lag <= XC_MAX_LAG, "st_xcorr_delay: max_lag %d outside [0, %d]", max_lag, XC_MAX_LAG);
    if (x->B == 0) return 0;
    ST_CHECK_ARG(delay && coef && ws, "st_xcorr_delay: null pointer");
    ST_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "st_xcorr_delay: the workspace must be 8-byte aligned");
    const int B = x->B, D = max_lag, nlags = 2 * D + 1;
    const int nch_stride = xcorr_chunk_rows(max_lx);               // rows of the workspace a pair: at least its own chunks
    double* part = reinterpret_cast<double*>(ws);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(xcorr_partial_kernel, dim3((unsigned)((nlags + XC_T - 1) / XC_T), (unsigned)nch_stride, B), dim3(XC_NT), 0, st, x->x, y->x, meta, D,
                       nch_stride, part);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(xcorr_finish_kernel, dim3(B), dim3(XC_FT), 0, st, x->x, y->x, meta, D, nch_stride, part, corr, delay, coef);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t st_sisdr_workspace_bytes(int B, int max_len) {
    if (B < 1 || B > XC_MAX_B || max_len < 1 || max_len > XC_MAX_LEN) return 0;
    return round64((size_t)B * ((max_len + SD_CHUNK - 1) / SD_CHUNK) * 5 * sizeof(double));
}

extern "C" int st_sisdr_batch(const st_wave_batch* x, const st_wave_batch* y, const int32_t* delay, int zero_mean, double* sums, float* score,
                              void* ws, void* stream) {
    (void)hipGetLastError();
    XcMeta meta;
    int max_lx, max_l, rc;
    if ((rc = pair_meta("st_sisdr_batch", x, y, meta, max_lx, max_l)) != 0) return rc;
    if (x->B == 0) return 0;
    ST_CHECK_ARG(sums && score && ws, "st_sisdr_batch: null pointer");
    ST_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "st_sisdr_batch: the workspace must be 8-byte aligned");
    const int B = x->B;
    const int nch_stride = (max_l + SD_CHUNK - 1) / SD_CHUNK;      // n <= the longer side of every pair
    double* part = reinterpret_cast<double*>(ws);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sisdr_partial_kernel, dim3((unsigned)nch_stride, B), dim3(XC_NT), 0, st, x->x, y->x, meta, delay, nch_stride, part);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(sisdr_finish_kernel, dim3(B), dim3(ST_WAVE), 0, st, meta, delay, zero_mean, nch_stride, part, sums, score);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_wave_gather(const float* src, long src_n, const long* src_off, float* dst, long dst_n, const long* dst_off, const int* len, int B,
                              void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(B >= 0 && B <= XC_MAX_B, "st_wave_gather: batch %d outside [0, %d]", B, XC_MAX_B);
    if (B == 0) return 0;
    ST_CHECK_ARG(src && dst && src_off && dst_off && len, "st_wave_gather: null pointer");
    GatherMeta meta;
    memset(&meta, 0, sizeof(meta));
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        ST_CHECK_ARG(len[b] >= 1 && len[b] <= XC_MAX_LEN, "st_wave_gather: span %d has %d samples, outside [1, %d]", b, len[b], XC_MAX_LEN);
        ST_CHECK_ARG(src_off[b] >= 0 && src_off[b] + len[b] <= src_n, "st_wave_gather: span %d [%ld, +%d) outside the %ld source samples", b, src_off[b],
                     len[b], src_n);
        ST_CHECK_ARG(dst_off[b] >= 0 && dst_off[b] + len[b] <= dst_n, "st_wave_gather: span %d [%ld, +%d) outside the %ld destination samples", b,
                     dst_off[b], len[b], dst_n);
        meta.so[b] = src_off[b]; meta.dof[b] = dst_off[b]; meta.len[b] = len[b];
        max_len = max(max_len, len[b]);
    }
    const int gx = min((max_len + XC_NT * 4 - 1) / (XC_NT * 4), 256);
    hipLaunchKernelGGL(wave_gather_kernel, dim3((unsigned)gx, B), dim3(XC_NT), 0, (hipStream_t)stream, src, dst, meta);
    ST_LAUNCH_CHECK();
    return 0;
}
