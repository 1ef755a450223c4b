// f0.hip -- pitch of a ragged batch of waveforms by the YIN difference function (st_f0_yin), and the F0 figures of two tracks along a
// DTW path (st_f0_path_scores).  Contracts: include/semitts.h.
//
// st_f0_yin.  A workgroup of 256 threads (4 waves) takes a run of F0_RUN consecutive frames of one utterance (fewer when
// (run - 1) hop + W + tau_max samples would not fit F0_MAX_SPAN: f0_run_length) and stages their common span of samples in LDS once,
// zero outside the utterance; the copy is also the non-finite check (a non-finite sample marks the frames whose slice holds it).
// Then a wave owns a frame: wave w takes the frames w, w + 4, ... of the run, and the lanes own lags.  Lane l of pass q holds the TL
// consecutive lags q 64 TL + l TL + k (k < TL) in registers and walks j = 0 .. W-1: x[s0 + j] is one address for the wave (a broadcast
// read), x[s0 + j + tau] is consecutive across lanes (no bank conflict), and J = 8 steps of j share one window of TL + J - 1 samples, so
// a step of J TL terms costs 2 J + TL - 1 LDS reads, not 2 J TL.  TL in {4, 6, 8} is chosen per call to waste the fewest lanes
// (f0_lags_per_lane).  Every d(tau) is ONE chain acc = fmaf(x - y, x - y, acc) over ascending j: its bits depend on the frame's samples
// alone.  The wave then forms c(tau) by a prefix sum (each lane sums a contiguous chunk of lags in ascending order, an inclusive scan
// of the 64 chunk sums by __shfl_up, and a second ascending walk), overwrites d by d', and finds tau0, tau* and the minimum by
// min-index reductions over the lanes.  No n_frames x tau_max array exists outside LDS.  No atomics: bitwise repeatable.
//
// st_f0_path_scores.  One workgroup of 256 threads per pair; thread tid takes the path entries tid, tid + 256, ... in ascending order
// into its own fp32 partial sums, the 64 partials of a wave are combined by the xor butterfly (offsets 32, 16, ..., 1) and the four
// wave sums as (w0 + w1) + (w2 + w3).
#include <math.h>
#include "st_common.h"

namespace {

constexpr int F0_NT = 256, F0_NW = F0_NT / ST_WAVE;
constexpr int F0_RUN = 8;                  // frames a workgroup takes from one staged span (ops.F0_RUN: the tests straddle it)
constexpr int F0_MAX_TAU = 1024, F0_MAX_W = 2048, F0_MAX_B = 64;
constexpr int F0_MAX_SPAN = 10240;         // staged samples of a run; one frame needs at most 3072
constexpr int F0_J = 8;                    // steps of j per window
constexpr int F0_PAD = ST_WAVE * 8 + F0_J; // zeros behind the span: the window reads of lags past tau_max (discarded) stay inside LDS

struct F0Meta {
    long off[F0_MAX_B];
    int len[F0_MAX_B];
};

inline int f0_run_length(int hop, int W, int tau_max) {
    long r = F0_RUN;
    while (r > 1 && (r - 1) * (long)hop + W + tau_max > F0_MAX_SPAN) --r;
    return (int)r;
}
// lags per lane: the passes of 64 TL lags that cover 0 .. tau_max cost passes * TL; the cheapest, the widest among equals
inline int f0_lags_per_lane(int tau_max) {
    int best = 4, cost = 1 << 30;
    for (int tl = 4; tl <= 8; tl += 2) {
        const int c = (tau_max + ST_WAVE * tl) / (ST_WAVE * tl) * tl;
        if (c <= cost) { cost = c; best = tl; }
    }
    return best;
}

__device__ __forceinline__ int f0_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float f0_wave_minf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// LDS: xs[span + F0_PAD] | dl[F0_NW][dstride], dstride = tau_max + 2.  grid (runs of T_pad, B).
template <int TL>
__global__ __launch_bounds__(F0_NT) void f0_yin_kernel(const float* __restrict__ x, F0Meta meta, int hop, int W, int tau_min, int tau_max,
                                                       float sample_rate, float threshold, int run, int span, float* __restrict__ f0,
                                                       float* __restrict__ aper, int T_pad) {
    extern __shared__ __align__(16) float f0_lds[];
    __shared__ int s_bad[F0_RUN];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int L = meta.len[b];
    const int T = 1 + L / hop;
    const int t0 = blockIdx.x * run;
    const int nt = min(run, T_pad - t0);           // frames of this run inside the output (>= 1 by the grid)
    const int nf = max(0, min(run, T - t0));       // frames of this run inside the utterance
    float* f0b = f0 + (size_t)b * T_pad + t0;
    float* apb = aper ? aper + (size_t)b * T_pad + t0 : nullptr;
    if (nf == 0) {                                 // (uniform) a run past the utterance: the padding rows
        for (int r = tid; r < nt; r += F0_NT) { f0b[r] = 0.0f; if (apb) apb[r] = 0.0f; }
        return;
    }
    float* xs = f0_lds;
    const int dstride = tau_max + 2;
    float* dl = f0_lds + span + F0_PAD + wave * dstride;
    const int slice = W + tau_max;                 // samples a frame reads: [s0, s0 + W + tau_max)
    if (tid < F0_RUN) s_bad[tid] = 0;
    __syncthreads();
    const float* xb = x + meta.off[b];
    const long g0 = (long)t0 * hop - W / 2;
    const int used = (nf - 1) * hop + slice;       // <= span
    for (int j = tid; j < span + F0_PAD; j += F0_NT) {
        const long i = g0 + j;
        float v = 0.0f;
        if (j < used && i >= 0 && i < L) {
            v = xb[i];
            if (!(fabsf(v) <= 3.402823466e38f)) {                   // NaN or an infinity: mark the frames r with r hop <= j < r hop + slice
                for (int r = 0; r < nf; ++r)
                    if (j >= r * hop && j - r * hop < slice) s_bad[r] = 1;      // (every writer stores 1)
            }
        }
        xs[j] = v;
    }
    __syncthreads();

    const int CH = (tau_max + ST_WAVE - 1) / ST_WAVE;              // lags a lane takes in the scan and the searches: 1 + lane CH ...
    const int lo = 1 + lane * CH, hi = min(tau_max, lane * CH + CH);   // [lo, hi], empty when lo > hi
    for (int it = 0; it < (run + F0_NW - 1) / F0_NW; ++it) {        // (uniform trip count: every wave reaches the barriers)
        const int r = it * F0_NW + wave;
        const bool act = r < nf;
        if (act) {
            const float* xf = xs + r * hop;
            for (int tb = lane * TL; tb - lane * TL <= tau_max; tb += ST_WAVE * TL) {     // (uniform: the pass base tb - lane TL)
                const float* xw = xf + tb;
                float acc[TL];
#pragma unroll
                for (int k = 0; k < TL; ++k) acc[k] = 0.0f;
                int j0 = 0;
                for (; j0 + F0_J <= W; j0 += F0_J) {
                    float xj[F0_J], win[TL + F0_J - 1];
#pragma unroll
                    for (int u = 0; u < F0_J; ++u) xj[u] = xf[j0 + u];
#pragma unroll
                    for (int u = 0; u < TL + F0_J - 1; ++u) win[u] = xw[j0 + u];
#pragma unroll
                    for (int u = 0; u < F0_J; ++u) {
#pragma unroll
                        for (int k = 0; k < TL; ++k) { const float e = xj[u] - win[u + k]; acc[k] = fmaf(e, e, acc[k]); }
                    }
                }
                for (; j0 < W; ++j0) {
                    const float a = xf[j0];
#pragma unroll
                    for (int k = 0; k < TL; ++k) { const float e = a - xw[j0 + k]; acc[k] = fmaf(e, e, acc[k]); }
                }
#pragma unroll
                for (int k = 0; k < TL; ++k)
                    if (tb + k <= tau_max) dl[tb + k] = acc[k];
            }
        }
        __syncthreads();
        // ---- c(tau) and d'(tau) in place
        float part = 0.0f;
        if (act) {
            for (int t = lo; t <= hi; ++t) part += dl[t];
            float inc = part;
#pragma unroll
            for (int o = 1; o < ST_WAVE; o <<= 1) { const float up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
            float c = __shfl_up(inc, 1, 64);                        // exclusive: the sum of the chunks of the lanes before
            if (lane == 0) c = 0.0f;
            for (int t = lo; t <= hi; ++t) {
                const float d = dl[t];
                c += d;
                dl[t] = c > 0.0f ? d * (float)t / c : 1.0f;
            }
        }
        __syncthreads();
        // ---- tau0: the first lag under the threshold; the minimum for an unvoiced frame
        int tau0 = 0x7fffffff;
        float dmin = INFINITY;
        if (act) {
            for (int t = max(lo, tau_min); t <= hi; ++t) {
                const float v = dl[t];
                dmin = fminf(dmin, v);
                if (v < threshold && tau0 == 0x7fffffff) tau0 = t;
            }
            tau0 = f0_wave_min(tau0);
            dmin = f0_wave_minf(dmin);
            float fo = 0.0f, ao = dmin;
            if (tau0 != 0x7fffffff) {              // (uniform in the wave)
                int ts = 0x7fffffff;
                for (int t = max(lo, tau0); t <= hi; ++t)
                    if (t == tau_max || dl[t + 1] >= dl[t]) { ts = t; break; }
                ts = f0_wave_min(ts);              // (tau_max always qualifies)
                const float pb = dl[ts];
                float delta = 0.0f;
                if (ts < tau_max) {
                    const float pa = dl[ts - 1], pc = dl[ts + 1];
                    if (pa > pb) delta = 0.5f * (pa - pc) / ((pa - pb) + (pc - pb));
                }
                fo = sample_rate / ((float)ts + delta);
                ao = pb;
            }
            if (s_bad[r]) { fo = NAN; ao = NAN; }
            if (lane == 0) { f0b[r] = fo; if (apb) apb[r] = ao; }
        }
        __syncthreads();                           // (the next frame of this wave overwrites dl)
    }
    for (int r = nf + tid; r < nt; r += F0_NT) { f0b[r] = 0.0f; if (apb) apb[r] = 0.0f; }
}

template <int TL>
void f0_launch(dim3 grid, size_t lds, hipStream_t st, const float* x, const F0Meta& meta, int hop, int W, int tau_min, int tau_max,
               float sample_rate, float threshold, int run, int span, float* f0, float* aper, int T_pad) {
    hipLaunchKernelGGL((f0_yin_kernel<TL>), grid, dim3(F0_NT), lds, st, x, meta, hop, W, tau_min, tau_max, sample_rate, threshold, run, span, f0,
                       aper, T_pad);
}

__global__ __launch_bounds__(F0_NT) void f0_path_scores_kernel(const float* __restrict__ fx, long x_sb, const float* __restrict__ fy, long y_sb,
                                                               const int32_t* __restrict__ path, const int32_t* __restrict__ path_len, int P,
                                                               int32_t* __restrict__ counts, float* __restrict__ sums) {
    __shared__ float s_f[F0_NW][2];
    __shared__ int s_i[F0_NW][3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int n = min(max(path_len[b], 0), P);
    const float* xb = fx + (size_t)b * x_sb;
    const float* yb = fy + (size_t)b * y_sb;
    const int32_t* pb = path + (size_t)b * P * 2;
    float s2 = 0.0f, s1 = 0.0f;
    int nb = 0, nv = 0, ng = 0;
    for (int p = tid; p < n; p += F0_NT) {
        const float a = xb[pb[2 * p]], c = yb[pb[2 * p + 1]];
        const bool va = a > 0.0f, vc = c > 0.0f;       // (NaN compares false: unvoiced)
        nv += va != vc;
        if (va && vc) {
            ++nb;
            const double da = (double)a, dc = (double)c;
            ng += fabs(da - dc) > 0.2 * dc;
            const float cents = (float)(1200.0 * log2(da / dc));      // one rounding to fp32
            s2 = fmaf(cents, cents, s2);
            s1 += cents;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s2 += __shfl_xor(s2, o, 64);
        s1 += __shfl_xor(s1, o, 64);
        nb += __shfl_xor(nb, o, 64);
        nv += __shfl_xor(nv, o, 64);
        ng += __shfl_xor(ng, o, 64);
    }
    if (lane == 0) { s_f[wave][0] = s2; s_f[wave][1] = s1; s_i[wave][0] = nb; s_i[wave][1] = nv; s_i[wave][2] = ng; }
    __syncthreads();
    if (tid == 0) {
        counts[4 * b] = n;
        for (int k = 0; k < 3; ++k) counts[4 * b + 1 + k] = (s_i[0][k] + s_i[1][k]) + (s_i[2][k] + s_i[3][k]);
        for (int k = 0; k < 2; ++k) sums[2 * b + k] = (s_f[0][k] + s_f[1][k]) + (s_f[2][k] + s_f[3][k]);
    }
}

}  // namespace

extern "C" int st_f0_run_length(int hop, int W, int tau_max) {
    if (hop < 1 || W < 1 || W > F0_MAX_W || tau_max < 3 || tau_max > F0_MAX_TAU) return 0;
    return f0_run_length(hop, W, tau_max);
}

extern "C" int st_f0_yin(const st_wave_batch* w, int hop, int W, int tau_min, int tau_max, float sample_rate, float threshold, float* f0,
                         float* aper, int T_pad, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(w && w->x && w->off && w->len && f0, "st_f0_yin: null pointer");
    ST_CHECK_ARG(w->B >= 1 && w->B <= F0_MAX_B, "st_f0_yin: batch %d outside [1, %d]", w->B, F0_MAX_B);
    ST_CHECK_ARG(hop >= 1, "st_f0_yin: hop %d below 1", hop);
    ST_CHECK_ARG(tau_min >= 2 && tau_min < tau_max && tau_max <= F0_MAX_TAU, "st_f0_yin: lags [%d, %d] outside 2 <= tau_min < tau_max <= %d", tau_min,
                 tau_max, F0_MAX_TAU);
    ST_CHECK_ARG(W >= 1 && W <= F0_MAX_W, "st_f0_yin: window %d outside [1, %d]", W, F0_MAX_W);
    ST_CHECK_ARG(threshold > 0.0f && threshold <= 1.0f, "st_f0_yin: threshold %g outside (0, 1]", (double)threshold);
    ST_CHECK_ARG(sample_rate > 0.0f && sample_rate < INFINITY, "st_f0_yin: sample rate must be finite and positive (got %g)", (double)sample_rate);
    F0Meta meta;
    memset(&meta, 0, sizeof(meta));
    long tmax = 0;
    for (int b = 0; b < w->B; ++b) {
        ST_CHECK_ARG(w->len[b] >= 1 && w->off[b] >= 0 && w->off[b] + w->len[b] <= w->n_samples, "st_f0_yin: utterance %d [%ld, +%d) outside the %ld samples",
                     b, w->off[b], w->len[b], w->n_samples);
        meta.off[b] = w->off[b];
        meta.len[b] = w->len[b];
        tmax = max(tmax, 1L + w->len[b] / hop);
    }
    ST_CHECK_ARG(T_pad >= tmax, "st_f0_yin: T_pad %d below the %ld frames of the longest utterance", T_pad, tmax);
    const int run = f0_run_length(hop, W, tau_max);
    const int span = (run - 1) * hop + W + tau_max;
    const size_t lds = ((size_t)span + F0_PAD + (size_t)F0_NW * (tau_max + 2)) * sizeof(float);      // at most 60 KiB
    const dim3 grid((unsigned)((T_pad + run - 1) / run), w->B);
    hipStream_t st = (hipStream_t)stream;
    switch (f0_lags_per_lane(tau_max)) {
        case 4: f0_launch<4>(grid, lds, st, w->x, meta, hop, W, tau_min, tau_max, sample_rate, threshold, run, span, f0, aper, T_pad); break;
        case 6: f0_launch<6>(grid, lds, st, w->x, meta, hop, W, tau_min, tau_max, sample_rate, threshold, run, span, f0, aper, T_pad); break;
        default: f0_launch<8>(grid, lds, st, w->x, meta, hop, W, tau_min, tau_max, sample_rate, threshold, run, span, f0, aper, T_pad); break;
    }
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_f0_path_scores(const float* f0_x, long x_sb, int Tx, const float* f0_y, long y_sb, int Ty, const int32_t* path,
                                 const int32_t* path_len, int B, int P, int32_t* counts, float* sums, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(f0_x && f0_y && path && path_len && counts && sums, "st_f0_path_scores: null pointer");
    ST_CHECK_ARG(B >= 1 && Tx >= 1 && Ty >= 1 && P >= 1, "st_f0_path_scores: B=%d, Tx=%d, Ty=%d, P=%d must all be at least 1", B, Tx, Ty, P);
    ST_CHECK_ARG(x_sb >= 0 && y_sb >= 0, "st_f0_path_scores: negative row strides %ld, %ld", x_sb, y_sb);
    hipLaunchKernelGGL(f0_path_scores_kernel, dim3(B), dim3(F0_NT), 0, (hipStream_t)stream, f0_x, x_sb, f0_y, y_sb, path, path_len, P, counts, sums);
    ST_LAUNCH_CHECK();
    return 0;
}
