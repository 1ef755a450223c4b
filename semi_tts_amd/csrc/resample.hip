// resample.hip -- sample-rate conversion of a ragged batch of waveforms (st_resample_batch): windowed-sinc interpolation as a
// polyphase FIR.  The filter (Hann-windowed sinc, the definition of include/semitts.h) is tabulated on the host per phase
// p = m mod n; the kernel is the dense part: y[m] = sum_k table[p][k] * x[floor(m o / n) + first[p] + k].
#include "st_common.h"

#include <limits.h>

namespace {

constexpr int RS_TILE = 1024;          // outputs per workgroup (RESAMPLE_TILE in ops.py: the tests straddle it)
constexpr int RS_THREADS = 256;        // 4 outputs per thread, strided by the workgroup: coalesced stores
constexpr int RS_MAX_B = 64;           // utterances per call (FEATURES_MAX_BATCH): the metadata travels by value
// LDS of one workgroup: the staged table rows (row stride taps | 1, plus one `first` per row) and the input span of the tile.
// Together at most 63 KB, so two workgroups fit the 160 KB of a CU at the largest accepted ratio.
constexpr int RS_MAX_TABLE = 9216;     // floats (RESAMPLE_MAX_TABLE_FLOATS)
constexpr int RS_MAX_STAGE = 6912;     // floats (RESAMPLE_MAX_STAGE_FLOATS)

struct ResampleMeta {
    long off[RS_MAX_B];        // first input sample of utterance b in the packed input
    long out_off[RS_MAX_B];    // first output sample of utterance b in the packed output
    int len[RS_MAX_B];         // input length L_b
    int out_len[RS_MAX_B];     // ceil(n L_b / o)
};

__device__ __forceinline__ float rs_sample(const float* x, long i) { return x[i]; }
__device__ __forceinline__ float rs_sample(const short* x, long i) { return (float)x[i] * (1.0f / 32768.0f); }      // exact

// grid (tiles of the longest output, B).  LDS: tab[R][S] | first[R] | xs[span], R = min(n, RS_TILE) rows starting at the phase of
// the tile's first output (a tile of RS_TILE consecutive outputs walks the phases cyclically), S = taps | 1 (odd stride: lanes
// reading tap k of consecutive rows fall on distinct banks).  xs[j] = x[s0 + j], s0 = floor(m0 o / n) + first_min, zero outside
// the utterance; span (from the host) covers the last output's last tap for any m0.
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const T* __restrict__ x, ResampleMeta meta, int o, int n, int taps, int S,
                                                              int R, int first_min, int span, const int* __restrict__ first,
                                                              const float* __restrict__ table, float* __restrict__ y) {
    extern __shared__ __align__(16) float rs_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Lout = meta.out_len[b];
    const int m0 = blockIdx.x * RS_TILE;
    if (m0 >= Lout) return;
    float* tab = rs_lds;
    int* fst = reinterpret_cast<int*>(rs_lds + R * S);
    float* xs = rs_lds + R * S + R;
    const int q0 = m0 / n, p0 = m0 - q0 * n;
    for (int idx = tid; idx < R * taps; idx += RS_THREADS) {
        const int r = idx / taps, k = idx - r * taps;
        int p = p0 + r;
        if (p >= n) p -= n;
        tab[r * S + k] = table[(long)p * taps + k];
    }
    for (int r = tid; r < R; r += RS_THREADS) {
        int p = p0 + r;
        if (p >= n) p -= n;
        fst[r] = first[p];
    }
    const long L = meta.len[b];
    const T* xb = x + meta.off[b];
    const long s0 = (long)q0 * o + (p0 * o) / n + first_min;      // (o n < 2^31, checked by the host)
    for (int j = tid; j < span; j += RS_THREADS) {
        const long i = s0 + j;
        xs[j] = (i >= 0 && i < L) ? rs_sample(xb, i) : 0.0f;
    }
    __syncthreads();
    const int cnt = min(RS_TILE, Lout - m0);
    float* yb = y + meta.out_off[b] + m0;
    for (int t = tid; t < cnt; t += RS_THREADS) {
        const int m = m0 + t;
        const int q = m / n, p = m - q * n;
        const int r = t % R;                                      // the staged row of phase p
        const long fl = (long)q * o + (p * o) / n;                // floor(m o / n)
        int base = (int)(fl - s0) + fst[r];                       // first tap: x[fl + first[p]]
        base = min(max(base, 0), span - taps);                   // (never moves a consistent table: keeps any `first` inside the stage)
        const float* h = tab + r * S;
        const float* xx = xs + base;
        float acc = 0.0f;
        for (int k = 0; k < taps; ++k) acc = fmaf(h[k], xx[k], acc);      // one chain, ascending taps: the same bits in any tile or batch
        yb[t] = acc;
    }
}

}  // namespace

extern "C" int st_resample_batch(const void* x, int pcm16, long n_samples, const long* off, const int* len, int B, int o, int n, int taps,
                                 int first_min, int first_max, const int* first, const float* table, float* y, long n_out,
                                 const long* out_off, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(x && off && len && first && table && y && out_off, "st_resample_batch: null pointer");
    ST_CHECK_ARG(B > 0 && B <= RS_MAX_B, "st_resample_batch: batch %d outside [1, %d]", B, RS_MAX_B);
    ST_CHECK_ARG(o > 0 && n > 0 && (long)o * n <= INT_MAX, "st_resample_batch: bad ratio %d / %d", o, n);
    ST_CHECK_ARG(taps > 0 && first_min <= first_max && (long)first_max - first_min < RS_MAX_STAGE, "st_resample_batch: bad taps %d / first [%d, %d]",
                 taps, first_min, first_max);
    const int S = taps | 1, R = min(n, RS_TILE);
    const long span = ((long)(RS_TILE - 1) * o + n - 1) / n + (first_max - first_min) + taps;
    ST_CHECK_ARG((long)R * S + R <= RS_MAX_TABLE, "st_resample_batch: %d phases of %d taps need %ld floats of LDS, the limit is %d", n, taps,
                 (long)R * S + R, RS_MAX_TABLE);
    ST_CHECK_ARG(span <= RS_MAX_STAGE, "st_resample_batch: a tile of %d outputs at %d / %d spans %ld input samples, the limit is %d", RS_TILE,
                 o, n, span, RS_MAX_STAGE);
    ResampleMeta meta;
    memset(&meta, 0, sizeof(meta));
    long lmax = 0;
    for (int b = 0; b < B; ++b) {
        ST_CHECK_ARG(len[b] > 0 && off[b] >= 0 && off[b] + len[b] <= n_samples, "st_resample_batch: utterance %d [%ld, +%d) outside the %ld samples",
                     b, off[b], len[b], n_samples);
        const long lo = ((long)n * len[b] + o - 1) / o;
        ST_CHECK_ARG(lo <= INT_MAX, "st_resample_batch: utterance %d gives %ld samples", b, lo);
        ST_CHECK_ARG(out_off[b] >= 0 && out_off[b] + lo <= n_out, "st_resample_batch: output %d [%ld, +%ld) outside the %ld samples", b,
                     out_off[b], lo, n_out);
        meta.off[b] = off[b];
        meta.out_off[b] = out_off[b];
        meta.len[b] = len[b];
        meta.out_len[b] = (int)lo;
        lmax = max(lmax, lo);
    }
    const dim3 grid((unsigned)((lmax + RS_TILE - 1) / RS_TILE), B);
    const size_t lds = ((size_t)R * S + R + span) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (pcm16)
        hipLaunchKernelGGL(resample_kernel<short>, grid, dim3(RS_THREADS), lds, s, (const short*)x, meta, o, n, taps, S, R, first_min, (int)span,
                           first, table, y);
    else
        hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(RS_THREADS), lds, s, (const float*)x, meta, o, n, taps, S, R, first_min, (int)span,
                           first, table, y);
    ST_LAUNCH_CHECK();
    return 0;
}
