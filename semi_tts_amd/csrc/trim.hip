// trim.hip -- leading / trailing silence of a ragged batch of waveforms by frame energy (st_trim_silence): the definition of
// librosa.effects.trim / split with ref = max, center = True and zero padding.  Contract: include/semitts.h.
//
// Launch 1 (trim_energy_kernel, grid (runs of T_pad, B)).  A workgroup of 256 threads (4 waves) takes a run of TR_RUN consecutive
// frames of one utterance (fewer when (run - 1) hop + frame_length samples would not fit TR_MAX_SPAN: trim_run_length) and stages
// their common span in LDS once, zero outside the utterance -- never the neighbour's samples of the packed buffer.  off[b] is
// arbitrary, so the span's first global address is not 16-byte aligned in general: up to three head samples go one by one, then every
// thread copies 16-byte groups (a group that straddles an end of the utterance or of the span falls back to guarded single loads).
// Then a wave owns a frame: wave w takes the frames w, w + 4, ... of the run; lane l forms ONE chain acc = fmaf(x, x, acc) over
// j = l, l + 64, l + 128, ... < frame_length in ascending j (consecutive across lanes: no bank conflict), the 64 partials combine by
// the xor butterfly (offsets 32, 16, ..., 1) and lane 0 stores sum / frame_length (one correctly rounded quotient).  A frame's bits
// depend on its samples and the framing alone.  A NaN or an infinity reaches exactly the frames that read it, by IEEE arithmetic.
//
// Launch 2 (trim_bounds_kernel, one workgroup per utterance).  Pass A: the maximum of max(e, 1e-10) over the row and a finiteness
// flag.  Pass B walks the row in chunks of TR_CHUNK = 256 frames, thread tid on frame c + tid: the non-silent flags of t - 1, t, t + 1
// mark the run starts and ends, an inclusive block scan of the starts (wave scan by __shfl_up, wave totals through LDS) carried
// across the chunks numbers the runs in order, so the start of run k and its end -- the end at t belongs to run (starts up to t) - 1
// -- are written by the threads that see them.  Count, first and last index are block reductions.  No atomics, no workspace.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "st_common.h"

namespace {

constexpr int TR_NT = 256, TR_NW = TR_NT / ST_WAVE;
constexpr int TR_RUN = 16;                 // frames a workgroup takes from one staged span (ops.TRIM_RUN: the tests straddle it)
constexpr int TR_MAX_FL = 8192, TR_MAX_B = 64;
constexpr int TR_MAX_SPAN = 12288;         // staged samples of a run (48 KiB); one frame needs at most 8192
constexpr int TR_CHUNK = TR_NT;            // frames per step of launch 2
constexpr float TR_FLOOR = 1e-10f;

struct TrimMeta {
    long off[TR_MAX_B];
    int len[TR_MAX_B];
};

inline int trim_run_length(int frame_length, int hop) {
    long r = TR_RUN;
    while (r > 1 && (r - 1) * (long)hop + frame_length > TR_MAX_SPAN) --r;
    return (int)r;
}

// LDS: xs[span], span = (run - 1) hop + frame_length.  grid (runs of T_pad, B).
__global__ __launch_bounds__(TR_NT) void trim_energy_kernel(const float* __restrict__ x, TrimMeta meta, int fl, int hop, int run,
                                                            float* __restrict__ energy, int T_pad) {
    extern __shared__ __align__(16) float xs[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int L = meta.len[b];
    const long T = 1 + (long)(L / hop);
    const long t0 = (long)blockIdx.x * run;
    const int nt = (int)min((long)run, (long)T_pad - t0);          // frames of this run inside the output (>= 1 by the grid)
    const int nf = (int)max(0L, min((long)run, T - t0));           // frames of this run inside the utterance
    float* eb = energy + (size_t)b * T_pad + t0;
    if (nf == 0) {                                                 // (uniform) a run past the utterance: the padding rows
        for (int r = tid; r < nt; r += TR_NT) eb[r] = 0.0f;
        return;
    }
    const float* xb = x + meta.off[b];
    const long g0 = t0 * hop - fl / 2;                             // xs[j] = x_b[g0 + j], 0 outside [0, L)
    const int used = (nf - 1) * hop + fl;                          // <= span
    // the first j whose global address is 16-byte aligned (the address is formed as an integer: g0 may be negative)
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(xb) + (uintptr_t)(g0 * (long)sizeof(float));
    const int head = (int)((4u - (unsigned)((a0 >> 2) & 3u)) & 3u);
    if (tid < head && tid < used) {
        const long i = g0 + tid;
        xs[tid] = (i >= 0 && i < L) ? xb[i] : 0.0f;
    }
    for (int j = head + 4 * tid; j < used; j += 4 * TR_NT) {
        const long i = g0 + j;
        if (i >= 0 && i + 3 < L && j + 3 < used) {
            const f32x4 v = st_ld4(xb + i);
            xs[j] = v[0]; xs[j + 1] = v[1]; xs[j + 2] = v[2]; xs[j + 3] = v[3];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j + u < used) { const long ii = i + u; xs[j + u] = (ii >= 0 && ii < L) ? xb[ii] : 0.0f; }
        }
    }
    __syncthreads();
    const float fln = (float)fl;
    for (int r = wave; r < nf; r += TR_NW) {                       // (uniform in the wave)
        const float* xf = xs + r * hop;                            // reads up to xs[(nf - 1) hop + fl - 1] = xs[used - 1]
        float acc = 0.0f;
        for (int j = lane; j < fl; j += ST_WAVE) { const float v = xf[j]; acc = fmaf(v, v, acc); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) eb[r] = acc / fln;
    }
    for (int r = nf + tid; r < nt; r += TR_NT) eb[r] = 0.0f;
}

// one workgroup per utterance
__global__ __launch_bounds__(TR_NT) void trim_bounds_kernel(const float* __restrict__ energy, TrimMeta meta, int hop, float ratio, int pad,
                                                            int max_iv, int T_pad, int32_t* __restrict__ bounds,
                                                            int32_t* __restrict__ intervals, int32_t* __restrict__ n_iv) {
    __shared__ float s_m[TR_NW];
    __shared__ int s_bad[TR_NW];
    __shared__ int s_w[TR_NW];
    __shared__ int s_r[TR_NW][3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int L = meta.len[b];
    const long T = 1 + (long)(L / hop);
    const float* e = energy + (size_t)b * T_pad;
    int32_t* ivb = intervals ? intervals + (size_t)b * max_iv * 2 : nullptr;
    // ---- pass A: ref = max_t max(e_t, 1e-10), and whether every e_t is finite
    float m = TR_FLOOR;
    int bad = 0;
    for (long t = tid; t < T; t += TR_NT) {
        const float v = e[t];
        bad |= !(fabsf(v) <= FLT_MAX);
        m = fmaxf(m, v);                                           // (a NaN leaves m as it is; bad is set)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) { s_m[wave] = m; s_bad[wave] = bad; }
    __syncthreads();
    const float ref = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    if (bad) {                                                     // (uniform)
        if (tid == 0) {
            bounds[4 * b] = 0; bounds[4 * b + 1] = L; bounds[4 * b + 2] = -1; bounds[4 * b + 3] = 1;
            if (n_iv) n_iv[b] = 0;
        }
        if (ivb) for (int k = tid; k < 2 * max_iv; k += TR_NT) ivb[k] = -1;
        return;
    }
    const float thr = ref * ratio;                                 // one fp32 product
    // non-silent: e_t > thr, strictly.  (e_t >= ref adds nothing unless the product rounded up to ref itself -- a ratio within 2^-23
    // of 1 -- where it keeps the loudest frame non-silent, as the exact product would.)
    auto loud = [&](long t) -> bool {
        if (t < 0 || t >= T) return false;
        const float v = fmaxf(e[t], TR_FLOOR);
        return v > thr || v >= ref;
    };
    // ---- pass B
    int carry = 0;                                                 // runs that started before this chunk
    int cnt = 0, first = INT_MAX, last = -1;                       // (frame indices fit an int: T <= T_pad)
    for (long c = 0; c < T; c += TR_CHUNK) {                       // (uniform trip count)
        const long t = c + tid;
        const bool cur = loud(t);
        const bool sf = cur && !loud(t - 1), ef = cur && !loud(t + 1);
        int v = sf;
#pragma unroll
        for (int o = 1; o < ST_WAVE; o <<= 1) { const int up = __shfl_up(v, o, 64); if (lane >= o) v += up; }
        if (lane == ST_WAVE - 1) s_w[wave] = v;
        __syncthreads();
        int base = carry, total = 0;
#pragma unroll
        for (int w = 0; w < TR_NW; ++w) { if (w < wave) base += s_w[w]; total += s_w[w]; }
        const int k = base + v - 1;                                // the run frame t lies in, when it is non-silent
        if (ivb && k < max_iv) {
            if (sf) ivb[2 * k] = (int32_t)(t * hop);
            if (ef) ivb[2 * k + 1] = (int32_t)min((long)L, (t + 1) * hop);
        }
        if (cur) { ++cnt; first = min(first, (int)t); last = max(last, (int)t); }
        carry += total;
        __syncthreads();                                           // (the next chunk overwrites s_w)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        first = min(first, __shfl_xor(first, o, 64));
        last = max(last, __shfl_xor(last, o, 64));
    }
    if (lane == 0) { s_r[wave][0] = cnt; s_r[wave][1] = first; s_r[wave][2] = last; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TR_NW; ++w) { cnt += s_r[w][0]; first = min(first, s_r[w][1]); last = max(last, s_r[w][2]); }
        bounds[4 * b] = (int32_t)max(0L, (long)first * hop - pad);       // (cnt >= 1: the loudest frame is non-silent)
        bounds[4 * b + 1] = (int32_t)min((long)L, ((long)last + 1) * hop + pad);
        bounds[4 * b + 2] = cnt;
        bounds[4 * b + 3] = 0;
        if (n_iv) n_iv[b] = carry;
    }
    if (ivb) for (int k = 2 * min(carry, max_iv) + tid; k < 2 * max_iv; k += TR_NT) ivb[k] = -1;
}

}  // namespace

extern "C" int st_trim_run_length(int frame_length, int hop) {
    if (hop < 1 || frame_length < hop || frame_length > TR_MAX_FL) return 0;
    return trim_run_length(frame_length, hop);
}

extern "C" int st_trim_silence(const st_wave_batch* w, int frame_length, int hop, float ratio, int pad, int max_iv, float* energy, int T_pad,
                               int32_t* bounds, int32_t* intervals, int32_t* n_iv, void* stream) {
    (void)hipGetLastError();
    ST_CHECK_ARG(w && w->x && w->off && w->len && energy && bounds, "st_trim_silence: null pointer");
    ST_CHECK_ARG(w->B >= 1 && w->B <= TR_MAX_B, "st_trim_silence: batch %d outside [1, %d]", w->B, TR_MAX_B);
    ST_CHECK_ARG(hop >= 1 && hop <= frame_length && frame_length <= TR_MAX_FL, "st_trim_silence: needs 1 <= hop <= frame_length <= %d (hop %d, frame_length %d)",
                 TR_MAX_FL, hop, frame_length);
    ST_CHECK_ARG(ratio > 0.0f && ratio < 1.0f, "st_trim_silence: ratio %g outside (0, 1)", (double)ratio);
    ST_CHECK_ARG(pad >= 0, "st_trim_silence: pad %d below 0", pad);
    ST_CHECK_ARG(max_iv >= 0 && (max_iv == 0) == (intervals == nullptr), "st_trim_silence: max_iv %d and intervals %s: max_iv is 0 exactly without intervals",
                 max_iv, intervals ? "given" : "NULL");
    TrimMeta meta;
    memset(&meta, 0, sizeof(meta));
    long tmax = 0;
    for (int b = 0; b < w->B; ++b) {
        ST_CHECK_ARG(w->len[b] >= 1 && w->off[b] >= 0 && w->off[b] + w->len[b] <= w->n_samples,
                     "st_trim_silence: utterance %d [%ld, +%d) outside the %ld samples", b, w->off[b], w->len[b], w->n_samples);
        meta.off[b] = w->off[b];
        meta.len[b] = w->len[b];
        tmax = max(tmax, 1L + w->len[b] / hop);
    }
    ST_CHECK_ARG(T_pad >= tmax, "st_trim_silence: T_pad %d below the %ld frames of the longest utterance", T_pad, tmax);
    const int run = trim_run_length(frame_length, hop);
    const size_t lds = ((size_t)(run - 1) * hop + frame_length) * sizeof(float);       // at most 48 KiB
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(trim_energy_kernel, dim3((unsigned)(((long)T_pad + run - 1) / run), w->B), dim3(TR_NT), lds, st, w->x, meta, frame_length, hop, run,
                       energy, T_pad);
    ST_LAUNCH_CHECK();
    hipLaunchKernelGGL(trim_bounds_kernel, dim3(w->B), dim3(TR_NT), 0, st, energy, meta, hop, ratio, pad, max_iv, T_pad, bounds, intervals, n_iv);
    ST_LAUNCH_CHECK();
    return 0;
}
