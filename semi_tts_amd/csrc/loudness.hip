// loudness.hip -- ITU-R BS.1770-4 / EBU R 128 integrated loudness of a ragged batch of waveforms (st_loudness_batch) and the gain
// that brings it to a target (st_wave_gain).  Contract: include/semitts.h.  Mono, channel 0, the raw waveform.  Out of scope:
// multichannel weighting, true (oversampled) peak, loudness range (Tech 3342) and short-term loudness.
//
// The K-weighting filter is two biquads, a 4th-order recurrence s' = A s + B x, y = C s + D x over the state s = (shelf s1, s2,
// high-pass s1, s2) of the DF2-transposed forms.  Time is cut into hops of 100 ms, the unit the meter sums over anyway, and a hop
// into 256 runs of r = ceil(hop / 256) samples, one per thread.  EVERYTHING along the recurrence is float64 (coefficients, states,
// powers of A, sums of squares): the high-pass has 1 + a1 + a2 = 2.5e-5 at 48 kHz, which fp32 cannot hold.
//
// Launch 1 (loud_hop_kernel<false>, grid (units, B)).  A workgroup stages its hop in LDS behind pad = 256 r - hop zeros, so that the
// short run sits at the FRONT of the hop; a thread filters its run from zero state, skipping the pad (zero input on zero state stays
// zero: the pad is exact).  A Kogge-Stone scan over the 256 end states, step k applying A^(r 2^k) to the state 2^k threads back,
// leaves the zero-state state after every run; thread 255 holds the hop's zero-state end state Q[h] and writes it to the workspace.
// The same launch reduces max |x| and a finiteness mark per unit; the unit of the tail (the samples past the last full hop) does
// only that.
// Launch 2 (loud_carry_kernel, one wave per utterance): S[0] = 0, S[h + 1] = A^hop S[h] + Q[h], lane 0 walking over Q staged in LDS.
// Launch 3 (loud_hop_kernel<true>, grid (H_pad, B)): the same staging and scan, then thread t starts from its true state
// (zero-state state after run t - 1) + A^(samples of the hop before run t) S[h] and filters its run again, summing y^2 in ONE
// ascending chain; the 256 chains combine by the xor butterfly (offsets 32 .. 1) and the four wave sums as (w0 + w1) + (w2 + w3);
// one store of e[h], rounded once.  Rows h >= H are written 0.
// Launch 4 (loud_gate_kernel, one workgroup per utterance): blocks, gates, statistics and the gain from the fp32 e[h], in float64;
// thread t sums the blocks t, t + 256, ... in ascending order, then the same butterfly.
// st_wave_gain: one elementwise launch that reads the gain from stats on the device.
// No atomics, no host read; every value depends on its utterance's samples and fs alone, so it is bitwise repeatable and a
// non-finite sample poisons exactly its utterance (the workspace rows of an utterance are its own).
#include <float.h>
#include <math.h>
#include "st_common.h"

namespace {

constexpr int LD_NT = 256, LD_NW = LD_NT / ST_WAVE;
constexpr int LD_MAX_B = 64, LD_MAX_R = 19;               // r = ceil(hop / 256) = 4 .. 19 for 8 .. 48 kHz
constexpr int LD_MIN_FS = 8000, LD_MAX_FS = 48000;
constexpr int LD_TAB_COEF = 0, LD_TAB_P = 8, LD_TAB_AH = 136, LD_TAB_T = 152;      // ST_LOUDNESS_TABLE_DOUBLES = 152 + 256 * 16
constexpr int LD_CARRY_CHUNK = 64;

struct LoudMeta {
    long off[LD_MAX_B];
    int len[LD_MAX_B];
};

struct KW { double b0, b1, b2, a1, a2, p1, p2; };

__device__ __forceinline__ KW ld_coefs(const double* __restrict__ tab) {
    return KW{tab[LD_TAB_COEF], tab[LD_TAB_COEF + 1], tab[LD_TAB_COEF + 2], tab[LD_TAB_COEF + 3], tab[LD_TAB_COEF + 4],
              tab[LD_TAB_COEF + 5], tab[LD_TAB_COEF + 6]};
}

// one sample through both stages (DF2 transposed; the high-pass has b = (1, -2, 1) exactly) -> the K-weighted sample
__device__ __forceinline__ double ld_step(const KW& k, double x, double s[4]) {
    const double y1 = k.b0 * x + s[0];
    s[0] = k.b1 * x - k.a1 * y1 + s[1];
    s[1] = k.b2 * x - k.a2 * y1;
    const double y = y1 + s[2];
    s[2] = -2.0 * y1 - k.p1 * y + s[3];
    s[3] = y1 - k.p2 * y;
    return y;
}

// v += M u, M a row-major 4 x 4 matrix
__device__ __forceinline__ void ld_matvec_add(const double* __restrict__ M, const double u[4], double v[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += M[4 * i] * u[0] + M[4 * i + 1] * u[1] + M[4 * i + 2] * u[2] + M[4 * i + 3] * u[3];
}

__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup in a fixed order; every thread gets it.  s_d: LD_NW doubles of LDS, free again after the call
__device__ __forceinline__ double ld_block_sum(double v, double* s_d) {
    v = ld_wave_sum(v);
    if ((threadIdx.x & (ST_WAVE - 1)) == 0) s_d[threadIdx.x / ST_WAVE] = v;
    __syncthreads();
    const double t = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ double ld_block_max(double v, double* s_d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & (ST_WAVE - 1)) == 0) s_d[threadIdx.x / ST_WAVE] = v;
    __syncthreads();
    const double t = fmax(fmax(s_d[0], s_d[1]), fmax(s_d[2], s_d[3]));
    __syncthreads();
    return t;
}

// workspace (doubles), U = H_pad + 1 units a row: Q (B, U, 4) | S (B, U, 4) | pk (B, U)
__device__ __forceinline__ double* ld_ws_q(double* ws, int B, int U, int b) { return ws + (size_t)b * U * 4; }
__device__ __forceinline__ double* ld_ws_s(double* ws, int B, int U, int b) { return ws + ((size_t)B * U + (size_t)b * U) * 4; }
__device__ __forceinline__ double* ld_ws_pk(double* ws, int B, int U, int b) { return ws + (size_t)B * U * 8 + (size_t)b * U; }

// FINAL = false: grid (largest ceil(L / hop), B) -> Q and pk.  FINAL = true: grid (H_pad, B) -> hop_energy.
template <bool FINAL>
__global__ __launch_bounds__(LD_NT) void loud_hop_kernel(const float* x, LoudMeta meta, int hop, int r, const double* __restrict__ tab,
                                                         double* ws, int U, float* __restrict__ hop_energy, int H_pad) {
    __shared__ float xs[LD_NT * LD_MAX_R];
    __shared__ double sv[LD_NT * 4];
    __shared__ double s_d[LD_NW];
    __shared__ float s_m[LD_NW];
    __shared__ int s_bad[LD_NW];
    const int b = blockIdx.y, B = gridDim.y, u = blockIdx.x, tid = threadIdx.x, lane = tid & (ST_WAVE - 1), wave = tid / ST_WAVE;
    const int L = meta.len[b];
    const int H = L / hop;
    if (FINAL) {
        if (u >= H) {                                              // (uniform) a padding row
            if (tid == 0) hop_energy[(size_t)b * H_pad + u] = 0.0f;
            return;
        }
    } else if (u > H || (u == H && (long)H * hop == L)) {          // (uniform) past the utterance
        return;
    }
    const float* xb = x + meta.off[b] + (long)u * hop;             // the unit's first sample
    float m = 0.0f;
    int bad = 0;
    const int pad = LD_NT * r - hop;                               // 0 <= pad < 256
    if (u < H) {
        for (int j = tid; j < LD_NT * r; j += LD_NT) {             // xs[j] = sample j - pad of the hop, 0 in the pad
            const int i = j - pad;
            const float v = i >= 0 ? xb[i] : 0.0f;                 // i < hop: inside the utterance
            xs[j] = v;
            if (!FINAL) { bad |= !(fabsf(v) <= FLT_MAX); m = fmaxf(m, fabsf(v)); }
        }
    } else if (!FINAL) {                                           // the tail: the peak only
        const int n = L - H * hop;                                 // 1 <= n < hop
        for (int i = tid; i < n; i += LD_NT) { const float v = xb[i]; bad |= !(fabsf(v) <= FLT_MAX); m = fmaxf(m, fabsf(v)); }
    }
    if (!FINAL) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); bad |= __shfl_xor(bad, o, 64); }
        if (lane == 0) { s_m[wave] = m; s_bad[wave] = bad; }
        __syncthreads();
        if (tid == 0) {
            const float mm = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
            ld_ws_pk(ws, B, U, b)[u] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? (double)NAN : (double)mm;
        }
        if (u == H) return;                                        // (uniform)
    } else {
        __syncthreads();
    }
    const KW kw = ld_coefs(tab);
    const float* xr = xs + tid * r;
    const int i0 = min(r, max(0, pad - tid * r));                  // the pad samples of this run are skipped
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = i0; i < r; ++i) (void)ld_step(kw, (double)xr[i], s);
#pragma unroll
    for (int c = 0; c < 4; ++c) sv[4 * tid + c] = s[c];
    // Kogge-Stone: after step k, s is the zero-state state at the end of run tid counted from run max(0, tid - 2^(k+1) + 1)
    for (int k = 0; k < 8; ++k) {                                  // (uniform)
        const int d = 1 << k;
        double p[4] = {0.0, 0.0, 0.0, 0.0};
        __syncthreads();
        if (tid >= d) {
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = sv[4 * (tid - d) + c];
        }
        __syncthreads();
        if (tid >= d) {
            ld_matvec_add(tab + LD_TAB_P + 16 * k, p, s);
#pragma unroll
            for (int c = 0; c < 4; ++c) sv[4 * tid + c] = s[c];
        }
    }
    if (!FINAL) {
        if (tid == LD_NT - 1) {
            double* q = ld_ws_q(ws, B, U, b) + 4 * (size_t)u;
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = s[c];
        }
        return;
    }
    __syncthreads();
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) st[c] = sv[4 * (tid - 1) + c];
    }
    {
        const double* sin_ = ld_ws_s(ws, B, U, b) + 4 * (size_t)u;
        const double s_in[4] = {sin_[0], sin_[1], sin_[2], sin_[3]};
        ld_matvec_add(tab + LD_TAB_T + 16 * tid, s_in, st);
    }
    double acc = 0.0;
    for (int i = i0; i < r; ++i) { const double y = ld_step(kw, (double)xr[i], st); acc = fma(y, y, acc); }
    acc = ld_wave_sum(acc);
    if (lane == 0) s_d[wave] = acc;
    __syncthreads();
    if (tid == 0) hop_energy[(size_t)b * H_pad + u] = (float)((s_d[0] + s_d[1]) + (s_d[2] + s_d[3]));
}

// one wave per utterance: S[0] = 0, S[h + 1] = A^hop S[h] + Q[h], for h < H
__global__ __launch_bounds__(ST_WAVE) void loud_carry_kernel(LoudMeta meta, int hop, const double* __restrict__ tab, double* ws, int U) {
    __shared__ double q[LD_CARRY_CHUNK * 4];
    __shared__ double so[LD_CARRY_CHUNK * 4];
    const int b = blockIdx.x, B = gridDim.x, lane = threadIdx.x;
    const int H = meta.len[b] / hop;
    const double* Q = ld_ws_q(ws, B, U, b);
    double* S = ld_ws_s(ws, B, U, b);
    double Ah[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Ah[i] = tab[LD_TAB_AH + i];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int h0 = 0; h0 < H; h0 += LD_CARRY_CHUNK) {               // (uniform)
        const int n = min(LD_CARRY_CHUNK, H - h0);
        for (int i = lane; i < 4 * n; i += ST_WAVE) q[i] = Q[4 * (size_t)h0 + i];
        __syncthreads();
        if (lane == 0) {
            for (int h = 0; h < n; ++h) {
                double nx[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) { so[4 * h + c] = s[c]; nx[c] = q[4 * h + c]; }
                ld_matvec_add(Ah, s, nx);
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = nx[c];
            }
        }
        __syncthreads();
        for (int i = lane; i < 4 * n; i += ST_WAVE) S[4 * (size_t)h0 + i] = so[i];
        __syncthreads();
    }
}

__device__ __forceinline__ double ld_lkfs(double z) { return -0.691 + 10.0 * log10(z); }

// one workgroup per utterance
__global__ __launch_bounds__(LD_NT) void loud_gate_kernel(const float* __restrict__ hop_energy, LoudMeta meta, int hop, double* ws, int U, int H_pad,
                                                          double target, double peak_db, double max_gain_db, float* __restrict__ stats,
                                                          int32_t* __restrict__ counts) {
    __shared__ double s_d[LD_NW];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
    const int L = meta.len[b];
    const int H = L / hop, nb = max(H - 3, 0);
    const int units = (int)(((long)L + hop - 1) / hop);
    const double* pk = ld_ws_pk(ws, B, U, b);
    const float* e = hop_energy + (size_t)b * H_pad;
    double m = 0.0, nanc = 0.0;
    for (int u = tid; u < units; u += LD_NT) { const double v = pk[u]; if (v != v) nanc = 1.0; else m = fmax(m, v); }
    const double peak = ld_block_max(m, s_d);
    const bool bad = ld_block_max(nanc, s_d) > 0.0;
    float* sb = stats + 8 * (size_t)b;
    int32_t* cb = counts + 4 * (size_t)b;
    if (bad || nb == 0) {                                          // (uniform) flag 1: a non-finite sample; flag 2: no block
        if (tid == 0) {
            sb[0] = NAN; sb[1] = NAN; sb[2] = NAN; sb[3] = bad ? NAN : (float)peak; sb[4] = NAN; sb[5] = 1.0f; sb[6] = 0.0f; sb[7] = 0.0f;
            cb[0] = nb; cb[1] = 0; cb[2] = 0; cb[3] = bad ? 1 : 2;
        }
        return;
    }
    const double den = 4.0 * (double)hop;
    auto block_z = [&](int j) -> double { return (((double)e[j] + (double)e[j + 1]) + ((double)e[j + 2] + (double)e[j + 3])) / den; };
    double sum_all = 0.0, sum_a = 0.0, n_a = 0.0, lmax = -INFINITY;
    for (int j = tid; j < nb; j += LD_NT) {
        const double z = block_z(j), l = ld_lkfs(z);
        sum_all += z;
        lmax = fmax(lmax, l);
        if (l > -70.0) { sum_a += z; n_a += 1.0; }
    }
    sum_all = ld_block_sum(sum_all, s_d);
    sum_a = ld_block_sum(sum_a, s_d);
    n_a = ld_block_sum(n_a, s_d);                                  // (counts below 2^53 are exact in a double)
    lmax = ld_block_max(lmax, s_d);
    const double ungated = ld_lkfs(sum_all / (double)nb);
    if (n_a == 0.0) {                                              // (uniform) flag 4: nothing above the absolute gate
        if (tid == 0) {
            sb[0] = -INFINITY; sb[1] = (float)lmax; sb[2] = -INFINITY; sb[3] = (float)peak; sb[4] = (float)ungated; sb[5] = 1.0f;
            sb[6] = 0.0f; sb[7] = 0.0f;
            cb[0] = nb; cb[1] = 0; cb[2] = 0; cb[3] = 4;
        }
        return;
    }
    const double gate = ld_lkfs(sum_a / n_a) - 10.0;
    double sum_r = 0.0, n_r = 0.0;
    for (int j = tid; j < nb; j += LD_NT) {
        const double z = block_z(j), l = ld_lkfs(z);
        if (l > -70.0 && l > gate) { sum_r += z; n_r += 1.0; }
    }
    sum_r = ld_block_sum(sum_r, s_d);
    n_r = ld_block_sum(n_r, s_d);                                  // >= 1: the loudest block of A lies above A's mean - 10
    if (tid == 0) {
        const double li = ld_lkfs(sum_r / n_r);
        double g = 1.0;
        int flags = 0;
        if (target == target) {                                    // NaN: measure only
            const double g0 = exp10((target - li) / 20.0), gp = exp10(peak_db / 20.0) / peak, gm = exp10(max_gain_db / 20.0);
            g = fmin(g0, fmin(gp, gm));
            if (gp < g0 && gp <= gm) flags = 8;                    // the limit that binds (the peak ceiling on a tie)
            else if (gm < g0) flags = 16;
        }
        sb[0] = (float)li; sb[1] = (float)lmax; sb[2] = (float)gate; sb[3] = (float)peak; sb[4] = (float)ungated; sb[5] = (float)g;
        sb[6] = 0.0f; sb[7] = 0.0f;
        cb[0] = nb; cb[1] = (int32_t)n_a; cb[2] = (int32_t)n_r; cb[3] = flags;
    }
}

// grid (chunks, B); x and out_f32 may be the same buffer
__global__ __launch_bounds__(LD_NT) void wave_gain_kernel(const float* x, LoudMeta meta, const float* __restrict__ stats, float* out_f32,
                                                          int16_t* __restrict__ out_i16) {
    const int b = blockIdx.y;
    const int L = meta.len[b];
    const long off = meta.off[b];
    const float g = stats[8 * (size_t)b + 5];
    for (long i = (long)blockIdx.x * LD_NT + threadIdx.x; i < L; i += (long)gridDim.x * LD_NT) {
        const float v = __fmul_rn(x[off + i], g);
        if (out_f32) out_f32[off + i] = v;
        if (out_i16) out_i16[off + i] = (int16_t)rint(fmin(fmax((double)v, -1.0), 1.0) * 32767.0);
    }
}

int loud_meta(const st_wave_batch* w, LoudMeta& meta, const char* who) {
    ST_CHECK_ARG(w && w->x && w->off && w->len, "%s: null pointer", who);
    ST_CHECK_ARG(w->B >= 1 && w->B <= LD_MAX_B, "%s: batch %d outside [1, %d]", who, w->B, LD_MAX_B);
    memset(&meta, 0, sizeof(meta));
    for (int b = 0; b < w->B; ++b) {
        ST_CHECK_ARG(w->len[b] >= 1 && w->off[b] >= 0 && w->off[b] + w->len[b] <= w->n_samples, "%s: utterance %d [%ld, +%d) outside the %ld samples", who,
                     b, w->off[b], w->len[b], w->n_samples);
        meta.off[b] = w->off[b];
        meta.len[b] = w->len[b];
    }
    return 0;
}

}  // namespace

extern "C" int st_loudness_run_length(int fs) {
    if (fs < LD_MIN_FS || fs > LD_MAX_FS) return 0;
    return ((fs + 5) / 10 + LD_NT - 1) / LD_NT;
}

extern "C" int st_loudness_batch(const st_wave_batch* w, int fs, const double* tables, double target, double peak_db, double max_gain_db,
                                 float* hop_energy, int H_pad, float* stats, int32_t* counts, double* ws, void* stream) {
    (void)hipGetLastError();
    LoudMeta meta;
    const int rc = loud_meta(w, meta, "st_loudness_batch");
    if (rc) return rc;
    ST_CHECK_ARG(tables && stats && counts && ws && (hop_energy || H_pad == 0), "st_loudness_batch: null pointer");
    ST_CHECK_ARG(fs >= LD_MIN_FS && fs <= LD_MAX_FS, "st_loudness_batch: sample rate %d outside [%d, %d]", fs, LD_MIN_FS, LD_MAX_FS);
    ST_CHECK_ARG(__builtin_isfinite(peak_db) && __builtin_isfinite(max_gain_db), "st_loudness_batch: peak_db %g and max_gain_db %g must be finite", peak_db, max_gain_db);
    ST_CHECK_ARG(!__builtin_isinf(target), "st_loudness_batch: target %g must be finite, or NaN to measure only", target);
    const int hop = (fs + 5) / 10, r = (hop + LD_NT - 1) / LD_NT;  // r <= LD_MAX_R by the rate limit
    long hmax = 0, umax = 0;
    for (int b = 0; b < w->B; ++b) {
        hmax = max(hmax, (long)(meta.len[b] / hop));
        umax = max(umax, ((long)meta.len[b] + hop - 1) / hop);
    }
    ST_CHECK_ARG(H_pad >= hmax, "st_loudness_batch: H_pad %d below the %ld hops of the longest utterance", H_pad, hmax);
    const int U = H_pad + 1;                                       // umax <= hmax + 1 <= U
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loud_hop_kernel<false>, dim3((unsigned)umax, w->B), dim3(LD_NT), 0, st, w->x, meta, hop, r, tables, ws, U, hop_energy, H_pad);
    ST_LAUNCH_CHECK();
    if (H_pad > 0) {
        hipLaunchKernelGGL(loud_carry_kernel, dim3(w->B), dim3(ST_WAVE), 0, st, meta, hop, tables, ws, U);
        ST_LAUNCH_CHECK();
        hipLaunchKernelGGL(loud_hop_kernel<true>, dim3((unsigned)H_pad, w->B), dim3(LD_NT), 0, st, w->x, meta, hop, r, tables, ws, U, hop_energy, H_pad);
        ST_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(loud_gate_kernel, dim3(w->B), dim3(LD_NT), 0, st, hop_energy, meta, hop, ws, U, H_pad, target, peak_db, max_gain_db, stats, counts);
    ST_LAUNCH_CHECK();
    return 0;
}

extern "C" int st_wave_gain(const st_wave_batch* w, const float* stats, float* out_f32, int16_t* out_i16, void* stream) {
    (void)hipGetLastError();
    LoudMeta meta;
    const int rc = loud_meta(w, meta, "st_wave_gain");
    if (rc) return rc;
    ST_CHECK_ARG(stats && (out_f32 || out_i16), "st_wave_gain: null pointer");
    int lmax = 1;
    for (int b = 0; b < w->B; ++b) lmax = max(lmax, meta.len[b]);
    const unsigned chunks = (unsigned)min(1024L, ((long)lmax + 4 * LD_NT - 1) / (4 * LD_NT));
    hipLaunchKernelGGL(wave_gain_kernel, dim3(chunks, w->B), dim3(LD_NT), 0, (hipStream_t)stream, w->x, meta, stats, out_f32, out_i16);
    ST_LAUNCH_CHECK();
    return 0;
}
